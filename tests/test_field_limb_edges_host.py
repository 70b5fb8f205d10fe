"""The device field arithmetic (snarkvm_amd/csrc/ff.hip.h, the square roots of serde.hip.h) compiled for the host, on operands chosen as internal
29-bit limb patterns (tests/helpers/limb_cases.py): every ordered pair of the list through add / sub / mul / op 9 / the lazy chain, every element
through the unary operations, the four-operand diff_of_products with all three branches of its correction counted, Fq2, and the square roots -
all exact against Python integers.  The host twin covers every operation of the hook, square roots included.  No GPU needed; the same cases run
on the device in tests/test_gpu_field_limb_edges.py."""
import numpy as np
import pytest

from tests.helpers import field_edge_checks as fc
from tests.helpers import limb_cases as lc

RUN = fc.Runner(device=False)


@pytest.mark.parametrize("field", [0, 1])
def test_limb_case_list_is_what_it_claims(field):
    c = lc.cases(field)
    f = c.field
    assert len(set(c.internal)) == len(c.internal) and all(0 <= v < f.p for v in c.internal)
    assert [lc.to_internal(f, m) for m in c.mem] == c.internal
    have = set(c.internal)
    top = f.p >> (29 * (f.N - 1))
    for v in (0, 1, 2, f.p - 1, f.p - 2, (f.p - 1) // 2, (f.p + 1) // 2, pow(2, 29 * f.N, f.p)):
        assert v in have
    for k in range(f.N):
        assert 1 << (29 * k) in have and f.p - (1 << (29 * k)) in have and (k == 0 or (1 << (29 * k)) - 1 in have)
        for v in (1 << (29 * k + 28), lc.FULL << (29 * k)):
            assert (v in have) == (v < f.p)
    ones = lc.from_limbs29([lc.FULL] * (f.N - 1) + [top - 1])
    assert ones in have and ones >> (29 * (f.N - 1)) == top - 1 and ones + (1 << (29 * (f.N - 1))) >= f.p  # the largest such value
    partners = 0
    for a in c.internal:
        if {f.p - a, f.p - a - 1, f.p - a + 1, a + 1} <= have:
            partners += 1
    assert partners >= 4
    assert (len(c.internal) >= 120) if field == 1 else (len(c.internal) >= 80)
    assert c.a.shape[0] == len(c.internal) ** 2 and np.array_equal(c.a[1], c.arr[0]) and np.array_equal(c.b[1], c.arr[1])


@pytest.mark.parametrize("field", [0, 1])
def test_binary_ops_on_every_ordered_pair(field):
    fc.check_binary_ops(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_add_sub_neg_dbl_mul_leave_canonical_internal_limbs(field):
    fc.check_raw_internal_limbs(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_unary_ops_on_every_element(field):
    fc.check_unary_ops(RUN, field)


@pytest.mark.parametrize("field", [0, 1])
def test_diff_of_products_four_operands_all_correction_branches(field):
    neg, mid, hi = fc.check_diff_of_products(RUN, field)
    print(f"field {field}: T < 0: {neg}, 0 <= T < p: {mid}, T >= p: {hi}")


def test_fq2_mul_sqr_inverse_diff_of_products():
    fc.check_fq2(RUN)


def test_fq_sqrt_every_two_adic_order(golden):
    fc.check_fq_sqrt(RUN, golden)


def test_fq2_sqrt_every_branch():
    fc.check_fq2_sqrt(RUN)


def test_hook_refuses_bad_arguments():
    from snarkvm_amd import _lib

    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint64)
    assert L.snarkvm_hip_selftest_field_ext(10, buf.ctypes.data, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_field_ext(-1, buf.ctypes.data, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_field_ext(0, None, buf.ctypes.data, 1) == 1
    assert L.snarkvm_hip_selftest_field_ext(0, None, None, 0) == 0
