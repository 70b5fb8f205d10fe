"""`snarkvm_hip_fr_reduce` and `snarkvm_hip_fr_support` without a GPU (include/snarkvm_hip.h): the per-thread accumulation of
fr_reduce_kernel / fr_support_kernel (csrc/poly.hip.h: fr_reduce_thread over Fp::sum_of_products, fr_support_thread), the combine steps and the
two-launch shape run on the CPU through snarkvm_hip_selftest_fr_reduce / _fr_support over a given launch geometry.  Every Fr comparison is
bit-exact against Python big-int sums of the oracle's `to_bigint` values (tests/helpers/reduce_cases.py): Fr elements have one representation,
so the summation order cannot show.  Support triples are compared with numpy on the same vector.
"""
import numpy as np
import pytest

from snarkvm_amd import _lib, fft, plugin, poly
from tests.helpers import reduce_cases as rc

LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1031]
GEOMETRIES = [(1, 64), (1, 256), (3, 256), (8, 256)]  # 8 x 256 > 1031: idle threads, and for the short lengths idle workgroups
INVALID_VALUE = 1  # hipErrorInvalidValue


@pytest.mark.parametrize("blocks,threads", GEOMETRIES)
@pytest.mark.parametrize("n", LENGTHS)
def test_sum_and_inner_product(n, blocks, threads):
    a, b = rc.mixed(n, 1), rc.mixed(n, 3)
    assert np.array_equal(rc.selftest_reduce(rc.SUM, a, None, n, blocks, threads), rc.expected(rc.SUM, a)), "sum"
    assert np.array_equal(rc.selftest_reduce(rc.DOT, a, b, n, blocks, threads), rc.expected(rc.DOT, a, b)), "dot"
    assert np.array_equal(rc.selftest_reduce(rc.DOT, a, a, n, blocks, threads), rc.expected(rc.DOT, a, a)), "a == b"


def test_the_device_geometry():
    g = rc.geometry(1)
    assert g["blocks"] == 1 and g["threads"] in (64, 128, 256) and 1 <= g["G"] <= 6 and g["cap"] >= 1
    cap = g["cap"] * g["threads"]
    assert rc.geometry(cap)["blocks"] == g["cap"] and rc.geometry(cap + 3)["blocks"] == g["cap"]  # capped: the stride loop takes the rest
    assert rc.geometry(g["threads"] + 1)["blocks"] == 2
    assert rc.geometry(0)["blocks"] == 1


@pytest.mark.parametrize("kind", ["max", "rawmax"])
def test_largest_column_sums_around_the_group_size(kind):
    """every term (r-1) * (r-1) - and both memory images the integer r - 1 - in per-thread runs of 1, G-1, G, G+1 and 2G+1 terms: whole groups
    of sum_of_products with nothing behind them, one short of a group, and single terms behind one and two groups"""
    G = rc.geometry(1)["G"]
    for run in sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1}):
        for blocks, threads in ((1, 64), (3, 256)):
            n = run * blocks * threads  # every thread owns exactly `run` terms
            a, b = rc.max_terms(n, kind)
            assert np.array_equal(rc.selftest_reduce(rc.DOT, a, b, n, blocks, threads), rc.expected(rc.DOT, a, b)), (run, blocks, threads)
            assert np.array_equal(rc.selftest_reduce(rc.SUM, a, None, n, blocks, threads), rc.expected(rc.SUM, a)), (run, blocks, threads)


def test_special_operands():
    """0, 1, 2, r-1, r-2, (r+-1)/2 against each other in every pairing"""
    n = 7 * 7 * 3
    a = rc.special(n)
    b = rc.special(7, 0)[(np.arange(n) // 7) % 7]
    for blocks, threads in GEOMETRIES:
        assert np.array_equal(rc.selftest_reduce(rc.DOT, a, b, n, blocks, threads), rc.expected(rc.DOT, a, b))
        assert np.array_equal(rc.selftest_reduce(rc.SUM, a, None, n, blocks, threads), rc.expected(rc.SUM, a))


@pytest.mark.parametrize("blocks,threads", GEOMETRIES)
def test_support_placements(blocks, threads):
    n = 257
    for name, v in rc.support_cases(n).items():
        assert rc.selftest_support(v, n, blocks, threads) == rc.expected_support(v), name


@pytest.mark.parametrize("n", LENGTHS)
def test_support_lengths(n):
    v = rc.mixed(n, 4)
    if n > 2:
        v[0] = v[n - 1] = 0  # neither end counts
    for blocks, threads in GEOMETRIES:
        assert rc.selftest_support(v, n, blocks, threads) == rc.expected_support(v), (blocks, threads)


def test_selftests_refuse_bad_arguments():
    L = _lib.lib()
    a = rc.rnd(4, 1)
    out = np.full((1, 4), rc.GUARD, dtype=np.uint64)
    o3 = np.full(3, rc.GUARD, dtype=np.uint64)
    assert L.snarkvm_hip_selftest_fr_reduce(2, out.ctypes.data, a.ctypes.data, a.ctypes.data, 4, 1, 64) == -1   # unknown op
    assert L.snarkvm_hip_selftest_fr_reduce(0, None, a.ctypes.data, None, 4, 1, 64) == -1                       # no result
    assert L.snarkvm_hip_selftest_fr_reduce(0, out.ctypes.data, None, None, 4, 1, 64) == -1                     # no a
    assert L.snarkvm_hip_selftest_fr_reduce(1, out.ctypes.data, a.ctypes.data, None, 4, 1, 64) == -1            # no b for an inner product
    assert L.snarkvm_hip_selftest_fr_reduce(0, out.ctypes.data, a.ctypes.data, None, 4, 0, 64) == -1            # no workgroup
    assert L.snarkvm_hip_selftest_fr_reduce(0, out.ctypes.data, a.ctypes.data, None, 4, 1, 96) == -1            # not 1, 2 or 4 waves
    assert L.snarkvm_hip_selftest_fr_support(o3.ctypes.data, None, 4, 1, 64) == -1
    assert L.snarkvm_hip_selftest_fr_support(None, a.ctypes.data, 4, 1, 64) == -1
    assert L.snarkvm_hip_selftest_fr_support(o3.ctypes.data, a.ctypes.data, 4, 1, 100) == -1
    assert (out == rc.GUARD).all() and (o3 == rc.GUARD).all()


# ---- the ABI itself, as far as it goes without a device ------------------------------------------------------------------
def _refused(err):
    with pytest.raises(_lib.HipError) as e:
        _lib.check(err)
    assert e.value.code == INVALID_VALUE and e.value.message, e.value


def test_argument_validation_fails_before_any_device_is_needed():
    L = _lib.lib()
    a = rc.rnd(4, 1)
    pa = a.ctypes.data
    out = np.full((3, 4), rc.GUARD, dtype=np.uint64)
    o3 = np.full(9, rc.GUARD, dtype=np.uint64)
    for on_device in (0, 1):
        _refused(L.snarkvm_hip_fr_reduce(2, out.ctypes.data, pa, pa, 4, on_device))    # unknown op
        _refused(L.snarkvm_hip_fr_reduce(-1, out.ctypes.data, pa, pa, 4, on_device))
        _refused(L.snarkvm_hip_fr_reduce(0, None, pa, None, 4, on_device))             # null result
        _refused(L.snarkvm_hip_fr_reduce(0, out.ctypes.data, None, None, 4, on_device))  # null a with n > 0
        _refused(L.snarkvm_hip_fr_reduce(1, out.ctypes.data, pa, None, 4, on_device))  # null b for op 1
        _refused(L.snarkvm_hip_fr_support(None, pa, 4, on_device))
        _refused(L.snarkvm_hip_fr_support(o3.ctypes.data, None, 4, on_device))
    _refused(L.snarkvm_hip_fr_reduce_strided(2, out.ctypes.data, pa, pa, 1, 3, 1, 0))
    _refused(L.snarkvm_hip_fr_reduce_strided(0, None, pa, None, 1, 3, 1, 0))
    _refused(L.snarkvm_hip_fr_reduce_strided(0, out.ctypes.data, None, None, 1, 3, 1, 0))
    _refused(L.snarkvm_hip_fr_reduce_strided(1, out.ctypes.data, pa, None, 1, 3, 1, 1))
    _refused(L.snarkvm_hip_fr_reduce_strided(0, out.ctypes.data, pa, None, 2, 2, 1, 0))  # stride < n
    _refused(L.snarkvm_hip_fr_support_strided(None, pa, 1, 3, 1))
    _refused(L.snarkvm_hip_fr_support_strided(o3.ctypes.data, None, 1, 3, 1))
    _refused(L.snarkvm_hip_fr_support_strided(o3.ctypes.data, pa, 2, 2, 1))            # stride < n
    assert (out == rc.GUARD).all() and (o3 == rc.GUARD).all()


def test_empty_input_needs_no_device():
    L = _lib.lib()
    a = rc.rnd(4, 1)
    for on_device in (0, 1):
        for op in (rc.SUM, rc.DOT):
            out = np.full((2, 4), rc.GUARD, dtype=np.uint64)
            _lib.check(L.snarkvm_hip_fr_reduce(op, out.ctypes.data, a.ctypes.data, a.ctypes.data, 0, on_device))
            assert not out[0].any() and (out[1] == rc.GUARD).all()
            _lib.check(L.snarkvm_hip_fr_reduce(op, out.ctypes.data, None, None, 0, on_device))  # a pointer may be null iff n == 0
        o3 = np.full(4, rc.GUARD, dtype=np.uint64)
        _lib.check(L.snarkvm_hip_fr_support(o3.ctypes.data, None, 0, on_device))
        assert o3[:3].tolist() == [0, 0, 0] and o3[3] == rc.GUARD
    out = np.full((4, 4), rc.GUARD, dtype=np.uint64)
    _lib.check(L.snarkvm_hip_fr_reduce_strided(rc.DOT, out.ctypes.data, None, None, 0, 3, 0, 0))
    assert not out[:3].any() and (out[3] == rc.GUARD).all()
    o3 = np.full(10, rc.GUARD, dtype=np.uint64)
    _lib.check(L.snarkvm_hip_fr_support_strided(o3.ctypes.data, None, 0, 3, 0))
    assert not o3[:9].any() and o3[9] == rc.GUARD
    # count == 0: a no-op success, whatever else is passed
    _lib.check(L.snarkvm_hip_fr_reduce_strided(7, None, None, None, 5, 0, 0, 0))
    _lib.check(L.snarkvm_hip_fr_support_strided(None, None, 5, 0, 0))
    # the Python layer
    assert not poly.inner_product(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)).any()
    assert not poly.vec_sum(np.zeros((0, 4), dtype=np.uint64)).any()
    assert poly.support(np.zeros((0, 4), dtype=np.uint64)) == (0, 0, 0)
    assert not plugin.fr_reduce_device(plugin.FR_REDUCE_DOT, 0, 0, 0).any()
    assert plugin.fr_support_device(0, 0).tolist() == [0, 0, 0]
    assert plugin.fr_reduce_strided_device(plugin.FR_REDUCE_SUM, 0, 0, 0, 2, 0).shape == (2, 4)
    assert plugin.fr_support_strided_device(0, 0, 2, 0).shape == (2, 3)


def test_python_layer_checks_lengths_before_ffi():
    with pytest.raises(ValueError):
        poly.inner_product(rc.rnd(4, 1), rc.rnd(5, 2))  # zip_eq
    with pytest.raises(ValueError):
        fft.Evaluations(rc.rnd(8, 1), fft.EvaluationDomain.new(8)).evaluate_with_coeffs(rc.rnd(7, 2))


def test_a_host_pointer_passed_as_device_memory_fails_loudly():
    """Without a GPU there is no device to run on; with one, host memory belongs to none: a non-zero code and a message either way"""
    a = rc.rnd(4, 1)
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_reduce_device(plugin.FR_REDUCE_SUM, a.ctypes.data, 0, 4)
    assert e.value.code != 0 and e.value.message
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_support_device(a.ctypes.data, 4)
    assert e.value.code != 0 and e.value.message
