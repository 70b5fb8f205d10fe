"""`snarkvm_hip_fr_open_fold` without a GPU (include/snarkvm_hip.h): the per-thread routines of the fused sweeps (csrc/poly.hip.h:
fr_lincomb_at, the walks of fr_span_fold_t and fr_span_plain_t, the span, scan and carry routines of the scaffolds) and the host-side bookkeeping of the call -
validation, longest-first order, the split into tables of FR_LINCOMB_CHUNK operands, the choice of the route - run on the CPU through
snarkvm_hip_selftest_fr_open_fold, which replays the launch plan over a given geometry.  Every comparison is bit-exact against the oracle
(tests/helpers/open_fold_cases.py): its AXPY chain for the combination, poly_divide by X - z for the quotient, poly_evaluate for the value.
"""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin, sonic_pc
from tests import util
from tests.helpers import lincomb as lc
from tests.helpers import open_fold_cases as oc

GUARD = oc.GUARD


def check(coeffs, polys, z, n, quot, value, geo=None, want="qr"):
    got_q, got_v = oc.run_host(coeffs, polys, z, n, geo, want)
    if "q" in want:
        assert np.array_equal(got_q, quot), (n, geo)
        assert not got_q[n - 1].any()
    if "r" in want:
        assert np.array_equal(got_v, value), (n, geo)


# ---- lengths at every ownership edge, over the geometry the device call launches ------------------------------------------------
def geo3(n):
    return oc.geometry(n)[:3]


def test_the_default_geometry_is_the_route_of_divide_by_linear():
    assert geo3(1) == (0, 32, 1) and geo3(2047) == (0, 32, 1)
    assert geo3(2048) == (1, 8, 1) and geo3(2049) == (1, 8, 2)
    assert geo3(3 * 2048 + 1) == (1, 8, 4)
    assert geo3(1 << 19) == (1, 8, 256) and geo3((1 << 19) + 1) == (1, 16, 129)
    assert geo3(1 << 20) == (1, 16, 256) and geo3((1 << 20) + 1) == (0, 32, 129)  # 32769 chunks
    # 24 operands per table; the fused sweep takes one term: a single member, or the sum the fr_lincomb launches have parked in the quotient
    assert oc.geometry(1)[3:] == (oc.CHUNK, 1) and oc.CHUNK == plugin.FR_LINCOMB_CHUNK == 24


@pytest.mark.parametrize("n", oc.SMALL_LENGTHS)
def test_lengths_small(n):
    coeffs, polys, z, quot, value = oc.case(n, 7, n % 5)
    check(coeffs, polys, z, n, quot, value)
    check(coeffs, polys, z, n, quot, value, want="r")  # the value alone: always the recursion


@pytest.mark.parametrize("n", oc.LARGE_LENGTHS)
def test_lengths_large(n):
    coeffs, polys, z, quot, value = oc.case(n, 3)  # lengths n, 0, 1
    check(coeffs, polys, z, n, quot, value)


# ---- explicit geometries: several workgroups at small n -------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,blocks", [(1, 1, 1), (255, 1, 1), (256, 1, 1), (257, 1, 2), (300, 1, 2), (512, 1, 2), (513, 1, 3), (600, 1, 3), (600, 2, 2),
                                        (1025, 2, 3), (1537, 3, 3), (600, 5, 1), (300, 1, 4), (259, 1, 257), (2100, 8, 2), (2100, 64, 1)])
def test_scan_route_under_forced_geometries(n, C, blocks):
    """C coefficients per thread, `blocks` workgroups of 256 threads: a workgroup's last and first thread, a lone coefficient in a workgroup,
    workgroups past the end that own nothing, and as many workgroups (257) as the carry of the first one has terms"""
    coeffs, polys, z, quot, value = oc.case(n, 7, 2)
    check(coeffs, polys, z, n, quot, value, (1, C, blocks))


@pytest.mark.parametrize("n,C", [(1, 2), (2, 2), (3, 2), (9, 2), (33, 2), (27, 3), (28, 3), (130, 5), (1025, 32), (70000, 16)])
def test_recursion_under_forced_chunk_sizes(n, C):
    """chunks of C coefficients at every level: more levels at a small n than POLY_CHUNK = 32 reaches below 2^15 coefficients"""
    coeffs, polys, z, quot, value = oc.case(n, 5, 3)
    geo = (0, C, ((n + C - 1) // C + 255) // 256)
    check(coeffs, polys, z, n, quot, value, geo)
    check(coeffs, polys, z, n, quot, value, geo, want="r")


def test_refused_geometries():
    coeffs, polys, z, _, _ = oc.case(600, 5, 3)
    ptrs, lens = [p.ctypes.data for p in polys], [len(p) for p in polys]
    quot = np.full((600, 4), GUARD, dtype=np.uint64)
    rem = np.full((1, 4), GUARD, dtype=np.uint64)
    for geo in [(1, 1, 2), (1, 0, 3), (1, 1, 258), (2, 8, 1), (-1, 8, 1), (0, 1, 3), (0, 32, 2), (0, 32, 0)]:
        assert oc.selftest(quot, rem, 600, ptrs, lens, coeffs, z, geo) == -1, geo
    assert oc.selftest(None, rem, 600, ptrs, lens, coeffs, z, (1, 1, 3)) == -1  # the scan route needs the quotient buffer
    assert (quot == GUARD).all() and (rem == GUARD).all()


# ---- member lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", oc.COUNTS)
def test_counts_and_ragged_lengths(count):
    """every group size, a short last group, one, two and three tables; lengths 0, 1, n - 1, n and between; on both routes, and the value alone
    (one up sweep per table, the values added)"""
    for n in (2050, 40):
        coeffs, polys, z, quot, value = oc.case(n, count, count % 5)
        check(coeffs, polys, z, n, quot, value)
        check(coeffs, polys, z, n, quot, value, want="r")
        check(coeffs, polys, z, n, quot, value, want="q")


@pytest.mark.parametrize("count", [2, oc.CHUNK + 1])
def test_the_longest_member_is_shorter_than_n(count):
    """the trailing quotient elements are zeros, written"""
    for n, longest in ((2100, 1500), (50, 20)):
        coeffs, polys, z, quot, value = oc.case(n, count, 1, longest=longest)
        assert not quot[longest - 1 :].any() and quot[longest - 2].any()
        check(coeffs, polys, z, n, quot, value)


def test_the_same_operand_twice_and_overlapping_operands():
    p, q = lc.rnd(2100, 1), lc.rnd(700, 2)
    polys = [p, q, p, p[3:200], q[:7], p]
    coeffs, z = lc.rnd(6, 7), oc.point("random")
    _, quot, value = oc.reference(coeffs, polys, 2100, z)
    check(coeffs, polys, z, 2100, quot, value)


def test_everything_cancels():
    """coefficients (1, r - 1) over the same operand: a zero quotient and a zero remainder, all written"""
    coeffs = np.concatenate([sonic_pc.FR_ONE.reshape(1, 4), util.ints_to_fr_mont([lc.R - 1])])
    for n in (2100, 33):
        p = lc.rnd(n, 2)
        got_q, got_v = oc.run_host(coeffs, [p, p], oc.point("random"), n)
        assert not got_q.any() and not got_v.any()


# ---- values and points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", oc.KINDS)
def test_edge_values(kind):
    for n, count in ((2100, 7), (33, oc.CHUNK + 1)):
        coeffs, polys, z, quot, value = oc.case(n, count, 1, kind)
        check(coeffs, polys, z, n, quot, value)


@pytest.mark.parametrize("name", oc.POINTS)
def test_points(name):
    """0 (the quotient is the combination shifted down), 1, r - 1 (order 2), a random point, and an element of order 2048: with C = 8 the
    tables of m^(2048 j) of the scan route are all ones"""
    for n in (4097, 1025):
        coeffs, polys, z, quot, value = oc.case(n, 6, 2, "mixed", name)
        check(coeffs, polys, z, n, quot, value)
    if name == "zero":
        comb = lc.expected(coeffs, polys, n)
        assert np.array_equal(quot[: n - 1], comb[1:]) and np.array_equal(value, comb[:1])


# ---- outputs --------------------------------------------------------------------------------------------------------------------------
def test_remainder_only_writes_nothing_else():
    coeffs, polys, z, _, value = oc.case(2100, 7, 2)
    would_be = np.full((2100, 4), GUARD, dtype=np.uint64)
    rem = np.zeros((1, 4), dtype=np.uint64)
    assert oc.selftest(None, rem, 2100, [p.ctypes.data for p in polys], [len(p) for p in polys], coeffs, z) == 0
    assert np.array_equal(rem, value) and (would_be == GUARD).all()
    # neither output: validated, nothing to deliver
    assert oc.selftest(None, None, 2100, [p.ctypes.data for p in polys], [len(p) for p in polys], coeffs, z) == 0


def test_refused_arguments_leave_the_outputs_untouched():
    n = 64
    buf = np.full((4 * n, 4), GUARD, dtype=np.uint64)
    rem = np.full((1, 4), GUARD, dtype=np.uint64)
    p = lc.rnd(n, 1)
    c, z = lc.rnd(2, 7), oc.point("random")
    q = buf.ctypes.data + 32 * n
    L = _lib.lib()
    assert oc.selftest(q, rem, n, [p.ctypes.data], [n + 1], c[:1], z) == -1                        # an operand longer than n
    assert oc.selftest(q, rem, n, [p.ctypes.data, q], [n, n], c, z) == -1                          # the quotient IS an operand
    assert oc.selftest(q, rem, n, [p.ctypes.data, q - 32], [n, 2], c, z) == -1                     # an operand ending inside the quotient
    assert oc.selftest(q, rem, n, [p.ctypes.data, q + 32 * (n - 1)], [n, 9], c, z) == -1           # an operand starting inside the quotient
    pp, pl, cs, zz = oc.call_args([0], [0], c[:1], z)
    pl[0] = 4
    args = (ctypes.c_void_p(q), ctypes.c_void_p(rem.ctypes.data), n, 1)
    assert L.snarkvm_hip_selftest_fr_open_fold(*args, pp, pl, ctypes.c_void_p(cs.ctypes.data), ctypes.c_void_p(zz.ctypes.data), 0, 32, 1) == -1  # a missing pointer
    pp, pl, cs, zz = oc.call_args([p.ctypes.data], [n], c[:1], z)
    assert L.snarkvm_hip_selftest_fr_open_fold(*args, pp, pl, ctypes.c_void_p(cs.ctypes.data), None, 0, 32, 1) == -1                              # a missing point
    assert L.snarkvm_hip_selftest_fr_open_fold(*args, pp, pl, None, ctypes.c_void_p(zz.ctypes.data), 0, 32, 1) == -1                              # missing coeffs
    assert L.snarkvm_hip_selftest_fr_open_fold(*args, None, pl, ctypes.c_void_p(cs.ctypes.data), ctypes.c_void_p(zz.ctypes.data), 0, 32, 1) == -1  # a missing list
    assert (buf == GUARD).all() and (rem == GUARD).all()
    # adjacent is not overlapping: an operand that ends where the quotient begins, and one that begins where it ends
    buf[:n], buf[2 * n : 3 * n] = p, p
    assert oc.selftest(q, rem, n, [buf.ctypes.data, q + 32 * n], [n, n], c, z) == 0
    _, quot, value = oc.reference(c, [p, p], n, z)
    assert np.array_equal(buf[n : 2 * n], quot) and np.array_equal(rem, value)
    assert np.array_equal(buf[:n], p) and np.array_equal(buf[2 * n : 3 * n], p) and (buf[3 * n :] == GUARD).all()


def test_no_coefficients_and_no_operands():
    z = oc.point("random")
    rem = np.full((1, 4), GUARD, dtype=np.uint64)
    would_be = np.full((4, 4), GUARD, dtype=np.uint64)
    p = lc.rnd(4, 1)
    # n == 0: success, the remainder is zero, nothing else is touched - not even looked at
    assert oc.selftest(would_be, rem, 0, [p.ctypes.data], [4], lc.rnd(1, 7), z) == 0
    assert not rem.any() and (would_be == GUARD).all()
    for ptrs, lens, coeffs in (([], [], np.zeros((0, 4), dtype=np.uint64)), ([0, 0], [0, 0], lc.rnd(2, 7))):
        for n in (7, 2100):
            quot = np.full((n + 1, 4), GUARD, dtype=np.uint64)
            rem[:] = GUARD
            assert oc.selftest(quot, rem, n, ptrs, lens, coeffs, z) == 0
            assert not quot[:n].any() and (quot[n] == GUARD).all() and not rem.any()


# ---- the ABI itself, as far as it goes without a device -------------------------------------------------------------------------
def test_nothing_to_write_is_success_and_needs_no_device():
    assert not plugin.fr_open_fold_device(0, 0, [], [], np.zeros((0, 4), dtype=np.uint64), oc.point("one")).any()
    p = np.ones((4, 4), dtype=np.uint64)
    out = np.full((4, 4), 7, dtype=np.uint64)
    for on_device in (0, 1):
        rem = np.full((1, 4), GUARD, dtype=np.uint64)
        pp, pl, cs, zz = oc.call_args([p.ctypes.data], [0], lc.rnd(1, 7), oc.point("one"))
        _lib.check(_lib.lib().snarkvm_hip_fr_open_fold(out.ctypes.data, rem.ctypes.data, 0, 1, pp, pl, cs.ctypes.data, zz.ctypes.data, on_device))
        assert not rem.any()
    assert (out == 7).all()
    # host operands, only empty members: the zero combination needs no device either
    rem = np.full((1, 4), GUARD, dtype=np.uint64)
    pp, pl, cs, zz = oc.call_args([0, 0], [0, 0], lc.rnd(2, 7), oc.point("one"))
    _lib.check(_lib.lib().snarkvm_hip_fr_open_fold(out.ctypes.data, rem.ctypes.data, 4, 2, pp, pl, cs.ctypes.data, zz.ctypes.data, 0))
    assert not out.any() and not rem.any()


def test_a_host_pointer_passed_as_device_memory_fails_loudly():
    """Without a GPU there is no device to run on; with one, host memory belongs to none: a non-zero code and a message either way"""
    p = np.ones((4, 4), dtype=np.uint64)
    out = np.full((4, 4), 7, dtype=np.uint64)
    with pytest.raises(_lib.HipError) as e:
        plugin.fr_open_fold_device(out.ctypes.data, 4, [p.ctypes.data], [4], lc.rnd(1, 7), oc.point("one"))
    assert e.value.code != 0 and e.value.message
    assert (out == 7).all()


@pytest.mark.parametrize("on_device", [0, 1])
def test_refusals_come_from_the_argument_check_itself(on_device):
    p = np.ones((5, 4), dtype=np.uint64)
    out = np.full((5, 4), 7, dtype=np.uint64)
    rem = np.full((1, 4), 7, dtype=np.uint64)
    L = _lib.lib()
    pp, pl, cs, zz = oc.call_args([p.ctypes.data], [5], lc.rnd(1, 7), oc.point("one"))
    for why, call in (("longer than n", lambda: L.snarkvm_hip_fr_open_fold(out.ctypes.data, rem.ctypes.data, 4, 1, pp, pl, cs.ctypes.data, zz.ctypes.data, on_device)),
                      ("missing point", lambda: L.snarkvm_hip_fr_open_fold(out.ctypes.data, rem.ctypes.data, 5, 1, pp, pl, cs.ctypes.data, None, on_device)),
                      ("missing coeffs", lambda: L.snarkvm_hip_fr_open_fold(out.ctypes.data, rem.ctypes.data, 5, 1, pp, pl, None, zz.ctypes.data, on_device)),
                      ("overlaps", lambda: L.snarkvm_hip_fr_open_fold(p.ctypes.data, rem.ctypes.data, 5, 1, pp, pl, cs.ctypes.data, zz.ctypes.data, on_device))):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(call())
        assert e.value.code == oc.INVALID_VALUE and why in e.value.message, (why, e.value.message)
    assert (out == 7).all() and (rem == 7).all() and (p == 1).all()


# ---- the host arithmetic of the drivers --------------------------------------------------------------------------------------------
def test_the_fold_of_the_challenges_is_the_field_product():
    a, b = lc.rnd(40, 3), np.concatenate([lc.special(7), lc.rnd(33, 4)])
    want = oracle.fr_op("mul", a, b)
    for k in range(40):
        assert np.array_equal(sonic_pc._fr_mul(a[k], b[k]), want[k])


def test_resident_polynomial_vouches_for_its_length():
    p = sonic_pc.ResidentPolynomial("w", 0x1000, 300, degree_bound=299, hiding_bound=1)
    assert (p.ptr, p.n, p.degree(), p.is_hiding()) == (0x1000, 300, 299, True)
    sonic_pc.check_degrees_and_bounds(399, [299], p)
    with pytest.raises(sonic_pc.PCError, match="IncorrectDegreeBound"):
        sonic_pc.check_degrees_and_bounds(399, [200, 299], sonic_pc.ResidentPolynomial("w", 0x1000, 300, degree_bound=200))
    assert sonic_pc.ResidentPolynomial("z", 0, 0).degree() == 0
