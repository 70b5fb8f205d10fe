"""`snarkvm_hip_fr_witness_evals` and `snarkvm_hip_fr_rowcheck_fold` through their host replays (`snarkvm_hip_selftest_fr_witness_evals`,
`snarkvm_hip_selftest_fr_rowcheck_fold`: the same validation, member tables and split into launches, the CPU in the kernels' place through the
kernels' own per-index routines, csrc/poly.hip.h: fr_witness_at, fr_rowcheck_at) - no GPU needed.

Every comparison is bit for bit.  Expected values (tests/helpers/rowcheck_cases.py): the fold and the counts by per-element Python integers, the
gather by numpy indexing and the oracle's subtraction, the fixture's w_lde and h_0 from tests/golden/varuna_circuit0.json with every transform and
division on the C++ oracle.
"""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin
from tests import util
from tests.helpers import rowcheck_cases as rc

R = rc.R
GUARD = rc.GUARD
CHUNK = rc.CHUNK


def test_the_chunk_the_tests_are_sized_for():
    assert CHUNK == plugin.FR_ROWCHECK_CHUNK and 1 <= rc.geometry()[1] <= 3


# ---- the fold against per-element integers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", rc.COUNTS)
@pytest.mark.parametrize("n", rc.SIZES)
def test_fold_and_counts(n, count):
    """members that overlap each other and, from the 17th on, repeat; multipliers 0, 1 and r - 1 among them; 2 CHUNK + 1 members take three
    launches, the later ones adding to out"""
    arrays, ints = rc.members(n, count, n + count)
    mus, mu_ints = rc.multipliers(count, count)
    out, viol = rc.selftest_fold(arrays, mus, n)
    assert np.array_equal(out, rc.expected_fold(ints, mu_ints, n))
    assert viol == rc.expected_violations(ints)
    if count == 0:
        assert not out.any() and viol == []


def test_repeated_members_a_zero_multiplier_and_an_all_zero_a():
    n = 257
    (a, b, c), (ai, bi, ci) = rc.members(n, 5, 3)
    zero = np.zeros((n, 4), dtype=np.uint64)
    arrays = ([a[0], a[0], zero, a[3], a[0]], [b[0], b[0], b[2], b[3], b[0]], [c[0], c[0], c[2], c[3], c[0]])
    ints = ([ai[0], ai[0], [0] * n, ai[3], ai[0]], [bi[0], bi[0], bi[2], bi[3], bi[0]], [ci[0], ci[0], ci[2], ci[3], ci[0]])
    mu_ints = [5, R - 5, 7, 0, 11]
    out, viol = rc.selftest_fold(arrays, rc.mont(mu_ints), n)
    assert np.array_equal(out, rc.expected_fold(ints, mu_ints, n)) and viol == rc.expected_violations(ints)
    assert viol[0] == viol[1] == viol[4]
    # member 2 alone: a = 0, so out = -mu c
    out, _ = rc.selftest_fold(([zero], [b[2]], [c[2]]), rc.mont([7]), n)
    assert util.fr_mont_to_ints(out) == [(-7 * z) % R for z in ci[2]]


def test_special_operands_only():
    """operands only from {0, 1, r - 1, (r - 1) / 2, (r + 1) / 2}, every multiplier of {0, 1, r - 1}"""
    n = 65
    arrays = tuple([rc.special(n, 3 * k + j) for k in range(3)] for j in range(3))
    ints = tuple([util.fr_mont_to_ints(v) for v in vs] for vs in arrays)
    out, viol = rc.selftest_fold(arrays, rc.mont(rc.MULTIPLIERS), n)
    assert np.array_equal(out, rc.expected_fold(ints, rc.MULTIPLIERS, n)) and viol == rc.expected_violations(ints)


# ---- violations --------------------------------------------------------------------------------------------------------------------------------
def _spoil(arrays, ints, k, i):
    """c_k[i] += 1"""
    ints[2][k][i] = (ints[2][k][i] + 1) % R
    arrays[2][k][i] = rc.mont([ints[2][k][i]])[0]


@pytest.mark.parametrize("where", ["none", "first", "last", "second_launch", "whole_member"])
def test_violation_counts_are_exact_per_member(where):
    n, count = 257, CHUNK + 3
    arrays, ints = rc.valid_members(n, count, 7)
    want = [0] * count
    if where == "first":
        _spoil(arrays, ints, 2, 0), want.__setitem__(2, 1)
    elif where == "last":
        _spoil(arrays, ints, 5, n - 1), want.__setitem__(5, 1)
    elif where == "second_launch":
        _spoil(arrays, ints, CHUNK + 1, 100), want.__setitem__(CHUNK + 1, 1)
    elif where == "whole_member":
        for i in range(n):
            _spoil(arrays, ints, 1, i)
        want[1] = n
    mus, mu_ints = rc.multipliers(count, 8)
    out, viol = rc.selftest_fold(arrays, mus, n)
    assert viol == want == rc.expected_violations(ints)
    assert np.array_equal(out, rc.expected_fold(ints, mu_ints, n))
    if where == "none":
        assert not out.any()  # a b - c = 0 everywhere


# ---- skipped outputs ---------------------------------------------------------------------------------------------------------------------------
def test_a_null_output_is_skipped():
    n, count = 256, CHUNK + 1
    arrays, ints = rc.members(n, count, 11)
    mus, mu_ints = rc.multipliers(count, 11)
    out, viol = rc.selftest_fold(arrays, mus, n, want="o")
    assert viol is None and np.array_equal(out, rc.expected_fold(ints, mu_ints, n))
    out, viol = rc.selftest_fold(arrays, mus, n, want="v")
    assert out is None and viol == rc.expected_violations(ints)
    # the check alone needs no multipliers
    pa, pb, pc = rc.pointer_lists(arrays, n)
    v = rc.guarded(count, 1)
    assert _lib.lib().snarkvm_hip_selftest_fr_rowcheck_fold(None, v[1:].ctypes.data, n, count, pa, pb, pc, None) == 0
    assert [int(x) for x in rc.unguard(v, count)[:, 0]] == rc.expected_violations(ints)
    assert rc.selftest_fold(arrays, mus, n, want="") == (None, None)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_fold_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    n = 9
    arrays, ints = rc.members(n, 2, 5)
    (a, b, c) = arrays
    pa, pb, pc = rc.pointer_lists(arrays, n)
    mu = rc.rnd(2, 3)
    out, viol = rc.guarded(n), rc.guarded(2, 1)
    ptrs = lambda *xs: (ctypes.c_void_p * len(xs))(*xs)

    def refused(o=out[1:].ctypes.data, v=viol[1:].ctypes.data, n=n, count=2, a=pa, b=pb, c=pc, mus=mu.ctypes.data):
        assert L.snarkvm_hip_selftest_fr_rowcheck_fold(o, v, n, count, a, b, c, mus) == -1
        assert (out == GUARD).all() and (viol == GUARD).all()

    refused(n=(1 << 28) + 1)
    big = 65536
    refused(count=big, a=(ctypes.c_void_p * big)(), b=(ctypes.c_void_p * big)(), c=(ctypes.c_void_p * big)(), mus=np.zeros((big, 4), dtype=np.uint64).ctypes.data)
    refused(a=None), refused(b=None), refused(c=None), refused(mus=None)                      # NULL host arrays with count > 0
    refused(a=ptrs(a[0].ctypes.data, None)), refused(c=ptrs(None, c[1].ctypes.data))           # a NULL member pointer with n > 0
    whole = np.concatenate([a[0], np.full((n, 4), GUARD, dtype=np.uint64)])                    # out directly behind a member is fine, one earlier is not
    wa = ptrs(whole.ctypes.data, a[1].ctypes.data)
    assert L.snarkvm_hip_selftest_fr_rowcheck_fold(whole[n - 1 :].ctypes.data, None, n, 2, wa, pb, pc, mu.ctypes.data) == -1
    assert np.array_equal(whole[:n], a[0]) and (whole[n:] == GUARD).all()
    refused(o=b[1][n - 1 :].ctypes.data), refused(o=c[0].ctypes.data)                          # out over a member (the pool has slack behind it)
    assert L.snarkvm_hip_selftest_fr_rowcheck_fold(whole[n:].ctypes.data, None, n, 2, wa, pb, pc, mu.ctypes.data) == 0
    assert np.array_equal(whole[n:], rc.expected_fold(ints, util.fr_mont_to_ints(mu), n))
    # successes that touch nothing: no output; n == 0 (violations are zero-filled, NULL members are fine)
    assert L.snarkvm_hip_selftest_fr_rowcheck_fold(None, None, n, 2, pa, pb, pc, mu.ctypes.data) == 0
    assert L.snarkvm_hip_selftest_fr_rowcheck_fold(out[1:].ctypes.data, None, 0, 2, ptrs(None, None), ptrs(None, None), ptrs(None, None), mu.ctypes.data) == 0
    assert (out == GUARD).all() and (viol == GUARD).all()
    assert L.snarkvm_hip_selftest_fr_rowcheck_fold(None, viol[1:].ctypes.data, 0, 2, ptrs(None, None), ptrs(None, None), ptrs(None, None), None) == 0
    assert not rc.unguard(viol, 2).any()


# ---- the gather of round 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 48, 256])
def test_witness_evals(n):
    """ratio in {1, 2, 4, n}, w_len in {0, 1, n - input_size - 1, n - input_size}, out of place and in place"""
    x = rc.mixed(n, n)
    for ratio in (1, 2, 4, n):
        input_size = n // ratio
        room = n - input_size
        for w_len in sorted({0, min(1, room), max(room - 1, 0), room}):
            w = rc.mixed(w_len, ratio + w_len) if w_len else np.zeros((0, 4), dtype=np.uint64)
            want = rc.expected_witness_evals(w, x, input_size)
            assert not want[::ratio].any()
            assert np.array_equal(rc.selftest_witness(w, x, input_size), want), (ratio, w_len)
            assert np.array_equal(rc.selftest_witness(w, x, input_size, in_place=True), want), (ratio, w_len)
    full = rc.expected_witness_evals(rc.mixed(n - n // 4, 1), x, n // 4)  # every free position holds its own variable
    assert util.fr_mont_to_ints(full[1:2]) == [(util.fr_mont_to_ints(rc.mixed(n - n // 4, 1)[0:1])[0] - util.fr_mont_to_ints(x[1:2])[0]) % R]


def test_witness_evals_refusals_leave_out_untouched():
    L = _lib.lib()
    n = 8
    x, w = rc.mixed(n + 4, 1), rc.mixed(n, 2)
    out = rc.guarded(n)

    def refused(o=out[1:].ctypes.data, n=n, w=w.ctypes.data, w_len=4, x=x.ctypes.data, input_size=4):
        assert L.snarkvm_hip_selftest_fr_witness_evals(o, n, w, w_len, x, input_size) == -1
        assert (out == GUARD).all()

    refused(input_size=0), refused(input_size=3), refused(input_size=16)    # zero, non-dividing (16 does not divide 8 either)
    refused(w_len=5), refused(input_size=8, w_len=1)                         # w longer than n - input_size
    refused(n=(1 << 28) + 4)
    refused(o=None), refused(x=None), refused(w=None)                        # a NULL pointer with a non-zero length
    refused(x=out[2:].ctypes.data), refused(x=out.ctypes.data), refused(w=out[4:].ctypes.data)  # overlaps other than out == x_evals
    before = x.copy()
    assert L.snarkvm_hip_selftest_fr_witness_evals(x[1:].ctypes.data, n, w.ctypes.data, 4, x.ctypes.data, 4) == -1  # out one element into x_evals
    assert np.array_equal(x, before)
    assert L.snarkvm_hip_selftest_fr_witness_evals(None, 0, None, 0, None, 4) == 0  # n == 0 touches nothing
    assert L.snarkvm_hip_selftest_fr_witness_evals(out[1:].ctypes.data, n, w.ctypes.data, 4, x.ctypes.data, 4) == 0
    assert np.array_equal(rc.unguard(out, n), rc.expected_witness_evals(w[:4], x[:n], 4))


# ---- known answers held by the reference (tests/golden/varuna_circuit0.json), neither asserted by any other test ---------------------------------
def test_calculate_w_gives_w_lde_of_the_fixture(golden):
    """first.rs:127-161 on the oracle with the replay's gather: x_poly = the interpolation of (1, 8, 32, 128) over the input domain, |V| = 8"""
    fx = rc.fixture_rounds12(golden["varuna"])
    x_poly = oracle.ntt(rc.mont(fx["public"]), direction=oracle.INVERSE)
    x_evals = oracle.ntt(rc.pad(x_poly, 8))
    evals = rc.selftest_witness(rc.mont(fx["private"]), x_evals, 4)
    assert np.array_equal(evals, rc.expected_witness_evals(rc.mont(fx["private"]), x_evals, 4))
    q, rem = oracle.poly_divide(oracle.ntt(evals, direction=oracle.INVERSE), rc.vanishing(4))
    assert rem.shape[0] == 0
    assert util.fr_mont_to_ints(q) == fx["w_lde"] and len(fx["w_lde"]) == 4


def test_the_coset_route_gives_h_0_of_the_fixture(golden):
    """second.rs:76-142 with combiners one: no row is violated, and the fold over the evaluations on the coset 22 R, scaled by 1 / (22^8 - 1) and
    transformed back, is h_0 (7 coefficients, the eighth zero); the reference's own route on the oracle agrees"""
    fx = rc.fixture_rounds12(golden["varuna"])
    z = [rc.mont(fx["z"][name]) for name in "ABC"]
    _, viol = rc.selftest_fold(([z[0]], [z[1]], [z[2]]), None, 8, want="v")
    assert viol == [0]
    on_coset = [oracle.ntt(oracle.ntt(v, direction=oracle.INVERSE), kind=oracle.COSET) for v in z]
    mu = rc.mont([pow(pow(rc.COSET_GENERATOR, 8, R) - 1, -1, R)])
    out, _ = rc.selftest_fold(([on_coset[0]], [on_coset[1]], [on_coset[2]]), mu, 8, want="o")
    h_0 = oracle.ntt(out, direction=oracle.INVERSE, kind=oracle.COSET)
    assert rc.trimmed_ints(h_0) == fx["h_0"] and len(fx["h_0"]) == 7 and not h_0[7].any()
    ref = rc.reference_h0([{"lg_r": 3, "circuit_combiner": 1, "instance_combiners": [1], "z": [tuple(z)]}], 3)
    assert np.array_equal(ref, h_0)
