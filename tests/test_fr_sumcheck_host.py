"""The Varuna round-4 matrix-sumcheck evaluations without a GPU (include/snarkvm_hip.h: snarkvm_hip_fr_matrix_sumcheck_evals; csrc/poly.hip.h:
fr_sumcheck_evals_kernel): the host replay `snarkvm_hip_selftest_fr_sumcheck` runs the kernel's own per-thread routine over an explicit geometry,
so the partition, the zero rule of the shared inversion and the constants are checked here; the refusals that need no device; the host-side
arithmetization (snarkvm_amd/matrices.py: matrix_evals); and the known answers of tests/golden/varuna_circuit0.json.

Every comparison is bit-exact; expected values come from Python big ints or the C++ oracle (tests/helpers/sumcheck_cases.py), never from the library.
"""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, matrices
from tests import util
from tests.helpers import reduce_cases as rc
from tests.helpers import sumcheck_cases as sc

R = sc.R


def _same(got, want):
    for g, w, name in zip(got, want, "abf"):
        assert g is None or np.array_equal(g, w), name


def _geometries(k):
    """(blocks, threads) with T = 1, T = k, T > k, T not dividing k, and the device call's own"""
    g = sc.geometry(k)
    out = [(1, 1), (1, k), (k, 1), (2, k), (1, k + 3), (g["blocks"], g["threads"])]
    if k > 3:
        out += [(1, next(t for t in range(2, k) if k % t)), (2, (k + 3) // 4)]
    return out


def test_geometry():
    L = _lib.lib()
    out = np.zeros(4, dtype=np.uint32)
    assert L.snarkvm_hip_selftest_fr_sumcheck_geometry(5, None) == -1
    assert L.snarkvm_hip_selftest_fr_sumcheck_geometry((1 << 28) + 1, out.ctypes.data) == -1
    shares = set()
    for k in (0, 1, 2, 7, 8, 1000, 1 << 12, (1 << 16) + 1, 1 << 17, 1 << 20, 1 << 28):
        g = sc.geometry(k)
        assert g["T"] == -(-k // g["share"]) and g["blocks"] == -(-g["T"] // g["threads"]) and g["threads"] % 64 == 0, (k, g)
        shares.add(g["share"])
    assert len(shares) > 1  # the share grows with k: more than one regime
    assert sc.geometry(1 << 17)["T"] > 4096  # more threads than the 32 per thread of fr_batch_inverse_run would give


@pytest.mark.parametrize("k", sc.edge_sizes())
def test_edge_sizes_over_every_geometry(k):
    alpha, beta, scales = sc.scalars(k)
    row, col, rcv = sc.arith(k, k, alpha, beta)
    want = sc.expected_py(row, col, rcv, alpha, beta, scales)
    assert not want[2][np.flatnonzero(~want[1].any(axis=1))].any()  # f = 0 wherever b = 0
    for blocks, threads in _geometries(k):
        _same(sc.selftest(row, col, rcv, alpha, beta, scales, blocks, threads), want)


@pytest.mark.parametrize("blocks,threads", [(2, 3), (1, 7), (3, 64)])
def test_zero_denominators_at_every_place_of_a_share(blocks, threads):
    """d = 0 first, in the middle and last in a thread's chain, and a thread whose whole share is zeros: b = f = 0 there, every neighbour exact"""
    T = blocks * threads
    k = 7 * T + T // 2
    alpha, beta, scales = sc.scalars(3)
    row, col, rcv = sc.arith(k, 5, alpha, beta, T=T)
    want = sc.expected_py(row, col, rcv, alpha, beta, scales)
    zero_b = np.flatnonzero(~want[1].any(axis=1))
    assert len(zero_b) >= 3 + k // T and set(range(T - 1, k, T)) <= set(zero_b.tolist())
    assert not want[2][zero_b].any()
    _same(sc.selftest(row, col, rcv, alpha, beta, scales, blocks, threads), want)
    for blocks2, threads2 in ((1, 1), (1, k), (5, 2)):  # the same bytes from any other partition
        _same(sc.selftest(row, col, rcv, alpha, beta, scales, blocks2, threads2), want)
    # every element a zero denominator
    row[:] = alpha[0]
    a, b, f = sc.selftest(row, col, rcv, alpha, beta, scales, blocks, threads)
    assert not b.any() and not f.any() and np.array_equal(a, want[0])


@pytest.mark.parametrize("alpha,beta,scales", [(0, None, None), (None, 0, None), (0, 0, (0, 0, 0)), (None, None, (1, 1, 1)), (None, None, (R - 1, R - 1, R - 1)),
                                               (R - 1, R - 1, (0, 1, R - 1))])
def test_special_challenges_and_scales(alpha, beta, scales):
    k = 45
    al, be, scl = sc.scalars(9, alpha, beta, scales)
    row, col, rcv = sc.arith(k, 9, al, be, T=6)
    row[5], col[6] = 0, 0  # with alpha = 0 or beta = 0 these are zero denominators too
    want = sc.expected_py(row, col, rcv, al, be, scl)
    for blocks, threads in ((2, 3), (1, 64)):
        _same(sc.selftest(row, col, rcv, al, be, scl, blocks, threads), want)


def test_all_r_minus_1():
    """every operand r - 1: the largest canonical limbs the chain of products sees"""
    k = 33
    top = util.ints_to_fr_mont([R - 1])
    row = col = rcv = np.tile(top, (k, 1))
    al, be, scl = sc.scalars(1, R - 2, 1, (R - 1, R - 1, R - 1))
    _same(sc.selftest(row, col, rcv, al, be, scl, 1, 4), sc.expected_py(row, col, rcv, al, be, scl))


@pytest.mark.parametrize("want", ["a", "b", "f", "ab", "af", "bf", "abf", ""])
def test_skipped_outputs(want):
    k = 29
    alpha, beta, scales = sc.scalars(2)
    row, col, rcv = sc.arith(k, 2, alpha, beta, T=5)
    full = sc.expected_py(row, col, rcv, alpha, beta, scales)
    got = sc.selftest(row, col, rcv, alpha, beta, scales, 1, 5, want=want)
    for g, w, name in zip(got, full, "abf"):
        assert (g is None) == (name not in want)
    _same(got, full)


def test_past_the_share_thresholds():
    """the sizes at which the share per thread changes, at the device call's own geometry, against the C++ oracle's composition"""
    small = sc.geometry(1)["share"]
    k = 1
    while sc.geometry(k)["share"] == small:  # the first k of the next regime, found by doubling and bisection
        k *= 2
    lo, hi = k // 2, k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if sc.geometry(mid)["share"] == small else (lo, mid)
    assert sc.geometry(lo)["share"] == small < sc.geometry(hi)["share"]
    alpha, beta, scales = sc.scalars(4)
    for k in (lo, hi):
        g = sc.geometry(k)
        row, col, rcv = sc.arith(k, 4, alpha, beta)
        _same(sc.selftest(row, col, rcv, alpha, beta, scales, g["blocks"], g["threads"]), sc.expected_oracle(row, col, rcv, alpha, beta, scales))


def test_the_two_references_agree():
    k = 200
    alpha, beta, scales = sc.scalars(6)
    row, col, rcv = sc.arith(k, 6, alpha, beta, T=9)
    _same(sc.expected_oracle(row, col, rcv, alpha, beta, scales), sc.expected_py(row, col, rcv, alpha, beta, scales))


def test_selftest_refusals():
    L = _lib.lib()
    k = 4
    alpha, beta, scales = sc.scalars(1)
    row, col, rcv = sc.arith(k, 1, alpha, beta)
    out = np.full((k, 4), sc.GUARD, dtype=np.uint64)
    p = lambda x: x.ctypes.data
    ok = [p(out), None, None, p(row), p(col), p(rcv), k, p(alpha), p(beta), p(scales), 1, 2]
    for at, bad in ((3, None), (4, None), (5, None), (6, (1 << 28) + 1), (7, None), (8, None), (9, None), (10, 0), (11, 0)):
        args = list(ok)
        args[at] = bad
        assert L.snarkvm_hip_selftest_fr_sumcheck(*args) == -1, at
    assert (out == sc.GUARD).all()
    assert L.snarkvm_hip_selftest_fr_sumcheck(None, None, None, None, None, None, 0, p(alpha), p(beta), p(scales), 1, 1) == 0


def _refused(err):
    with pytest.raises(_lib.HipError) as e:
        _lib.check(err)
    assert e.value.code == sc.INVALID_VALUE and e.value.message, e.value


def test_refusals_that_need_no_device():
    L = _lib.lib()
    x = rc.rnd(4, 1).copy()
    p = x.ctypes.data
    _refused(L.snarkvm_hip_fr_arith_register(None, 4, p, p, p))
    for args in ((4, None, p, p), (4, p, None, p), (4, p, p, None), ((1 << 28) + 1, p, p, p)):
        h = ctypes.c_void_p(0xDEAD)
        _refused(L.snarkvm_hip_fr_arith_register(ctypes.byref(h), *args))
        assert not h.value
    L.snarkvm_hip_fr_arith_free(None)
    alpha, beta, scales = sc.scalars(1)
    out = np.full((8, 4), sc.GUARD, dtype=np.uint64)
    outs = (ctypes.c_void_p * 17)(*([out.ctypes.data] * 17))
    nulls = (ctypes.c_void_p * 17)()
    call = lambda ariths, count: L.snarkvm_hip_fr_matrix_sumcheck_evals(ariths, count, outs, None, None, alpha.ctypes.data, beta.ctypes.data, scales.ctypes.data, 0)
    _refused(call(nulls, 17))  # count > 16
    _refused(call(nulls, 1))   # a NULL handle in the list
    _refused(call(None, 1))
    _lib.check(call(nulls, 0))  # count == 0: success, nothing touched, no device needed
    _lib.check(call(None, 0))
    assert (out == sc.GUARD).all()


# ---- the arithmetization on the host -------------------------------------------------------------------------------------------------------------
def test_matrix_evals_against_python():
    (m,) = sc.random_circuit(3, lg_r=5, lg_c=6, lg_k=(7,), lg_input=2)
    got = matrices.matrix_evals(m, 128, 64, 4)
    want = sc.arith_py(m, 128, 32, 64, 4)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert m.nnz < 128 and util.fr_mont_to_ints(got[0][m.nnz :]) == [1] * (128 - m.nnz) and not got[2][m.nnz :].any()
    wider = matrices.matrix_evals(m, 128, 64, 4, constraint_domain_size=64)
    assert np.array_equal(wider[1], got[1]) and not np.array_equal(wider[0], got[0])
    with pytest.raises(ValueError):
        matrices.matrix_evals(m, 64, 64, 4)  # more entries than |K|
    with pytest.raises(ValueError):
        matrices.matrix_evals(m, 100, 64, 4)


def _fixture_matrices(tv):
    return {k: matrices.SparseMatrix.from_rows([[(v, j) for j, v in enumerate(row) if v] for row in tv["instance"][k]], 7) for k in "ABC"}


def test_matrix_evals_of_the_fixture(golden):
    fx = sc.fixture(golden["varuna"])
    for name, m in _fixture_matrices(golden["varuna"]).items():
        for g, w in zip(matrices.matrix_evals(m, 8, 8, 4), fx["ariths"][name]):
            assert np.array_equal(g, w), name
    assert np.array_equal(matrices.sumcheck_scales(3, 3, fx["alpha"], fx["beta"]), fx["scales"])


# ---- known answers held by the reference ---------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_fixture_through_the_host_replay(golden):
    """g_a, g_b = the coefficients from 1 on of iNTT_8(f_A), iNTT_8(f_B); sum = f[0]; the three remainders of (a - b f) / (X^8 - 1) are zero and
    sum_M delta_M lhs_M = h_2 pins C (the fixture's g_c is a copy of its g_b and is not asserted on)"""
    fx = sc.fixture(golden["varuna"])
    w = fx["domain"][1]
    lhs = {}
    for name, (row, col, rcv) in fx["ariths"].items():
        want = sc.expected_py(row, col, rcv, fx["alpha"], fx["beta"], fx["scales"])
        for blocks, threads in ((1, 1), (1, 3), (1, 64)):
            got = sc.selftest(row, col, rcv, fx["alpha"], fx["beta"], fx["scales"], blocks, threads)
            _same(got, want)
        total, q, g, a_poly, b_poly, rem = sc.chain_expected(row, col, rcv, fx["alpha"], fx["beta"], fx["scales"], 8)
        assert rem.shape[0] == 0, name
        f_ints = util.fr_mont_to_ints(got[2])
        assert util.fr_mont_to_ints(total) == [sum(f_ints) * pow(8, -1, R) % R]  # f[0] of the interpolation = the mean of the evaluations
        assert util.fr_mont_to_ints(oracle.ntt(got[2], direction=oracle.INVERSE))[1:] == util.fr_mont_to_ints(g)
        if name in fx["g"]:
            assert sc.trimmed_ints(g) == fx["g"][name], name
        lhs[name] = util.fr_mont_to_ints(q)
    deltas = util.fr_mont_to_ints(fx["deltas"])
    h_2 = [sum(d * lhs[name][i] for d, name in zip(deltas, "ABC")) % R for i in range(8)]
    while h_2 and h_2[-1] == 0:
        h_2.pop()
    assert h_2 == fx["h_2"]
    assert w != 1
