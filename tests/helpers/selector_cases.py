"""Cases and expected values shared by tests/test_fr_selector_host.py (CPU, through the host replay) and tests/test_gpu_fr_selector.py: the members
of `snarkvm_hip_fr_selector_fold`, the round-3 chain built on it (snarkvm_amd/matrices.py: assignment_device, lineval_sumcheck_witness) and what
every result is compared with, bit for bit.

Expected values do not come from the library and never from the tiling identity the kernel rests on.  The fold: the reference's own four steps
(ahp/selectors.rs:111-118) restated on the C++ oracle - scale, `poly_divide` by X^n - 1, `mul_by_vanishing(N)`, `poly_divide` by X^n - 1 again,
the second remainder asserted zero - and the members added up with `fr_vec_op("add")`.  The sums: the member folded to its source domain,
`oracle.ntt` over that domain, and the evaluations added up (third.rs:317).  The chain: third.rs:280-327 and 179-213 on `oracle.lagrange_coefficients`,
tests/helpers/spmv_cases.expected, `oracle.ntt` and `oracle.polymul`.
"""
import ctypes

import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib
from tests import util

R = pyref.R_MOD
GUARD = 0x5A5A5A5A5A5A5A5A
INVALID_VALUE = 1  # hipErrorInvalidValue
ZERO = np.zeros((0, 4), dtype=np.uint64)
SPECIAL = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2]


def mont(xs):
    return util.ints_to_fr_mont(list(xs)) if len(xs) else ZERO.copy()


def rnd(n, seed):
    """n random field elements in memory form (any canonical residue is one: the top limb stays below that of r)"""
    rng = np.random.default_rng(1000 + seed)
    v = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    v[:, 3] >>= np.uint64(4)
    return v


def special(n, seed):
    """n elements cycling through 0, 1, r - 1, (r - 1) / 2, (r + 1) / 2"""
    tab = mont(SPECIAL)
    return tab[(np.arange(n) + seed) % len(SPECIAL)].copy()


def mixed(n, seed):
    v = rnd(n, seed)
    v[::3] = special(len(v[::3]), seed)
    return v


_X_N_MINUS_1 = {}


def vanishing(n):
    if n not in _X_N_MINUS_1:
        one = mont([1, R - 1])
        _X_N_MINUS_1[n] = [(0, one[1]), (n, one[0])]
    return _X_N_MINUS_1[n]


def pad(v, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    assert v.shape[0] <= n, (v.shape, n)
    out[: v.shape[0]] = v
    return out


def tree_sum(v):
    """the sum of the elements of v by halving with the oracle's vector addition -> (1, 4)"""
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
    if v.shape[0] == 0:
        return np.zeros((1, 4), dtype=np.uint64)
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.concatenate([v, np.zeros((1, 4), dtype=np.uint64)])
        half = v.shape[0] // 2
        v = oracle.fr_vec_op("add", v[:half], v[half:])
    return v


def expected_member(p, n, N, mu):
    """(h_i, xg_i) of apply_randomized_selector with a remainder witness: h_i trimmed, xg_i of N coefficients (None when N is None)"""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4)
    scaled = oracle.fr_vec_op("scale", p, mu) if p.shape[0] else p
    h, xg = oracle.poly_divide(scaled, vanishing(n)) if p.shape[0] else (ZERO, ZERO)
    if N is None:
        return h, None
    q, rem = oracle.poly_divide(oracle.mul_by_vanishing(xg, N), vanishing(n))
    assert rem.shape[0] == 0, "the second remainder of the selector is not zero"
    return h, pad(q, N)


def expected_sum(p, n):
    """the sum of the member over its source domain of n elements: fold to n coefficients, transform, add up"""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4)
    if p.shape[0] == 0:
        return np.zeros((1, 4), dtype=np.uint64)
    rem = oracle.poly_divide(p, vanishing(n))[1]
    assert n & (n - 1) == 0, "expected_sum: a source domain is a power of two"
    return tree_sum(oracle.ntt(pad(rem, n)))


def expected(polys, src_sizes, mus, N, h_len):
    """(h, xg, sums) of the whole call: h of h_len coefficients, xg of N (None when N is None), sums (count, 4)"""
    h = np.zeros((h_len, 4), dtype=np.uint64)
    xg = None if N is None else np.zeros((N, 4), dtype=np.uint64)
    sums = np.zeros((len(polys), 4), dtype=np.uint64)
    for k, (p, n) in enumerate(zip(polys, src_sizes)):
        hi, xi = expected_member(p, n, N, mus[k : k + 1])
        if hi.shape[0]:
            h = oracle.fr_vec_op("add", h, pad(hi, h_len))
        if xg is not None:
            xg = oracle.fr_vec_op("add", xg, xi)
        sums[k] = expected_sum(p, n)[0]
    return h, xg, sums


def quotient_len(polys, src_sizes):
    return max([max(len(p) - n, 0) for p, n in zip(polys, src_sizes)] + [0])


# ---- calls -------------------------------------------------------------------------------------------------------------------------------------
def arrays(polys, src_sizes, mus):
    """the four host arrays of the C call (kept alive by the caller)"""
    k = len(polys)
    polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
    pp = (ctypes.c_void_p * max(1, k))(*[p.ctypes.data if p.shape[0] else None for p in polys])
    pl = (ctypes.c_size_t * max(1, k))(*[p.shape[0] for p in polys])
    ps = (ctypes.c_size_t * max(1, k))(*[int(n) for n in src_sizes])
    mu = np.ascontiguousarray(mus, dtype=np.uint64).reshape(-1, 4) if k else ZERO.copy()
    return polys, pp, pl, ps, mu


def guarded(n):
    """n elements to be written, a guard element in front and behind"""
    return np.full((n + 2, 4), GUARD, dtype=np.uint64)


def unguard(buf, n):
    assert (buf[0] == GUARD).all() and (buf[n + 1] == GUARD).all(), "a guard element was written"
    return buf[1 : n + 1]


def selftest(polys, src_sizes, mus, N, h_len, want="hxs"):
    """snarkvm_hip_selftest_fr_selector_fold -> (h, xg, sums), None for the outputs not wanted; every output sits between two guards"""
    polys, pp, pl, ps, mu = arrays(polys, src_sizes, mus)
    k = len(polys)
    bufs = {"h": guarded(h_len) if "h" in want else None, "x": guarded(N or 0) if "x" in want else None, "s": guarded(k) if "s" in want else None}
    at = lambda b: b[1:].ctypes.data if b is not None else None
    rcode = _lib.lib().snarkvm_hip_selftest_fr_selector_fold(at(bufs["h"]), h_len, at(bufs["x"]), N or 0, at(bufs["s"]), k, pp, pl, ps, mu.ctypes.data if k else None)
    assert rcode == 0
    sizes = {"h": h_len, "x": N or 0, "s": k}
    return tuple(None if bufs[w] is None else unguard(bufs[w], sizes[w]).copy() for w in "hxs")


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------
def class_lengths(n):
    """L in {0, 1, n - 1, n, n + 1, 2n - 1, 2n, 2n + 1, 3n + 5}"""
    return sorted({0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n + 5})


SRC_SIZES = (1, 2, 8, 64)
RATIOS = (1, 2, 8)
MULTIPLIERS = [0, 1, R - 1]


# ---- the committed fixture (tests/golden/varuna_circuit0.json) ---------------------------------------------------------------------------------
def fixture_round3(tv):
    """round 3 of the Varuna test vector in the non-hiding mode: alpha = challenges[0], eta_b = challenges[2], eta_c = challenges[3], circuit and
    instance combiners one, R = C = 8 elements, the input domain 4.  -> dict with the known answers as Python ints (w_lde, z_lde, g_1, h_1) and
    the three dense matrices"""
    ch = [int(x) for x in tv["challenges"].split()]
    poly = lambda name: [int(x) for x in tv["polynomials"][name]]
    return {"alpha": ch[0], "eta_b": ch[2], "eta_c": ch[3], "w_lde": poly("w_lde"), "z_lde": poly("z_lde"), "g_1": poly("g_1"), "h_1": poly("h_1"),
            "matrices": {name: [[int(v) for v in row] for row in tv["instance"][name]] for name in "ABC"}, "domain": [int(x) for x in tv["domain"]["C"]]}


def sparse(dense, cols):
    from snarkvm_amd import matrices

    return matrices.SparseMatrix.from_rows([[(v, j) for j, v in enumerate(row) if v] for row in dense], cols)


def trimmed_ints(v):
    x = util.fr_mont_to_ints(v)
    while x and x[-1] == 0:
        x.pop()
    return x


# ---- the chain by the oracle -------------------------------------------------------------------------------------------------------------------
def m_at_alpha(matrix_t, lg_r, lg_c, alpha):
    """third.rs:303-311: M(alpha, X) as |C| coefficients - the transposed SparseMatrix times l_alpha (tests/helpers/spmv_cases.expected), interpolated"""
    from tests.helpers import spmv_cases

    lag = oracle.lagrange_coefficients(lg_r, alpha)
    evals = spmv_cases.expected(matrix_t, lag[: matrix_t.cols], 1 << lg_c)
    return oracle.ntt(evals, direction=oracle.INVERSE)


def chain_expected(circuits, alpha, eta_b, eta_c, lg_n, mask=None):
    """calculate_lineval_sumcheck_witness by the oracle.  circuits: dicts {transposes: three SparseMatrix, lg_r, lg_c, circuit_combiner (int),
    instance_combiners (ints), assignments: (len, 4) arrays}; alpha, eta_b, eta_c: (1, 4).  -> (h_1, xg_1, sums): h_1 trimmed-then-summed at its
    longest length, xg_1 of N coefficients, sums per circuit (instances, 3, 4)"""
    N = 1 << lg_n
    combiners = [1] + util.fr_mont_to_ints(np.concatenate([eta_b, eta_c]))
    hs, xg, sums = [], np.zeros((N, 4), dtype=np.uint64), []
    for c in circuits:
        size_c = 1 << c["lg_c"]
        ms = [m_at_alpha(t, c["lg_r"], c["lg_c"], alpha) for t in c["transposes"]]
        per = np.zeros((len(c["assignments"]), 3, 4), dtype=np.uint64)
        for i, z in enumerate(c["assignments"]):
            lg_p = max(size_c + len(z) - 2, 0).bit_length()
            for m in range(3):
                prod = oracle.polymul(lg_p, [ms[m], z])[: size_c + len(z) - 1]
                per[i, m] = expected_sum(prod, size_c)[0]
                mu = mont([c["circuit_combiner"] * c["instance_combiners"][i] * combiners[m] * size_c * pow(N, -1, R)])
                h_i, xg_i = expected_member(prod, size_c, N, mu)
                hs.append(h_i)
                xg = oracle.fr_vec_op("add", xg, xg_i)
        sums.append(per)
    if mask is not None:
        h_m, xg_m = oracle.poly_divide(mask, vanishing(N))
        hs.append(h_m)
        xg = oracle.fr_vec_op("add", xg, pad(xg_m, N))
    h_len = max([h.shape[0] for h in hs] + [0])
    h = np.zeros((h_len, 4), dtype=np.uint64)
    for x in hs:
        if x.shape[0]:
            h = oracle.fr_vec_op("add", h, pad(x, h_len))
    return h, xg, sums
