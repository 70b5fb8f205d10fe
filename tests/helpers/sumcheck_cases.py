"""Cases and expected values shared by tests/test_fr_sumcheck_host.py (CPU) and tests/test_gpu_fr_sumcheck.py: the arithmetizations, challenges and
scales of `snarkvm_hip_fr_matrix_sumcheck_evals`, the round-4 chain built on it (snarkvm_amd/matrices.py: matrix_sumcheck_witness, h_2), and what
every result is compared with, bit for bit.

Expected values do not come from the library.  Small cases: `oracle.fr_op("to_bigint")` turns every operand into a Python int, a, b and f are
computed mod r in Python (f = 0 where (alpha - row)(beta - col) = 0) and `oracle.fr_op("from_bigint")` gives the memory form back - the route of
tests/helpers/reduce_cases.py.  Large cases: the composition of `oracle.fr_vec_op` and `oracle.batch_inversion_and_mul`, the CPU restatement of the
reference's fourth.rs:178-211.  The chain: `oracle.ntt`, `oracle.polymul` and `oracle.poly_divide`.  Boundary sizes are derived from the geometry
that `snarkvm_hip_selftest_fr_sumcheck_geometry` reports, not hard-coded.
"""
import numpy as np

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib
from tests import util
from tests.helpers import reduce_cases as rc

R = rc.R
GUARD = rc.GUARD
INVALID_VALUE = 1  # hipErrorInvalidValue
to_ints = rc.to_ints


def from_ints(xs):
    """Python ints -> (n, 4) memory form through the oracle"""
    return oracle.fr_op("from_bigint", util.ints_to_fr([x % R for x in xs])) if len(xs) else np.zeros((0, 4), dtype=np.uint64)


def geometry(k):
    """{T, threads, blocks, share} of what the device call launches for a member of k elements: T threads in all, `threads` per workgroup,
    `share` elements per thread (snarkvm_hip_selftest_fr_sumcheck_geometry)"""
    out = np.zeros(4, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_sumcheck_geometry(k, out.ctypes.data) == 0
    return dict(zip(("T", "threads", "blocks", "share"), (int(x) for x in out)))


def edge_sizes():
    """k in {1, 2, 7, 8}; one below, at and one above one thread's share and one workgroup's share; several workgroups with a ragged tail"""
    g = geometry(1)
    share, wg = g["share"], g["share"] * g["threads"]
    sizes = [1, 2, 7, 8, share - 1, share, share + 1, wg - 1, wg, wg + 1, 2 * wg + wg // 3 + 1]
    assert all(geometry(k)["share"] == share for k in sizes)  # still the small-size regime the boundaries were derived in
    return sorted({k for k in sizes if k >= 1})


# ---- expected values -------------------------------------------------------------------------------------------------------------------------
def expected_py(row, col, rcv, alpha, beta, scales):
    """(a, b, f) by Python big ints"""
    r, c, v = to_ints(row), to_ints(col), to_ints(rcv)
    (al,), (be,), (sa, sb, sf) = to_ints(alpha), to_ints(beta), to_ints(scales)
    d = [(al - x) * (be - y) % R for x, y in zip(r, c)]
    a = [sa * x % R for x in v]
    b = [sb * x % R for x in d]
    f = [sf * x % R * pow(y, -1, R) % R if y else 0 for x, y in zip(v, d)]
    return from_ints(a), from_ints(b), from_ints(f)


def expected_oracle(row, col, rcv, alpha, beta, scales):
    """(a, b, f) by the C++ oracle's vector passes: fourth.rs:178 (a), :192 (b; (row - alpha)(col - beta) is the same element as the expanded
    form), :203-211 (f: the product, batch_inversion_and_mul, the product with row_col_val)"""
    scales = np.asarray(scales, dtype=np.uint64).reshape(3, 4)
    d = oracle.fr_vec_op("mul", oracle.fr_vec_op("sub_scalar", row, alpha), oracle.fr_vec_op("sub_scalar", col, beta))
    a = oracle.fr_vec_op("scale", rcv, scales[0:1])
    b = oracle.fr_vec_op("scale", d, scales[1:2])
    f = oracle.fr_vec_op("mul", oracle.batch_inversion_and_mul(d, scales[2:3]), rcv)
    return a, b, f


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
def scalars(seed, alpha=None, beta=None, scales=None):
    """alpha (1, 4), beta (1, 4), scales (3, 4): random unless given as Python ints"""
    v = rc.rnd(5, 40 + seed)
    al = v[0:1].copy() if alpha is None else util.ints_to_fr_mont([alpha])
    be = v[1:2].copy() if beta is None else util.ints_to_fr_mont([beta])
    sc = v[2:5].copy() if scales is None else util.ints_to_fr_mont(list(scales))
    return al, be, sc


def arith(k, seed, alpha, beta, T=None, zeros=True):
    """row, col, row_col_val of k elements: random, with row_col_val in {0, 1, r - 1} at every third place and padding triples (1, 1, 0) at the
    end.  zeros (for a partition into T threads, thread t owning t, t + T, ...): entries with row = alpha or col = beta (d = 0) at the first, the
    middle and the last place of the shares of threads 0, 1 and 2 (as far as they exist) and over the whole share of the last thread."""
    row, col, rcv = rc.rnd(k, 50 + seed).copy(), rc.rnd(k, 60 + seed).copy(), rc.rnd(k, 70 + seed).copy()
    sp = util.ints_to_fr_mont([0, 1, R - 1])
    rcv[::3] = sp[np.arange(len(rcv[::3])) % 3]
    pad = max(1, k // 8) if k > 2 else 0
    if pad:
        one = util.ints_to_fr_mont([1])[0]
        row[k - pad :], col[k - pad :], rcv[k - pad :] = one, one, 0
    if zeros:
        T = geometry(k)["T"] if T is None else min(T, k)
        owned = lambda t: list(range(t, k, T))
        places = []
        for t, pick in ((0, lambda o: o[0]), (1, lambda o: o[len(o) // 2]), (2, lambda o: o[-1])):
            if t < T:
                places.append(pick(owned(t)))
        places += owned(T - 1) if T > 3 else []
        for n, i in enumerate(sorted(set(places))):
            if n % 2:
                row[i] = alpha[0]
            else:
                col[i] = beta[0]
    return row, col, rcv


def selftest(row, col, rcv, alpha, beta, scales, blocks, threads, want="abf"):
    """snarkvm_hip_selftest_fr_sumcheck -> (a, b, f), None for the outputs not wanted; the element behind every output is a guard"""
    k = row.shape[0]
    outs = {w: np.full((k + 1, 4), GUARD, dtype=np.uint64) if w in want else None for w in "abf"}
    p = lambda x: x.ctypes.data if x is not None and x.size else None
    rcode = _lib.lib().snarkvm_hip_selftest_fr_sumcheck(p(outs["a"]), p(outs["b"]), p(outs["f"]), p(row), p(col), p(rcv), k, p(alpha), p(beta), p(scales), blocks, threads)
    assert rcode == 0
    for o in outs.values():
        assert o is None or (o[k] == GUARD).all()
    return tuple(None if outs[w] is None else outs[w][:k] for w in "abf")


# ---- the committed fixture (tests/golden/varuna_circuit0.json) -------------------------------------------------------------------------------
def fixture(tv):
    """the Varuna test vector: alpha = challenges[0], beta = challenges[4], deltas = challenges[5:8]; R, C and K are the domain of 8 elements, the
    input domain has 4; per matrix the arithmetization (row, col, row_col_val) by Python ints straight from ahp/matrices.rs:156-181"""
    from snarkvm_amd import matrices

    ch = [int(x) for x in tv["challenges"].split()]
    dom = [int(x) for x in tv["domain"]["K"]]
    assert dom == [int(x) for x in tv["domain"]["R"]] == [int(x) for x in tv["domain"]["C"]] and len(dom) == 8
    ariths = {}
    for name in "ABC":
        row, col, rcv = [], [], []
        for i, entries in enumerate(tv["instance"][name]):
            for j, val in enumerate(entries):
                if val:
                    r, c = dom[i], dom[matrices.reindex_by_subdomain(8, 4, j)]
                    row.append(r), col.append(c), rcv.append(int(val) * r * c % R)
        assert len(row) == 7
        pad = 8 - len(row)
        ariths[name] = tuple(util.ints_to_fr_mont(x) for x in (row + [1] * pad, col + [1] * pad, rcv + [0] * pad))
    alpha, beta = util.ints_to_fr_mont([ch[0]]), util.ints_to_fr_mont([ch[4]])
    a_scale = (pow(ch[0], 8, R) - 1) * (pow(ch[4], 8, R) - 1) % R
    scales = util.ints_to_fr_mont([a_scale, 64, a_scale * pow(64, -1, R)])
    return {"alpha": alpha, "beta": beta, "deltas": util.ints_to_fr_mont(ch[5:8]), "scales": scales, "ariths": ariths, "domain": dom,
            "g": {n: [int(x) for x in tv["polynomials"]["g_" + n.lower()]] for n in "AB"}, "h_2": [int(x) for x in tv["polynomials"]["h_2"]]}


def trimmed_ints(v):
    x = util.fr_mont_to_ints(v)
    while x and x[-1] == 0:
        x.pop()
    return x


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------
def random_circuit(seed, lg_r=9, lg_c=9, lg_k=(10, 10, 10), lg_input=4):
    """three random SparseMatrix of 2^lg_r - 3 rows over 2^lg_c - 5 variables, matrix m with about 7/8 of 2^lg_k[m] entries"""
    from snarkvm_amd.matrices import SparseMatrix

    rng = np.random.default_rng(seed)
    rows, cols = (1 << lg_r) - 3, (1 << lg_c) - 5
    out = []
    for m, lg in enumerate(lg_k):
        nnz = (7 << lg) // 8
        lens = np.bincount(rng.integers(0, rows, nnz), minlength=rows)
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        out.append(SparseMatrix(rows, cols, row_ptr, rng.integers(0, cols, nnz).astype(np.uint32), rc.rnd(nnz, 80 + seed + m)))
    return out


def chain_expected(row, col, rcv, alpha, beta, scales, k_max):
    """calculate_matrix_sumcheck_witness by the oracle: (sum, lhs, g, a_poly, b_poly, remainder), every polynomial UNTRIMMED at the length the
    device chain leaves (lhs, a_poly, b_poly: |K|; g: |K| - 1) except the remainder, which is trimmed"""
    k = row.shape[0]
    lg = k.bit_length() - 1
    a, b, f = expected_oracle(row, col, rcv, alpha, beta, scales)
    a_poly, b_poly, f_poly = (oracle.ntt(x, direction=oracle.INVERSE) for x in (a, b, f))
    h = np.zeros((2 * k, 4), dtype=np.uint64)
    h[:k] = a_poly
    h = oracle.fr_vec_op("sub", h, oracle.polymul(lg + 1, [b_poly, f_poly]))
    one = util.ints_to_fr_mont([1, R - 1])
    q, rem = oracle.poly_divide(h, [(0, one[1]), (k, one[0])])
    lhs = np.zeros((k, 4), dtype=np.uint64)
    lhs[: q.shape[0]] = oracle.fr_vec_op("scale", q, util.ints_to_fr_mont([k * pow(k_max, -1, R) % R])) if q.shape[0] else q
    return f_poly[0:1], lhs, f_poly[1:], a_poly, b_poly, rem


def arith_py(matrix, k, constraint_size, variable_size, input_size):
    """ahp/matrices.rs:156-181 by Python ints, independent of snarkvm_amd.matrices.matrix_evals except for reindex_by_subdomain"""
    from snarkvm_amd import matrices

    wr, wc = pyref.domain_group_gen(constraint_size.bit_length() - 1), pyref.domain_group_gen(variable_size.bit_length() - 1)
    vals = to_ints(matrix.vals)
    rp, ci = matrix.row_ptr.tolist(), matrix.col_idx.tolist()
    row, col, rcv = [], [], []
    for i in range(matrix.rows):
        r = pow(wr, i, R)
        for e in range(rp[i], rp[i + 1]):
            c = pow(wc, matrices.reindex_by_subdomain(variable_size, input_size, ci[e]), R)
            row.append(r), col.append(c), rcv.append(vals[e] * r * c % R)
    pad = k - len(row)
    return tuple(util.ints_to_fr_mont(x) for x in (row + [1] * pad, col + [1] * pad, rcv + [0] * pad))
