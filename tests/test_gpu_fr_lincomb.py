"""`snarkvm_hip_fr_lincomb` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_lincomb_kernel): a linear combination of
polynomials of ragged lengths in one pass, and `SonicKZG10.open_combinations` on top of it.

Every comparison is bit-exact against the oracle's own `fr_vec_op("axpy" | "add")` chain over zero-padded operands
(tests/helpers/lincomb.py).  n_out: one element, one workgroup of 256 less one / exact / plus one, several workgroups with a ragged
last one (4099), and 2^21 + 3 - past the 8192 x 256 threads of the grid, so that the stride loop runs.
"""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, kzg10, plugin, sonic_pc
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.helpers import lincomb as lc

pytestmark = pytest.mark.gpu

INVALID_VALUE = 1  # hipErrorInvalidValue
GUARD = 0x5A5A5A5A5A5A5A5A


class Arena:
    """the operands of one call in ONE device block, each followed by a guard element; out (n_out + guard) at the end"""

    def __init__(self, polys, n_out):
        self.lens = [len(p) for p in polys]
        parts, self.offs, at = [], [], 0
        for p in polys:
            self.offs.append(at)
            parts += [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4), np.full((1, 4), GUARD, dtype=np.uint64)]
            at += len(p) + 1
        self.out_off, self.n_out = at, n_out
        parts.append(np.full((n_out + 1, 4), GUARD, dtype=np.uint64))
        self.host = np.concatenate(parts)
        self.mem = HipMem.from_numpy(self.host)

    def ptr(self, k):
        return self.mem.ptr + 32 * self.offs[k]

    def ptrs(self):
        return [self.ptr(k) for k in range(len(self.lens))]

    @property
    def out(self):
        return self.mem.ptr + 32 * self.out_off

    def result(self):
        """out, after checking that nothing but out has changed"""
        now = self.mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[: self.out_off], self.host[: self.out_off]), "an operand or a guard was written"
        assert (now[-1] == GUARD).all(), "the element behind out was written"
        return now[self.out_off : self.out_off + self.n_out]


def run(coeffs, polys, n_out, on_device):
    if on_device:
        a = Arena(polys, n_out)
        plugin.fr_lincomb_device(a.out, n_out, a.ptrs(), a.lens, coeffs)
        return a.result()
    out = np.full((n_out + 1, 4), GUARD, dtype=np.uint64)
    pp, pl, cs = lc.call_args([p.ctypes.data for p in polys], [len(p) for p in polys], coeffs)
    _lib.check(_lib.lib().snarkvm_hip_fr_lincomb(out.ctypes.data, n_out, len(polys), pp, pl, cs.ctypes.data, 0))
    assert (out[n_out] == GUARD).all()
    return out[:n_out]


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n_out", [1, 255, 256, 257, 4099])
def test_counts_and_ragged_lengths(n_out, on_device):
    for count in lc.COUNTS:
        for longest in sorted({n_out, n_out * 2 // 3}):  # n_out at, and past, the longest operand
            coeffs, polys = lc.make_case(count, longest, count % 5)
            assert np.array_equal(run(coeffs, polys, n_out, on_device), lc.expected(coeffs, polys, n_out)), (count, n_out, longest)


@pytest.mark.parametrize("kind", ["special", "max", "rawmax"])
def test_edge_values(kind):
    for count in (1, 6, 7, lc.CHUNK + 1):
        coeffs, polys = lc.make_case(count, 300, 1, kind)
        assert np.array_equal(run(coeffs, polys, 300, 1), lc.expected(coeffs, polys, 300)), (kind, count)


def test_no_operands_zero_fills():
    for on_device in (0, 1):
        assert not run(np.zeros((0, 4), dtype=np.uint64), [], 300, on_device).any()
        assert not run(lc.rnd(2, 7), [lc.rnd(0, 1), lc.rnd(0, 2)], 300, on_device).any()


@pytest.mark.parametrize("count", [2, 7])
def test_past_the_grid_cap(count):
    """2^21 + 3 elements: more than the 8192 x 256 threads fr_grid launches, every thread takes a second element and three a third"""
    n_out = (1 << 21) + 3
    lens = [n_out, n_out - 5, (1 << 21) - 1, 1 << 20, 77, n_out, 1][:count]
    polys = [lc.rnd(n, 1 + k) for k, n in enumerate(lens)]
    coeffs = lc.rnd(count, 7)
    assert np.array_equal(run(coeffs, polys, n_out, 1), lc.expected(coeffs, polys, n_out))


@pytest.mark.parametrize("count", [1, 7, lc.CHUNK + 1, 2 * lc.CHUNK + 1])
@pytest.mark.parametrize("which", ["first", "last"])
def test_in_place(count, which):
    """out is the start of an operand: with more than one launch that operand must not be read after out has been written - also when it is the
    shortest operand, listed last"""
    n_out = 4099
    coeffs, polys = lc.make_case(count, n_out, 3)
    k = 0 if which == "first" else count - 1
    polys[k] = lc.rnd(n_out if which == "first" else 700, 5)
    want = lc.expected(coeffs, polys, n_out)
    a = Arena(polys[:k] + polys[k + 1 :], n_out)
    a.mem.upload(np.ascontiguousarray(polys[k]), 32 * a.out_off)
    ptrs = a.ptrs()
    ptrs.insert(k, a.out)
    lens = [len(p) for p in polys]
    plugin.fr_lincomb_device(a.out, n_out, ptrs, lens, coeffs)
    assert np.array_equal(a.result(), want), (count, which)


def test_refused_overlaps_and_errors():
    n = 512
    buf = HipMem.from_numpy(np.full((3 * n, 4), GUARD, dtype=np.uint64))
    other = HipMem.from_numpy(lc.rnd(n, 1))
    c = lc.rnd(2, 7)
    L = _lib.lib()

    def refused(out, n_out, ptrs, lens, coeffs, on_device=1):
        pp, pl, cs = lc.call_args(ptrs, lens, coeffs)
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_hip_fr_lincomb(out, n_out, len(ptrs), pp, pl, cs.ctypes.data, on_device))
        assert e.value.code == INVALID_VALUE, e.value

    refused(buf.ptr + 32, n, [buf.ptr, other.ptr], [n, n], c)            # out one element into an operand
    refused(buf.ptr, n, [other.ptr, buf.ptr + 32 * (n - 1)], [n, 9], c)  # an operand starting inside out
    refused(buf.ptr, n - 1, [other.ptr], [n], c[:1])                     # an operand longer than n_out
    pp, pl, cs = lc.call_args([0], [0], c[:1])
    pl[0] = 4
    with pytest.raises(_lib.HipError) as e:                             # a missing pointer
        _lib.check(L.snarkvm_hip_fr_lincomb(buf.ptr, n, 1, pp, pl, cs.ctypes.data, 1))
    assert e.value.code == INVALID_VALUE
    host = lc.rnd(n, 2)
    refused(buf.ptr, n, [other.ptr, host.ctypes.data], [n, n], c)        # a host operand among device operands
    assert (buf.download(dtype=np.uint64) == GUARD).all()               # no partial result
    # an operand that ends where out begins is not an overlap
    plugin.fr_lincomb_device(buf.ptr + 32 * n, n, [buf.ptr, other.ptr], [n, n], c)


def test_inside_a_scope_with_the_opening_division_behind_it():
    """lincomb -> snarkvm_hip_fr_divide_by_linear on device memory inside one scope: the quotient is the opening witness, the remainder the
    combination's evaluation (get_lc_eval); a repeat of the calls grows no workspace"""
    n = 3000
    count = lc.CHUNK + 3
    coeffs, polys = lc.make_case(count, n, 4)
    z = lc.rnd(1, 9)
    comb = lc.expected(coeffs, polys, n)
    one = oracle.fr_op("from_bigint", np.array([[1, 0, 0, 0]], dtype=np.uint64))
    want_q, _ = oracle.poly_divide(comb, [(0, oracle.fr_op("neg", z)[0]), (1, one[0])])
    a = Arena(polys, n)
    quot = HipMem(32 * n)
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    for attempt in range(2):
        rem = np.zeros((1, 4), dtype=np.uint64)
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(a.mem.ptr)))
        try:
            plugin.fr_lincomb_device(a.out, n, a.ptrs(), a.lens, coeffs)
            _lib.check(L.snarkvm_hip_fr_divide_by_linear(ctypes.c_void_p(quot.ptr), ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(a.out), ctypes.c_size_t(n),
                                                         ctypes.c_void_p(z.ctypes.data), 1))
        finally:
            _lib.check(L.snarkvm_hip_scope_end())
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        else:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        assert np.array_equal(a.result(), comb)
        got_q = quot.download(32 * (n - 1), dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(got_q[: len(want_q)], want_q) and not got_q[len(want_q) :].any()
        assert np.array_equal(rem, oracle.poly_evaluate(comb, z))
    assert not stats[:4].any(), stats


def test_a_repeated_host_call_grows_no_workspace():
    coeffs, polys = lc.make_case(7, 1000, 1)
    L = _lib.lib()
    run(coeffs, polys, 1000, 0)
    L.snarkvm_hip_alloc_stats(None, 1)
    got = run(coeffs, polys, 1000, 0)
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert np.array_equal(got, lc.expected(coeffs, polys, 1000))


def test_poly_lincomb_trims_like_a_dense_polynomial():
    from snarkvm_amd import poly

    p, q = lc.rnd(50, 1), lc.rnd(80, 2).copy()
    q[50:] = 0
    minus_one = util.ints_to_fr_mont([lc.R - 1])
    got = poly.lincomb(np.concatenate([sonic_pc.FR_ONE.reshape(1, 4), minus_one]), [p, p])
    assert got.shape == (0, 4)  # p - p
    got = poly.lincomb(lc.rnd(2, 7), [p, q])
    assert np.array_equal(got, lc.expected(lc.rnd(2, 7), [p, q], 80)[:50]) and got.shape[0] == 50
    assert poly.lincomb([], []).shape == (0, 4)


# ---- SonicKZG10.open_combinations (sonic_pc/mod.rs:413-473) -------------------------------------------------------------------
class Challenges:
    """Stand-in for the Fiat-Shamir sponge: hands out a fixed list of Fr challenges in order."""

    def __init__(self, seed, n=32):
        self.vals = lc.rnd(n + seed, 6)[seed:].copy()
        self.vals[1] = sonic_pc.FR_ONE  # `coeff.is_one()` takes the plain-addition branch (mod.rs:555-557)
        self.k = 0

    def squeeze_short_nonnative_field_element(self):
        v = self.vals[self.k]
        self.k += 1
        return v


def _linear_divisor(point):
    one = oracle.fr_op("from_bigint", np.array([[1, 0, 0, 0]], dtype=np.uint64))
    return [(0, oracle.fr_op("neg", np.asarray(point).reshape(1, 4))[0]), (1, one[0])]


def test_open_combinations_matches_reference_formulas():
    G = util.g1_generator_affine()
    N = 400  # max_degree + 1
    powers = oracle.g1_gen_bases(G, 1, N)
    gamma = oracle.g1_gen_bases(G, 5000, 8)
    bounds = [200, 399]
    shifted = oracle.g1_gen_bases(G, 9000, bounds[-1] + 1)
    shifted_gamma = {b: oracle.g1_gen_bases(G, 20000 + b, 4) for b in bounds}
    ck = sonic_pc.CommitterUnionKey(powers, gamma, shifted, shifted_gamma, bounds)
    LP, LC, ONE = sonic_pc.LabeledPolynomial, sonic_pc.LinearCombination, sonic_pc.ONE
    polys = [LP("a", lc.rnd(N, 1)), LP("b", lc.rnd(300, 2)), LP("h", lc.rnd(257, 3), hiding_bound=2), LP("g", lc.rnd(120, 4), hiding_bound=1),
             LP("bounded", lc.rnd(180, 5), degree_bound=200, hiding_bound=1)]
    rands = [kzg10.KZGRandomness.empty(), kzg10.KZGRandomness.empty(), kzg10.KZGRandomness(lc.rnd(4, 11).copy()), kzg10.KZGRandomness(lc.rnd(3, 12).copy()),
             kzg10.KZGRandomness(lc.rnd(3, 13).copy())]
    c = lc.rnd(8, 8)
    lcs = [
        LC.new("lc_one", [(c[0], "a"), (c[1], ONE), (c[2], "h"), (c[3], "a")]),  # a ONE term (skipped), "a" twice (merged), the hiding polynomial "h"
        LC.new("lc_bounded", [(sonic_pc.FR_ONE, "bounded")]),                    # degree-bounded: alone, coefficient one
        LC.new("lc_shared", [(c[4], "h"), (c[5], "b"), (c[6], "g")]),            # "h" again: one hiding polynomial shared by two combinations
    ]
    z1, z2 = lc.rnd(1, 21), lc.rnd(1, 22)
    query_set = [("lc_one", ("beta", z1)), ("lc_shared", ("beta", z1)), ("lc_shared", ("alpha", z2)), ("lc_bounded", ("alpha", z2))]
    proofs = sonic_pc.SonicKZG10.open_combinations(N - 1, ck, lcs, polys, rands, query_set, Challenges(3))

    # ---- the same from the oracle: AXPY chains, poly_divide, g1_msm
    by_label = {p.label: (p.coeffs, r.blinding_polynomial) for p, r in zip(polys, rands)}
    c03 = oracle.fr_op("add", c[0:1], c[3:4])[0]
    terms = {"lc_one": [(c03, "a"), (c[2], "h")], "lc_bounded": [(sonic_pc.FR_ONE, "bounded")], "lc_shared": [(c[4], "h"), (c[5], "b"), (c[6], "g")]}
    lc_poly, lc_rand = {}, {}
    for name, ts in terms.items():
        n_p = max(len(by_label[t][0]) for _, t in ts)
        n_r = max(len(by_label[t][1]) for _, t in ts)
        lc_poly[name] = lc.expected([k for k, _ in ts], [by_label[t][0] for _, t in ts], n_p)
        lc_rand[name] = lc.expected([k for k, _ in ts], [by_label[t][1] for _, t in ts], n_r)
    chal = Challenges(3)
    for proof, (name, point, labels) in zip(proofs, [("alpha", z2, ["lc_bounded", "lc_shared"]), ("beta", z1, ["lc_one", "lc_shared"])]):
        ch = [chal.squeeze_short_nonnative_field_element() for _ in labels]
        comb = lc.expected(ch, [lc_poly[lb] for lb in labels], max(len(lc_poly[lb]) for lb in labels))
        comb_r = lc.expected(ch, [lc_rand[lb] for lb in labels], max(len(lc_rand[lb]) for lb in labels))
        chal.squeeze_short_nonnative_field_element()  # the unused `_randomizer`
        wq, _ = oracle.poly_divide(comb, _linear_divisor(point))
        want_w = oracle.g1_msm(powers[: wq.shape[0]], oracle.fr_op("to_bigint", wq))
        bq, _ = oracle.poly_divide(comb_r, _linear_divisor(point))
        want_w = oracle.g1_add(want_w, oracle.g1_msm(gamma[: bq.shape[0]], oracle.fr_op("to_bigint", bq)))
        assert util.affine_equal(np.array([proof.w]), oracle.g1_to_affine(want_w)), name
        assert np.array_equal(proof.random_v, oracle.poly_evaluate(comb_r, point)), name

    # ---- the three error paths
    with pytest.raises(kzg10.PCError, match="MissingPolynomial"):
        sonic_pc.SonicKZG10.open_combinations(N - 1, ck, [LC.new("bad", [(c[0], "nope")])], polys, rands, [("bad", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="EquationHasDegreeBounds"):
        sonic_pc.SonicKZG10.open_combinations(N - 1, ck, [LC.new("bad", [(sonic_pc.FR_ONE, "bounded"), (c[0], "a")])], polys, rands, [("bad", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="must be one"):
        sonic_pc.SonicKZG10.open_combinations(N - 1, ck, [LC.new("bad", [(c[0], "bounded")])], polys, rands, [("bad", ("beta", z1))], Challenges(1))
    ck.close()
