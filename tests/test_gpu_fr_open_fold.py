"""`snarkvm_hip_fr_open_fold` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: the fr_horner(2)_up/down_kernel sweeps over fr_span_fold_t): a linear
combination of polynomials, its quotient by X - z and its value in one sweep up and one down, and the resident drivers of
snarkvm_amd/sonic_pc.py on top of it (`evaluate_combinations_device`, `open_combinations_device`).

Every comparison is bit-exact against the oracle (tests/helpers/open_fold_cases.py): its AXPY chain for the combination, poly_divide by
X - z for the quotient, poly_evaluate for the value, g1_msm for a commitment.  Lengths: every ownership edge of both routes - the chunk
levels of the recursion, the route switch at 2048, a workgroup's last and first thread, the doubling of C past 2^19, the switch back past 2^20.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, kzg10, plugin, poly, sonic_pc
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.helpers import lincomb as lc
from tests.helpers import open_fold_cases as oc

pytestmark = pytest.mark.gpu

GUARD = oc.GUARD


class Arena:
    """the operands of one call in ONE device block, each followed by a guard element; the quotient (n + guard) at the end"""

    def __init__(self, polys, n):
        self.lens = [len(p) for p in polys]
        parts, self.offs, at = [], [], 0
        for p in polys:
            self.offs.append(at)
            parts += [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4), np.full((1, 4), GUARD, dtype=np.uint64)]
            at += len(p) + 1
        self.q_off, self.n = at, n
        parts.append(np.full((n + 1, 4), GUARD, dtype=np.uint64))
        self.host = np.concatenate(parts)
        self.mem = HipMem.from_numpy(self.host)

    def ptrs(self):
        return [self.mem.ptr + 32 * o for o in self.offs]

    @property
    def quot(self):
        return self.mem.ptr + 32 * self.q_off

    def result(self):
        """the quotient buffer, after checking that nothing else has changed"""
        now = self.mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[: self.q_off], self.host[: self.q_off]), "an operand or a guard was written"
        assert (now[-1] == GUARD).all(), "the element behind the quotient was written"
        return now[self.q_off : self.q_off + self.n]


def run(coeffs, polys, z, n, on_device, want="qr"):
    """-> (quotient (n, 4) or None, value (1, 4) or None); without "q" the would-be quotient must stay guard-filled"""
    if on_device:
        a = Arena(polys, n)
        value = plugin.fr_open_fold_device(a.quot if "q" in want else None, n, a.ptrs(), a.lens, coeffs, z, remainder="r" in want)
        got = a.result()
        if "q" not in want:
            assert (got == GUARD).all()
        return (got if "q" in want else None), value
    quot = np.full((n + 1, 4), GUARD, dtype=np.uint64)
    rem = np.full((2, 4), GUARD, dtype=np.uint64)
    pp, pl, cs, zz = oc.call_args([p.ctypes.data for p in polys], [len(p) for p in polys], coeffs, z)
    _lib.check(_lib.lib().snarkvm_hip_fr_open_fold(quot.ctypes.data if "q" in want else None, rem.ctypes.data if "r" in want else None, n, len(polys), pp, pl,
                                                   cs.ctypes.data if len(polys) else None, zz.ctypes.data, 0))
    assert (quot[n] == GUARD).all() and (rem[1] == GUARD).all()
    if "q" not in want:
        assert (quot == GUARD).all()
    if "r" not in want:
        assert (rem == GUARD).all()
    return (quot[:n] if "q" in want else None), (rem[:1] if "r" in want else None)


def check(coeffs, polys, z, n, quot, value, on_device, want="qr"):
    got_q, got_v = run(coeffs, polys, z, n, on_device, want)
    if "q" in want:
        assert np.array_equal(got_q, quot), (n, on_device, want)
        assert not got_q[n - 1].any()
    if "r" in want:
        assert np.array_equal(got_v, value), (n, on_device, want)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", oc.SMALL_LENGTHS)
def test_lengths_small(n, on_device):
    coeffs, polys, z, quot, value = oc.case(n, 7, n % 5)
    check(coeffs, polys, z, n, quot, value, on_device)
    check(coeffs, polys, z, n, quot, value, on_device, "r")


@pytest.mark.parametrize("n", oc.LARGE_LENGTHS)
def test_lengths_large(n):
    coeffs, polys, z, quot, value = oc.case(n, 3)
    check(coeffs, polys, z, n, quot, value, 1)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("count", oc.COUNTS)
def test_counts_and_ragged_lengths(count, on_device):
    for n in (2050, 40):
        coeffs, polys, z, quot, value = oc.case(n, count, count % 5)
        for want in ("qr", "q", "r"):
            check(coeffs, polys, z, n, quot, value, on_device, want)


@pytest.mark.parametrize("count", [2, oc.CHUNK + 1])
def test_the_longest_member_is_shorter_than_n(count):
    for n, longest in ((2100, 1500), (50, 20)):
        coeffs, polys, z, quot, value = oc.case(n, count, 1, longest=longest)
        check(coeffs, polys, z, n, quot, value, 1)


def test_the_same_operand_twice():
    """one device vector listed twice (and a slice of it a third time): operands are only read"""
    n = 2100
    p, q = lc.rnd(n, 1), lc.rnd(700, 2)
    a = Arena([p, q], n)
    ptrs = [a.ptrs()[0], a.ptrs()[1], a.ptrs()[0], a.ptrs()[0] + 32 * 3]
    lens = [n, 700, n, 197]
    coeffs, z = lc.rnd(4, 7), oc.point("random")
    _, quot, value = oc.reference(coeffs, [p, q, p, p[3:200]], n, z)
    got_v = plugin.fr_open_fold_device(a.quot, n, ptrs, lens, coeffs, z)
    assert np.array_equal(a.result(), quot) and np.array_equal(got_v, value)


def test_everything_cancels():
    coeffs = np.concatenate([sonic_pc.FR_ONE.reshape(1, 4), util.ints_to_fr_mont([lc.R - 1])])
    for n in (2100, 33):
        p = lc.rnd(n, 2)
        got_q, got_v = run(coeffs, [p, p], oc.point("random"), n, 1)
        assert not got_q.any() and not got_v.any()


@pytest.mark.parametrize("kind", oc.KINDS)
def test_edge_values(kind):
    for n, count in ((2100, 7), (33, oc.CHUNK + 1)):
        coeffs, polys, z, quot, value = oc.case(n, count, 1, kind)
        check(coeffs, polys, z, n, quot, value, 1)


@pytest.mark.parametrize("name", oc.POINTS)
def test_points(name):
    for n in (4097, 1025):
        coeffs, polys, z, quot, value = oc.case(n, 6, 2, "mixed", name)
        check(coeffs, polys, z, n, quot, value, 1)


def test_no_coefficients_and_no_operands():
    z = oc.point("random")
    for on_device in (0, 1):
        for n in (7, 2100):
            got_q, got_v = run(np.zeros((0, 4), dtype=np.uint64), [], z, n, on_device)
            assert not got_q.any() and not got_v.any()
            got_q, got_v = run(lc.rnd(2, 7), [lc.rnd(0, 1), lc.rnd(0, 2)], z, n, on_device)
            assert not got_q.any() and not got_v.any()


def test_refused_overlaps_and_errors():
    n = 512
    buf = HipMem.from_numpy(np.full((3 * n, 4), GUARD, dtype=np.uint64))
    other = HipMem.from_numpy(lc.rnd(n, 1))
    c, z = lc.rnd(2, 7), oc.point("random")
    L = _lib.lib()
    rem = np.full((1, 4), GUARD, dtype=np.uint64)
    q = buf.ptr + 32 * n

    def refused(quot, n_, ptrs, lens, coeffs, point=z, no_coeffs=False):
        pp, pl, cs, zz = oc.call_args(ptrs, lens, coeffs, z)
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_hip_fr_open_fold(quot, rem.ctypes.data, n_, len(ptrs), pp, pl, None if no_coeffs else cs.ctypes.data,
                                                  None if point is None else zz.ctypes.data, 1))
        assert e.value.code == oc.INVALID_VALUE, e.value

    refused(q, n, [other.ptr, q], [n, n], c)                       # the quotient IS an operand: no in-place form
    refused(q, n, [other.ptr, q - 32], [n, 2], c)                  # an operand ending inside the quotient
    refused(q, n, [other.ptr, q + 32 * (n - 1)], [n, 9], c)        # an operand starting inside the quotient
    refused(q, n - 1, [other.ptr], [n], c[:1])                     # an operand longer than n
    refused(q, n, [other.ptr], [n], c[:1], point=None)             # a missing point
    refused(q, n, [other.ptr], [n], c[:1], no_coeffs=True)         # missing coeffs
    pp, pl, cs, zz = oc.call_args([0], [0], c[:1], z)
    pl[0] = 4
    with pytest.raises(_lib.HipError) as e:                        # a missing pointer
        _lib.check(L.snarkvm_hip_fr_open_fold(q, rem.ctypes.data, n, 1, pp, pl, cs.ctypes.data, zz.ctypes.data, 1))
    assert e.value.code == oc.INVALID_VALUE
    host = lc.rnd(n, 2)
    refused(q, n, [other.ptr, host.ctypes.data], [n, n], c)        # a host operand among device operands
    assert (buf.download(dtype=np.uint64) == GUARD).all() and (rem == GUARD).all()  # no partial result
    # operands that end where the quotient begins and begin where it ends are no overlap
    buf.upload(np.ascontiguousarray(lc.rnd(n, 3)))
    buf.upload(np.ascontiguousarray(lc.rnd(n, 4)), 32 * 2 * n)
    got_v = plugin.fr_open_fold_device(q, n, [buf.ptr, q + 32 * n], [n, n], c, z)
    _, quot, value = oc.reference(c, [lc.rnd(n, 3), lc.rnd(n, 4)], n, z)
    assert np.array_equal(buf.download(32 * n, 32 * n, dtype=np.uint64).reshape(-1, 4), quot) and np.array_equal(got_v, value)


@pytest.mark.parametrize("n,count", [(3000, oc.CHUNK + 3), (700, 7)])
def test_inside_a_scope_with_the_support_of_the_quotient_behind_it(n, count):
    """the call is only enqueued: the remainder arrives when the scope ends, and so does the pending support of the quotient; a repeat of the
    calls grows no workspace"""
    coeffs, polys, z, quot, value = oc.case(n, count, 4)
    a = Arena(polys, n)
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    trimmed = poly.trim(quot).shape[0]
    for attempt in range(2):
        _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(a.mem.ptr)))
        try:
            rem = plugin.fr_open_fold_device(a.quot, n, a.ptrs(), a.lens, coeffs, z)
            support = plugin.fr_support_device(a.quot, n)
            only = plugin.fr_open_fold_device(None, n, a.ptrs(), a.lens, coeffs, z)
            assert not rem.any() and not only.any()  # nothing has been delivered yet
        finally:
            _lib.check(L.snarkvm_hip_scope_end())
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        else:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        assert np.array_equal(a.result(), quot)
        assert np.array_equal(rem, value) and np.array_equal(only, value)
        assert int(support[0]) == trimmed and int(support[1]) == 0
    assert not stats[:4].any(), stats


def test_a_repeated_host_call_grows_no_workspace():
    coeffs, polys, z, quot, value = oc.case(2100, 7, 1)
    L = _lib.lib()
    run(coeffs, polys, z, 2100, 0)
    L.snarkvm_hip_alloc_stats(None, 1)
    got_q, got_v = run(coeffs, polys, z, 2100, 0)
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert np.array_equal(got_q, quot) and np.array_equal(got_v, value)


def test_poly_open_fold_trims_like_a_dense_polynomial():
    p, q = lc.rnd(50, 1), lc.rnd(80, 2).copy()
    q[50:] = 0
    z = oc.point("random")
    minus_one = util.ints_to_fr_mont([lc.R - 1])
    got_q, got_v = poly.open_fold(np.concatenate([sonic_pc.FR_ONE.reshape(1, 4), minus_one]), [p, p], z)
    assert got_q.shape == (0, 4) and not got_v.any()  # p - p
    c = lc.rnd(2, 7)
    got_q, got_v = poly.open_fold(c, [p, q], z)
    _, quot, value = oc.reference(c, [p, q], 80, z)
    assert got_q.shape[0] == 49 and np.array_equal(got_q, quot[:49]) and np.array_equal(got_v, value)
    got_q, got_v = poly.open_fold([], [], z)
    assert got_q.shape == (0, 4) and not got_v.any()


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin, poly
from snarkvm_amd.devmem import HipMem
from tests.helpers import open_fold_cases as oc

assert msm.num_devices() == 2, msm.num_devices()
for n, count in ((2100, oc.CHUNK + 2), (300, 5)):
    coeffs, polys, z, quot, value = oc.case(n, count, 4)
    flat = np.concatenate([np.ascontiguousarray(p) for p in polys])
    offs = np.cumsum([0] + [len(p) for p in polys])
    for device in (0, 1, 1, 0):
        ins = HipMem.from_numpy(flat, device)
        out = HipMem.from_numpy(np.full((n + 1, 4), oc.GUARD, dtype=np.uint64), device)
        got_v = plugin.fr_open_fold_device(out.ptr, n, [ins.ptr + 32 * int(o) for o in offs[:-1]], [len(p) for p in polys], coeffs, z)
        now = out.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[:n], quot) and (now[n] == oc.GUARD).all() and np.array_equal(got_v, value), (n, device)
        only = plugin.fr_open_fold_device(None, n, [ins.ptr + 32 * int(o) for o in offs[:-1]], [len(p) for p in polys], coeffs, z)
        assert np.array_equal(only, value), (n, device)
        ins.free(), out.free()
    got_q, got_v = poly.open_fold(coeffs, polys, z)
    assert np.array_equal(got_q, poly.trim(quot)) and np.array_equal(got_v, value)
print("OPEN_FOLD_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "OPEN_FOLD_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the two span policies under one sweep (csrc/poly.hip.h: fr_span_plain_t, fr_span_fold_t) ---------------------------------------
# a lone coefficient; one, two and three levels of the recursion; the first sizes of the scan route; a part-filled last workgroup; C = 16
TIE_LENGTHS = [1, 2, 32, 33, 1025, 2047, 2048, 2049, 3 * 2048 + 1, (1 << 19) + 1]


def fold_of_one_member_is_the_division():
    """the fold of a single resident member with coefficient one against `snarkvm_hip_fr_divide_by_linear` of that member: both instantiations
    of every sweep kernel walk the same coefficients, so quotient and value agree bit for bit - with a quotient (either route) and without"""
    L = _lib.lib()
    top = max(TIE_LENGTHS)
    z = oc.point("random")
    src = HipMem.from_numpy(lc.rnd(top, 3))
    folded = HipMem.from_numpy(np.full((top + 1, 4), GUARD, dtype=np.uint64))
    divided = HipMem.from_numpy(np.full((top, 4), GUARD, dtype=np.uint64))
    for n in TIE_LENGTHS:
        for quotient in (True, False):
            value = plugin.fr_open_fold_device(folded.ptr if quotient else None, n, [src.ptr], [n], oc.ONE, z)
            rem = np.full((1, 4), GUARD, dtype=np.uint64)
            _lib.check(L.snarkvm_hip_fr_divide_by_linear(ctypes.c_void_p(divided.ptr) if quotient else None, ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(src.ptr),
                                                         ctypes.c_size_t(n), ctypes.c_void_p(z.ctypes.data), 1))
            assert np.array_equal(value, rem), (n, quotient)
            if quotient:
                got = folded.download(32 * (n + 1), dtype=np.uint64).reshape(-1, 4)
                want = divided.download(32 * n, dtype=np.uint64).reshape(-1, 4)
                assert np.array_equal(got[: n - 1], want[: n - 1]), n
                assert not got[n - 1].any() and (got[n] == GUARD).all() and (want[n - 1] == GUARD).all(), n
    for m in (src, folded, divided):
        m.free()


TIE_SCRIPT = r'''
import sys
sys.path.insert(0, %r)
from tests.test_gpu_fr_open_fold import fold_of_one_member_is_the_division
fold_of_one_member_is_the_division()
print("OPEN_FOLD_TIE_OK")
'''


def test_fold_of_one_member_is_the_division():
    fold_of_one_member_is_the_division()


def test_fold_of_one_member_is_the_division_on_the_chunk_recursion():
    """the same with the scan route switched off (tuning horner2=0, read once per process): every length takes the recursion"""
    env = dict(os.environ, SNARKVM_HIP_TUNING="horner2=0")
    r = subprocess.run([sys.executable, "-c", TIE_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert r.returncode == 0 and "OPEN_FOLD_TIE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the resident drivers (snarkvm_amd/sonic_pc.py) ---------------------------------------------------------------------------------
class Challenges:
    """Stand-in for the Fiat-Shamir sponge: hands out a fixed list of Fr challenges in order and counts them."""

    def __init__(self, seed, n=32):
        self.vals = lc.rnd(n + seed, 6)[seed:].copy()
        self.vals[1] = sonic_pc.FR_ONE
        self.k = 0

    def squeeze_short_nonnative_field_element(self):
        v = self.vals[self.k]
        self.k += 1
        return v


def resident(polys):
    return [sonic_pc.ResidentPolynomial(p.label, HipMem.from_numpy(p.coeffs) if p.coeffs.shape[0] else 0, p.coeffs.shape[0], p.degree_bound, p.hiding_bound)
            for p in polys]


def assert_same_proofs(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array(g.w).tobytes() == np.array(w.w).tobytes()
        assert (g.random_v is None) == (w.random_v is None) and (g.random_v is None or np.array_equal(g.random_v, w.random_v))


def reference_case():
    """the case of tests/test_gpu_fr_lincomb.py::test_open_combinations_matches_reference_formulas: a ONE term, a repeated label, a hiding
    polynomial shared by two combinations and a degree-bounded combination"""
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
    lcs = [LC.new("lc_one", [(c[0], "a"), (c[1], ONE), (c[2], "h"), (c[3], "a")]), LC.new("lc_bounded", [(sonic_pc.FR_ONE, "bounded")]),
           LC.new("lc_shared", [(c[4], "h"), (c[5], "b"), (c[6], "g")])]
    z1, z2 = lc.rnd(1, 21), lc.rnd(1, 22)
    query_set = [("lc_one", ("beta", z1)), ("lc_shared", ("beta", z1)), ("lc_shared", ("alpha", z2)), ("lc_bounded", ("alpha", z2))]
    return N, ck, polys, rands, lcs, query_set, c


def test_open_combinations_device_gives_the_proofs_of_open_combinations():
    N, ck, polys, rands, lcs, query_set, c = reference_case()
    S = sonic_pc.SonicKZG10
    host_rng, dev_rng = Challenges(3), Challenges(3)
    want = S.open_combinations(N - 1, ck, lcs, polys, rands, query_set, host_rng)
    res = resident(polys)
    got = S.open_combinations_device(N - 1, ck, lcs, res, rands, query_set, dev_rng)
    assert_same_proofs(got, want)
    assert dev_rng.k == host_rng.k == 6  # two combinations and the unused randomizer per point

    # ---- the values of the combinations: the oracle's combination at the point plus the ONE coefficients
    values = S.evaluate_combinations_device(lcs, res, query_set)
    by_label = {p.label: p.coeffs for p in polys}
    terms = {"lc_one": [(c[0], "a"), (c[2], "h"), (c[3], "a")], "lc_bounded": [(sonic_pc.FR_ONE, "bounded")], "lc_shared": [(c[4], "h"), (c[5], "b"), (c[6], "g")]}
    assert set(values) == {(label, name) for label, (name, _) in query_set}
    for label, (name, z) in query_set:
        comb = lc.expected([k for k, _ in terms[label]], [by_label[t] for _, t in terms[label]], N)
        want_v = oracle.poly_evaluate(comb, z)
        if label == "lc_one":
            want_v = oracle.fr_op("add", want_v, c[1:2])
        assert np.array_equal(values[(label, name)].reshape(1, 4), want_v), (label, name)

    # ---- the error paths of open_combinations, and the padded length
    LC, z1 = sonic_pc.LinearCombination, query_set[0][1][1]
    with pytest.raises(kzg10.PCError, match="MissingPolynomial"):
        S.open_combinations_device(N - 1, ck, [LC.new("bad", [(c[0], "nope")])], res, rands, [("bad", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="MissingPolynomial"):
        S.open_combinations_device(N - 1, ck, lcs, res, rands, [("nope", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="EquationHasDegreeBounds"):
        S.open_combinations_device(N - 1, ck, [LC.new("bad", [(sonic_pc.FR_ONE, "bounded"), (c[0], "a")])], res, rands, [("bad", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="must be one"):
        S.open_combinations_device(N - 1, ck, [LC.new("bad", [(c[0], "bounded")])], res, rands, [("bad", ("beta", z1))], Challenges(1))
    with pytest.raises(kzg10.PCError, match="length mismatch"):
        S.open_combinations_device(N - 1, ck, lcs, res, rands[:-1], query_set, Challenges(1))
    padded = [sonic_pc.ResidentPolynomial("a", res[0].ptr, N + 1)] + res[1:]
    with pytest.raises(kzg10.PCError, match="TooManyCoefficients"):
        S.open_combinations_device(N - 1, ck, lcs, padded, rands, query_set, Challenges(1))

    # ---- both refuse to run inside a caller's scope
    L = _lib.lib()
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(res[0].ptr)))
    try:
        with pytest.raises(kzg10.PCError, match="not inside a scope"):
            S.evaluate_combinations_device(lcs, res, query_set)
        with pytest.raises(kzg10.PCError, match="not inside a scope"):
            S.open_combinations_device(N - 1, ck, lcs, res, rands, query_set, Challenges(3))
    finally:
        _lib.check(L.snarkvm_hip_scope_end())
    ck.close()


def test_open_combinations_device_on_the_scan_route_and_more_members_than_one_table():
    """one polynomial of 3000 coefficients (the scan route) and a point with FR_LINCOMB_CHUNK + 2 members; w also against the oracle's MSM over
    the oracle's quotient"""
    G = util.g1_generator_affine()
    N = 3000
    powers = oracle.g1_gen_bases(G, 1, N)
    gamma = oracle.g1_gen_bases(G, 5000, 8)
    ck = sonic_pc.CommitterUnionKey(powers, gamma)
    LP, LC, ONE = sonic_pc.LabeledPolynomial, sonic_pc.LinearCombination, sonic_pc.ONE
    k = oc.CHUNK + 2
    lens = [N] + [100 + 37 * j for j in range(k - 1)]
    polys = [LP(f"p{j:02d}", lc.rnd(n, 1 + j % 5) if j % 4 else lc.rnd(n + j, 2)[j:]) for j, n in enumerate(lens)]
    rands = [kzg10.KZGRandomness.empty() for _ in polys]
    c = lc.rnd(k + 1, 8)
    lcs = [LC.new("big", [(c[j], f"p{j:02d}") for j in range(k - 3)] + [(c[k], ONE)]), LC.new("tail", [(c[j], f"p{j:02d}") for j in range(k - 5, k)])]
    z = lc.rnd(1, 23)
    query_set = [("big", ("gamma", z)), ("tail", ("gamma", z))]
    S = sonic_pc.SonicKZG10
    host_rng, dev_rng = Challenges(2), Challenges(2)
    want = S.open_combinations(N - 1, ck, lcs, polys, rands, query_set, host_rng)
    res = resident(polys)
    got = S.open_combinations_device(N - 1, ck, lcs, res, rands, query_set, dev_rng)
    assert_same_proofs(got, want)
    assert dev_rng.k == host_rng.k == 3

    chal = Challenges(2)
    xi = [chal.squeeze_short_nonnative_field_element() for _ in range(2)]
    big = lc.expected([c[j] for j in range(k - 3)], [polys[j].coeffs for j in range(k - 3)], N)
    tail = lc.expected([c[j] for j in range(k - 5, k)], [polys[j].coeffs for j in range(k - 5, k)], N)
    comb = lc.expected(xi, [big, tail], N)
    wq, _ = oracle.poly_divide(comb, [(0, oracle.fr_op("neg", z)[0]), (1, oc.ONE[0])])
    want_w = oracle.g1_msm(powers[: wq.shape[0]], oracle.fr_op("to_bigint", wq))
    assert util.affine_equal(np.array([got[0].w]), oracle.g1_to_affine(want_w)) and got[0].random_v is None

    values = S.evaluate_combinations_device(lcs, res, query_set)
    assert np.array_equal(values[("big", "gamma")].reshape(1, 4), oracle.fr_op("add", oracle.poly_evaluate(big, z), c[k : k + 1]))
    assert np.array_equal(values[("tail", "gamma")].reshape(1, 4), oracle.poly_evaluate(tail, z))
    ck.close()
