"""`snarkvm_hip_fr_matrix_sumcheck_evals` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_sumcheck_evals_kernel) over registered
arithmetizations: host and device outputs, batches with skipped outputs, refusals, inside a scope, on two logical devices, and the round-4 chain
built on it (snarkvm_amd/matrices.py: matrix_sumcheck_witness, h_2) against the committed Varuna fixture and against the oracle's chain.

Every comparison is bit-exact.  Expected values are Python big ints or the C++ oracle's composition (tests/helpers/sumcheck_cases.py); the host
replay of the kernel (`snarkvm_hip_selftest_fr_sumcheck`) must give the same bytes as the device.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from snarkvm_amd import _lib, matrices, plugin
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import RegisteredArithmetization
from tests import util
from tests.helpers import reduce_cases as rc
from tests.helpers import sumcheck_cases as sc

pytestmark = pytest.mark.gpu

GUARD = sc.GUARD
R = sc.R


class Outputs:
    """the outputs of one call in ONE device block: for member m and every output in want[m] a row of ks[m] elements, a guard element before the
    first row and behind every row"""

    def __init__(self, ks, want):
        self.ks, self.want = list(ks), [want] * len(ks) if isinstance(want, str) else list(want)
        self.off, at = {}, 1
        for m, k in enumerate(self.ks):
            for w in self.want[m]:
                self.off[(m, w)] = at
                at += k + 1
        self.host = np.full((at, 4), GUARD, dtype=np.uint64)
        self.mem = HipMem.from_numpy(self.host)

    def ptrs(self, w):
        return [self.mem.ptr + 32 * self.off[(m, w)] if (m, w) in self.off else None for m in range(len(self.ks))]

    def lists(self):
        """the three pointer lists; a list is None when no member wants that output"""
        return [self.ptrs(w) if any(w in x for x in self.want) else None for w in "abf"]

    def results(self):
        """{(member, output): array} after checking that every guard still stands"""
        now = self.mem.download(dtype=np.uint64).reshape(-1, 4)
        written = np.zeros(len(now), dtype=bool)
        out = {}
        for (m, w), at in self.off.items():
            out[(m, w)] = now[at : at + self.ks[m]]
            written[at : at + self.ks[m]] = True
        assert (now[~written] == GUARD).all(), "a guard was written"
        return out

    def free(self):
        self.mem.free()


def evaluate(regs, alpha, beta, scales, want="abf", on_device=1):
    """-> {(member, output): array} through snarkvm_hip_fr_matrix_sumcheck_evals"""
    ks = [r.k for r in regs]
    if on_device:
        o = Outputs(ks, want)
        plugin.fr_sumcheck_evals_device([r.handle for r in regs], *o.lists(), alpha, beta, scales)
        res = o.results()
        o.free()
        return res
    want = [want] * len(ks) if isinstance(want, str) else want
    host = {(m, w): np.full((k + 1, 4), GUARD, dtype=np.uint64) for m, k in enumerate(ks) for w in want[m]}
    hs = (ctypes.c_void_p * len(ks))(*[r.handle for r in regs])
    lists = [(ctypes.c_void_p * len(ks))(*[host[(m, w)].ctypes.data if (m, w) in host else None for m in range(len(ks))]) for w in "abf"]
    _lib.check(_lib.lib().snarkvm_hip_fr_matrix_sumcheck_evals(hs, len(ks), lists[0], lists[1], lists[2], alpha.ctypes.data, beta.ctypes.data, scales.ctypes.data, 0))
    for (m, w), v in host.items():
        assert (v[ks[m]] == GUARD).all(), "the element behind a host output was written"
    return {key: v[: ks[key[0]]] for key, v in host.items()}


def _check(res, m, want):
    for w, x in zip("abf", want):
        if (m, w) in res:
            assert np.array_equal(res[(m, w)], x), (m, w)


# ---- kernel edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("k", sc.edge_sizes())
def test_edge_sizes(k, on_device):
    alpha, beta, scales = sc.scalars(k)
    row, col, rcv = sc.arith(k, k, alpha, beta)
    want = sc.expected_py(row, col, rcv, alpha, beta, scales)
    g = sc.geometry(k)
    twin = sc.selftest(row, col, rcv, alpha, beta, scales, g["blocks"], g["threads"])
    reg = RegisteredArithmetization(row, col, rcv)
    res = evaluate([reg], alpha, beta, scales, on_device=on_device)
    _check(res, 0, want)
    assert all(res[(0, w)].tobytes() == t.tobytes() for w, t in zip("abf", twin))
    reg.close()
    reg.close()  # idempotent


@pytest.mark.parametrize("alpha,beta,scales", [(0, 0, (0, 1, R - 1)), (R - 1, None, (R - 1, 0, 1)), (None, 0, (1, R - 1, 0))])
def test_special_challenges_and_scales(alpha, beta, scales):
    k = 3 * sc.geometry(1)["share"] * sc.geometry(1)["threads"] // 2 + 5
    al, be, scl = sc.scalars(9, alpha, beta, scales)
    row, col, rcv = sc.arith(k, 9, al, be)
    row[5], col[6] = 0, 0
    reg = RegisteredArithmetization(row, col, rcv)
    _check(evaluate([reg], al, be, scl), 0, sc.expected_py(row, col, rcv, al, be, scl))
    reg.close()


def test_every_denominator_zero_and_all_r_minus_1():
    k = 300
    al, be, scl = sc.scalars(1, R - 2, 1, (R - 1, R - 1, R - 1))
    top = np.tile(util.ints_to_fr_mont([R - 1]), (k, 1))
    zero_d = np.tile(al, (k, 1))
    regs = [RegisteredArithmetization(top, top, top), RegisteredArithmetization(zero_d, top, top)]
    res = evaluate(regs, al, be, scl)
    _check(res, 0, sc.expected_py(top, top, top, al, be, scl))
    assert not res[(1, "b")].any() and not res[(1, "f")].any() and np.array_equal(res[(1, "a")], res[(0, "a")])
    for r in regs:
        r.close()


def test_the_transfer_private_size_once():
    """|K| = 2^17, three members, against the C++ oracle's composition"""
    k = 1 << 17
    alpha, beta, scales = sc.scalars(17)
    cases = [sc.arith(k, 20 + m, alpha, beta) for m in range(3)]
    regs = [RegisteredArithmetization(*c) for c in cases]
    res = evaluate(regs, alpha, beta, scales)
    for m, c in enumerate(cases):
        _check(res, m, sc.expected_oracle(*c, alpha, beta, scales))
    for r in regs:
        r.close()


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
_batch = {}


def _batch_case():
    if not _batch:
        alpha, beta, scales = sc.scalars(8)
        g = sc.geometry(1)
        ks = [g["share"] * g["threads"] + 77, 0, 13]
        cases = [sc.arith(k, 30 + m, alpha, beta) if k else tuple(np.zeros((0, 4), dtype=np.uint64) for _ in range(3)) for m, k in enumerate(ks)]
        want = [sc.expected_py(*c, alpha, beta, scales) if len(c[0]) else None for c in cases]
        _batch.update(alpha=alpha, beta=beta, scales=scales, ks=ks, cases=cases, want=want)
    return _batch


@pytest.mark.parametrize("on_device", [0, 1])
def test_three_members_of_different_lengths_and_every_combination_of_skipped_outputs(on_device):
    b = _batch_case()
    regs = [RegisteredArithmetization(*c) for c in b["cases"]]
    combos = ["".join(c) for n in range(4) for c in itertools.combinations("abf", n)]
    for first in combos:  # the long member takes every combination, the short one the complement
        want = [first, "abf", "".join(w for w in "abf" if w not in first)]
        res = evaluate(regs, b["alpha"], b["beta"], b["scales"], want=want, on_device=on_device)
        assert set(res) == {(m, w) for m in (0, 1, 2) for w in want[m]}
        for m in (0, 2):
            _check(res, m, b["want"][m])
    for r in regs:
        r.close()


def test_sixteen_members_and_the_same_handle_twice():
    b = _batch_case()
    regs = [RegisteredArithmetization(*b["cases"][2 * (m % 2)]) for m in range(15)]
    regs.append(regs[0])  # a handle may appear twice: it is only read
    res = evaluate(regs, b["alpha"], b["beta"], b["scales"], want=["abf" if m % 3 else "f" for m in range(16)])
    for m in range(16):
        _check(res, m, b["want"][0 if m == 15 else 2 * (m % 2)])
    for r in regs[:15]:
        r.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(_lib.HipError) as e:
        fn()
    assert e.value.code == sc.INVALID_VALUE and e.value.message, e.value


def test_refusals_leave_the_outputs_untouched():
    b = _batch_case()
    L = _lib.lib()
    regs = [RegisteredArithmetization(*b["cases"][2]) for _ in range(2)]
    k = regs[0].k
    o = Outputs([k, k], "abf")
    host_out = np.full((k, 4), GUARD, dtype=np.uint64)
    al, be, scl = (x.ctypes.data for x in (b["alpha"], b["beta"], b["scales"]))

    def call(handles=None, count=2, a=None, bl=None, f=None, alpha=al, beta=be, scales=scl, on_device=1, lists=True):
        handles = [r.handle for r in regs] if handles is None else handles
        hs = (ctypes.c_void_p * max(1, len(handles)))(*handles)
        mk = lambda given, w: (ctypes.c_void_p * max(2, count))(*(o.ptrs(w) if given is None else given)) if lists else None
        return lambda: _lib.check(L.snarkvm_hip_fr_matrix_sumcheck_evals(hs, count, mk(a, "a"), mk(bl, "b"), mk(f, "f"), alpha, beta, scales, on_device))

    _refused(call(handles=[regs[0].handle] * 17, count=17))
    _refused(call(handles=[regs[0].handle, None]))
    _refused(call(alpha=None))
    _refused(call(beta=None))
    _refused(call(scales=None))
    pa, pb, pf = o.ptrs("a"), o.ptrs("b"), o.ptrs("f")
    _refused(call(a=[pa[0], pa[0]]))                      # two members into one vector
    _refused(call(bl=[pa[0] + 32 * (k - 1), pb[1]]))      # b of member 0 starts inside a of member 0
    _refused(call(f=[pf[0], pf[0] - 32]))                 # f of member 1 ends inside f of member 0
    _refused(call(a=[pa[0], host_out.ctypes.data]))       # outputs that do not live on one device
    _refused(call(a=[host_out.ctypes.data, None], bl=[None, None], f=[None, None]))  # a host vector with on_device = 1
    assert (host_out == GUARD).all()
    o.results()  # every guard stands ...
    assert np.array_equal(o.mem.download(dtype=np.uint64).reshape(-1, 4), o.host)  # ... and no output row was written either
    # successes that touch nothing: count == 0, no output wanted, every k_m == 0
    _lib.check(L.snarkvm_hip_fr_matrix_sumcheck_evals(None, 0, None, None, None, None, None, None, 1))
    call(lists=False)()
    empty = RegisteredArithmetization(*(np.zeros((0, 4), dtype=np.uint64) for _ in range(3)))
    assert empty.handle
    call(handles=[empty.handle, empty.handle])()
    assert np.array_equal(o.mem.download(dtype=np.uint64).reshape(-1, 4), o.host)
    # registration: refused before a device is needed, *handle NULL afterwards
    x = b["cases"][2][0]
    for args in ((k, None, x.ctypes.data, x.ctypes.data), (k, x.ctypes.data, x.ctypes.data, None), ((1 << 28) + 1, x.ctypes.data, x.ctypes.data, x.ctypes.data)):
        h = ctypes.c_void_p(0xDEAD)
        _refused(lambda: _lib.check(L.snarkvm_hip_fr_arith_register(ctypes.byref(h), *args)))
        assert not h.value
    _refused(lambda: _lib.check(L.snarkvm_hip_fr_arith_register(None, k, x.ctypes.data, x.ctypes.data, x.ctypes.data)))
    L.snarkvm_hip_fr_arith_free(None)
    empty.close()
    for r in regs:
        r.close()
    o.free()


# ---- runtime behaviour -------------------------------------------------------------------------------------------------------------------------
def test_inside_a_scope_and_a_repeat_grows_no_workspace():
    """enqueued in a scope with the transform behind it: the results are there after scope_end and equal the calls outside a scope; a handle freed
    before the scope ends is safe; repeats, on device and on host memory, grow no workspace"""
    from oracle import cpu as oracle

    lg = 11
    k = 1 << lg
    alpha, beta, scales = sc.scalars(12)
    row, col, rcv = sc.arith(k, 12, alpha, beta)
    want = sc.expected_oracle(row, col, rcv, alpha, beta, scales)
    want_f = oracle.ntt(want[2], direction=oracle.INVERSE)
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    seen = []
    for attempt in range(3):
        reg = RegisteredArithmetization(row, col, rcv)
        o = Outputs([k], "abf")
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(o.mem.ptr)))
        try:
            plugin.fr_sumcheck_evals_device([reg.handle], *o.lists(), alpha, beta, scales)
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(o.ptrs("f")[0]), lg, 0, 1, 0))
            if attempt == 1:
                reg.close()  # before the scope ends: the release waits for the enqueued evaluation
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        reg.close()
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        res = o.results()
        assert np.array_equal(res[(0, "a")], want[0]) and np.array_equal(res[(0, "b")], want[1]) and np.array_equal(res[(0, "f")], want_f), attempt
        seen.append(b"".join(res[(0, w)].tobytes() for w in "abf"))
        o.free()
    assert seen[0] == seen[1] == seen[2]
    assert not stats[:4].any(), stats
    reg = RegisteredArithmetization(row, col, rcv)
    evaluate([reg], alpha, beta, scales, on_device=0)
    L.snarkvm_hip_alloc_stats(None, 1)
    _check(evaluate([reg], alpha, beta, scales, on_device=0), 0, want)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    a, b, f = plugin.fr_sumcheck_evals([reg.handle], [k], alpha, beta, scales, want="af")
    assert b is None and np.array_equal(a[0], want[0]) and np.array_equal(f[0], want[2])
    reg.close()


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import RegisteredArithmetization
from tests.helpers import sumcheck_cases as sc

assert msm.num_devices() == 2, msm.num_devices()
k = 1500
alpha, beta, scales = sc.scalars(2)
row, col, rcv = sc.arith(k, 2, alpha, beta)
want = sc.expected_py(row, col, rcv, alpha, beta, scales)
reg = RegisteredArithmetization(row, col, rcv)  # a replica on both logical devices
for device in (0, 1, 1, 0):
    mem = HipMem.from_numpy(np.full((3 * (k + 1), 4), sc.GUARD, dtype=np.uint64), device)
    ptrs = [mem.ptr + 32 * j * (k + 1) for j in range(3)]
    plugin.fr_sumcheck_evals_device([reg.handle], ptrs[0:1], ptrs[1:2], ptrs[2:3], alpha, beta, scales)
    now = mem.download(dtype=np.uint64).reshape(3, k + 1, 4)
    for j in range(3):
        assert np.array_equal(now[j, :k], want[j]) and (now[j, k] == sc.GUARD).all(), (device, j)
    mem.free()
a, b, f = plugin.fr_sumcheck_evals([reg.handle], [k], alpha, beta, scales)
assert np.array_equal(a[0], want[0]) and np.array_equal(b[0], want[1]) and np.array_equal(f[0], want[2])
reg.close()
print("SUMCHECK_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "SUMCHECK_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- known answers held by the reference (tests/golden/varuna_circuit0.json) ---------------------------------------------------------------
def test_round_four_and_five_of_the_fixture(golden):
    """matrix_sumcheck_witness + h_2 on the device: g_a, g_b and h_2 of the fixture exactly (g_c of the fixture is a copy of g_b and is not asserted
    on; C is pinned through h_2), the sums equal f[0] computed in Python, the remainders are zero (the chain raises otherwise)"""
    tv = golden["varuna"]
    fx = sc.fixture(tv)
    mats = {k: matrices.SparseMatrix.from_rows([[(v, j) for j, v in enumerate(row) if v] for row in tv["instance"][k]], 7) for k in "ABC"}
    regs = [RegisteredArithmetization.from_matrix(mats[k], 8, 8, 4) for k in "ABC"]
    wit = matrices.matrix_sumcheck_witness(regs, 3, 3, fx["alpha"], fx["beta"], 8)
    for name, (total, lhs, g, a_poly, b_poly) in zip("ABC", wit):
        f_evals = util.fr_mont_to_ints(sc.expected_py(*fx["ariths"][name], fx["alpha"], fx["beta"], fx["scales"])[2])
        assert util.fr_mont_to_ints(total) == [sum(f_evals) * pow(8, -1, R) % R], name
        assert (g.n, lhs.n, a_poly.n, b_poly.n) == (7, 8, 8, 8)
        if name in fx["g"]:
            assert sc.trimmed_ints(g.download()) == fx["g"][name], name
        want = sc.chain_expected(*fx["ariths"][name], fx["alpha"], fx["beta"], fx["scales"], 8)
        for got, w in zip((total, lhs.download(), g.download(), a_poly.download(), b_poly.download()), want):
            assert np.array_equal(got, w), name
    h2 = matrices.h_2([w[1] for w in wit], fx["deltas"])
    assert sc.trimmed_ints(h2.download()) == fx["h_2"]
    for r in regs:
        r.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg_k,k_max", [((10, 10, 10), 1 << 10), ((10, 9, 10), 1 << 11)])
def test_chain_of_a_random_circuit(lg_k, k_max):
    """|R| = |C| = 2^9, |K| = 2^10 (and one member of 2^9 under a |K_max| of 2^11: the |K_M| / |K_max| multiplier) against the oracle's chain"""
    mats = sc.random_circuit(5, lg_k=lg_k)
    alpha, beta, _ = sc.scalars(5)
    ariths = [matrices.matrix_evals(m, 1 << lg, 1 << 9, 1 << 4) for m, lg in zip(mats, lg_k)]
    for got, want in zip(ariths[1], sc.arith_py(mats[1], 1 << lg_k[1], 1 << 9, 1 << 9, 1 << 4)):
        assert np.array_equal(got, want)
    scales = matrices.sumcheck_scales(9, 9, alpha, beta)
    al, be = util.fr_mont_to_ints(alpha)[0], util.fr_mont_to_ints(beta)[0]
    a_scale = (pow(al, 512, R) - 1) * (pow(be, 512, R) - 1) % R
    assert util.fr_mont_to_ints(scales) == [a_scale, 1 << 18, a_scale * pow(1 << 18, -1, R) % R]
    regs = [RegisteredArithmetization(*x) for x in ariths]
    wit = matrices.matrix_sumcheck_witness(regs, 9, 9, alpha, beta, k_max)
    lhs_want = []
    for m, (total, lhs, g, a_poly, b_poly) in enumerate(wit):
        want = sc.chain_expected(*ariths[m], alpha, beta, scales, k_max)
        assert want[5].shape[0] == 0 and want[1].any()
        for got, w in zip((total, lhs.download(), g.download(), a_poly.download(), b_poly.download()), want):
            assert np.array_equal(got, w), m
        lhs_want.append(want[1])
    deltas = rc.rnd(3, 7)
    h2 = matrices.h_2([w[1] for w in wit], deltas).download()
    n = max(len(x) for x in lhs_want)
    ints = [util.fr_mont_to_ints(x) + [0] * (n - len(x)) for x in lhs_want]
    ds = util.fr_mont_to_ints(deltas)
    assert util.fr_mont_to_ints(h2) == [sum(d * x[i] for d, x in zip(ds, ints)) % R for i in range(n)]
    for r in regs:
        r.close()


def test_chain_raises_on_a_non_zero_remainder():
    """alpha = the constraint-domain element of a row that has an entry: d = 0 at that row's entries, so f = 0 there.  With the reference's own
    scales nothing is left to divide - v_R(alpha) = 0 makes a_scale and f_scale zero, a = f = 0 and a - b f is the zero polynomial (the oracle's chain
    agrees: zero remainder, zero lhs) - so the chain must NOT raise there.  With scales that do not vanish (those of another alpha; `scales=`) a is not
    zero at those entries while b f is: the remainder is non-zero, in the oracle's chain too, and matrix_sumcheck_witness must raise."""
    from oracle import pyref

    mats = sc.random_circuit(5, lg_k=(10,))
    row_with_entry = int(np.flatnonzero(mats[0].row_lengths())[0])
    alpha = util.ints_to_fr_mont([pow(pyref.domain_group_gen(9), row_with_entry, R)])
    other_alpha, beta, _ = sc.scalars(5)
    x = matrices.matrix_evals(mats[0], 1 << 10, 1 << 9, 1 << 4)
    reg = RegisteredArithmetization(*x)
    own = matrices.sumcheck_scales(9, 9, alpha, beta)
    assert util.fr_mont_to_ints(own)[0] == 0 and util.fr_mont_to_ints(own)[2] == 0
    want = sc.chain_expected(*x, alpha, beta, own, 1 << 10)
    assert want[5].shape[0] == 0 and not want[1].any()
    ((total, lhs, g, a_poly, b_poly),) = matrices.matrix_sumcheck_witness([reg], 9, 9, alpha, beta, 1 << 10)
    for got, w in zip((total, lhs.download(), g.download(), a_poly.download(), b_poly.download()), want):
        assert np.array_equal(got, w)
    live = matrices.sumcheck_scales(9, 9, other_alpha, beta)
    assert all(util.fr_mont_to_ints(live))
    assert sc.chain_expected(*x, alpha, beta, live, 1 << 10)[5].shape[0] > 0  # the oracle's remainder is not zero either
    with pytest.raises(ValueError, match="non-zero remainder"):
        matrices.matrix_sumcheck_witness([reg], 9, 9, alpha, beta, 1 << 10, scales=live)
    reg.close()
