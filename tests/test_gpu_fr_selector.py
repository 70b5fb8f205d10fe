"""`snarkvm_hip_fr_selector_fold` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_selector_fold_kernel, fr_tile_kernel): host and device
operands, every class shape, member counts across the launch boundary, skipped outputs, refusals, one size past the cap of the launch grid, inside
a scope, on two logical devices, and the round-3 chain built on it (snarkvm_amd/matrices.py: assignment_device, lineval_sumcheck_witness)
against the committed Varuna fixture and against the oracle's restatement of third.rs:179-213 and 280-327.

Every comparison is bit-exact.  Expected values: tests/helpers/selector_cases.py (the reference's four-step selector on the C++ oracle, never
the tiling identity); the host replay of the kernel must give the same bytes as the device.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from snarkvm_amd import _lib, matrices, plugin, poly
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import DevicePoly, LinevalCircuit, RegisteredMatrix
from tests import util
from tests.helpers import selector_cases as sel
from tests.helpers import sumcheck_cases as sc

pytestmark = pytest.mark.gpu

R = sel.R
GUARD = sel.GUARD


class Block:
    """vectors in ONE device block, a guard element in front of the first and behind every one"""

    def __init__(self, vectors, device=-1):
        self.lens = [len(v) for v in vectors]
        self.off, at = [], 1
        for n in self.lens:
            self.off.append(at)
            at += n + 1
        self.host = np.full((at, 4), GUARD, dtype=np.uint64)
        for o, v in zip(self.off, vectors):
            self.host[o : o + len(v)] = v
        self.mem = HipMem.from_numpy(self.host, device)

    def ptr(self, j):
        return self.mem.ptr + 32 * self.off[j]

    def results(self):
        """the vectors now, after checking that every guard still stands"""
        now = self.mem.download(dtype=np.uint64).reshape(-1, 4)
        inside = np.zeros(len(now), dtype=bool)
        for o, n in zip(self.off, self.lens):
            inside[o : o + n] = True
        assert (now[~inside] == GUARD).all(), "a guard was written"
        return [now[o : o + n] for o, n in zip(self.off, self.lens)]

    def free(self):
        self.mem.free()


def fold(polys, src_sizes, mus, N, h_len, want="hxs", on_device=1, device=-1):
    """-> (h, xg, sums) through snarkvm_hip_fr_selector_fold, None for the outputs not wanted; members are checked to be unchanged"""
    k = len(polys)
    sizes = {"h": h_len, "x": N or 0, "s": k}
    if not on_device:
        polys, pp, pl, ps, mu = sel.arrays(polys, src_sizes, mus)
        bufs = {w: sel.guarded(sizes[w]) if w in want else None for w in "hxs"}
        at = lambda b: b[1:].ctypes.data if b is not None else None
        _lib.check(_lib.lib().snarkvm_hip_fr_selector_fold(at(bufs["h"]), h_len, at(bufs["x"]), N or 0, at(bufs["s"]), k, pp, pl, ps, mu.ctypes.data if k else None, 0))
        return tuple(None if bufs[w] is None else sel.unguard(bufs[w], sizes[w]).copy() for w in "hxs")
    ins = Block(polys, device)
    outs = Block([np.full((sizes[w], 4), GUARD + 1, dtype=np.uint64) for w in "hxs"], device)
    ptr = lambda j, w: outs.ptr(j) if w in want else None
    plugin.fr_selector_fold_device(ptr(0, "h"), h_len, ptr(1, "x"), N or 0, ptr(2, "s"), [ins.ptr(j) if len(p) else None for j, p in enumerate(polys)],
                                   [len(p) for p in polys], src_sizes, mus)
    res = outs.results()
    for got, p in zip(ins.results(), polys):
        assert np.array_equal(got, p), "a member was written"
    for j, w in enumerate("hxs"):
        if w not in want:
            assert (res[j] == GUARD + 1).all(), "a skipped output was written"
    ins.free(), outs.free()
    return tuple(res[j].copy() if w in want else None for j, w in enumerate("hxs"))


def check(polys, src_sizes, mus, N, h_len=None, want="hxs", on_device=1, twin=True):
    h_len = sel.quotient_len(polys, src_sizes) if h_len is None else h_len
    got = fold(polys, src_sizes, mus, N, h_len, want, on_device)
    exp = sel.expected(polys, src_sizes, mus, N, h_len)
    for w, g, e in zip("hxs", got, exp):
        if w in want:
            assert g is not None and np.array_equal(g, e), w
    if twin:
        for g, t in zip(got, sel.selftest(polys, src_sizes, mus, N, h_len, want)):
            assert (g is None and t is None) or g.tobytes() == t.tobytes()
    return got


# ---- the cases of the host file, on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("ratio", sel.RATIOS)
@pytest.mark.parametrize("n", sel.SRC_SIZES)
def test_class_shapes(n, ratio, on_device):
    mu = sel.rnd(1, n + ratio)
    for L in sel.class_lengths(n):
        p = sel.mixed(L, 7 * n + L)
        check([p], [n], mu, n * ratio, on_device=on_device)
        h, _, _ = check([p], [n], mu, n * ratio, h_len=max(L - n, 0) + 5, on_device=on_device)
        assert not h[max(L - n, 0) :].any()


def _members(count, n, seed):
    lens = sel.class_lengths(n)
    polys = [sel.mixed(lens[(k + seed) % len(lens)], 100 * seed + k) for k in range(count)]
    mus = sel.rnd(count, 50 + seed)
    mus[: min(count, 3)] = sel.mont(sel.MULTIPLIERS)[: min(count, 3)]
    return polys, [n] * count, mus


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("count", [1, 3, 24, 25])
def test_member_counts(count, on_device):
    polys, srcs, mus = _members(count, 8, count)
    check(polys, srcs, mus, 16, on_device=on_device)
    check(polys, srcs, mus, 8, h_len=40, on_device=on_device)


@pytest.mark.parametrize("on_device", [0, 1])
def test_mixed_source_sizes_the_same_polynomial_twice_and_special_operands(on_device):
    srcs = [256, 512, 1024, 256, 1024]
    lens = [2 * 256 + 1, 512 + 3, 3 * 1024 + 5, 255, 1024]
    check([sel.mixed(L, 11 + k) for k, L in enumerate(lens)], srcs, sel.rnd(5, 4), 1024, on_device=on_device)
    p = sel.mixed(21, 5)
    h, xg, sums = check([p, p], [8, 8], sel.mont([3, R - 3]), 16, on_device=on_device)
    assert not h.any() and not xg.any() and np.array_equal(sums[0], sums[1]) and sums.any()
    for m, mu in enumerate(sel.MULTIPLIERS):
        polys = [sel.special(L, L + m) for L in (17, 8, 29)]
        check(polys, [8, 8, 8], sel.mont([mu, sel.MULTIPLIERS[(m + 1) % 3], mu]), 16, on_device=on_device)
    top = np.tile(sel.mont([R - 1]), (3 * 64 + 5, 1))
    check([top, top], [64, 64], sel.mont([R - 1, R - 1]), 128, on_device=on_device)


def test_one_device_array_under_two_source_domains():
    """the same device vector listed twice, and a prefix of it: members may overlap each other"""
    p = sel.mixed(21, 5)
    mus = sel.rnd(3, 6)
    ins, outs = Block([p]), Block([np.zeros((13 + 4, 4), dtype=np.uint64), np.zeros((16, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)])
    plugin.fr_selector_fold_device(outs.ptr(0), 17, outs.ptr(1), 16, outs.ptr(2), [ins.ptr(0)] * 3, [21, 21, 9], [8, 4, 8], mus)
    for got, want in zip(outs.results(), sel.expected([p, p, p[:9]], [8, 4, 8], mus, 16, 17)):
        assert np.array_equal(got, want)
    ins.free(), outs.free()


@pytest.mark.parametrize("on_device", [0, 1])
def test_every_combination_of_skipped_outputs_and_empty_members(on_device):
    polys, srcs, mus = _members(5, 8, 9)
    polys[2] = sel.ZERO
    for r in range(4):
        for combo in itertools.combinations("hxs", r):
            got = check(polys, srcs, mus, 16, want="".join(combo), on_device=on_device)
            assert got[2] is None or not got[2][2].any()
    h, xg, sums = fold([], [], sel.ZERO, 8, 5, on_device=on_device)  # no member: zero-filled
    assert h.shape == (5, 4) and xg.shape == (8, 4) and not h.any() and not xg.any()
    h, xg, sums = poly.selector_fold(polys, srcs, mus, 16) if not on_device else fold(polys, srcs, mus, 16, sel.quotient_len(polys, srcs))
    for got, want in zip((h, xg, sums), sel.expected(polys, srcs, mus, 16, sel.quotient_len(polys, srcs))):
        assert np.array_equal(got, want)


def test_one_size_past_the_cap_of_the_launch_grid():
    """n = 2^20 into N = 2^22 with L = 3 2^20 + 3: h has 2^21 + 3 coefficients and the tiled part of xg 3 2^20, each more than the 8192 x 256
    threads a launch is capped at"""
    n, N = 1 << 20, 1 << 22
    L = 3 * n + 3
    assert L - n > 8192 * 256 and N - n > 8192 * 256
    check([sel.rnd(L, 77)], [n], sel.rnd(1, 78), N, twin=False)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(_lib.HipError) as e:
        fn()
    assert e.value.code == sel.INVALID_VALUE and e.value.message, e.value


def test_refusals_leave_every_output_untouched():
    L = _lib.lib()
    p0, p1 = sel.mixed(21, 1), sel.mixed(9, 2)
    mu = sel.rnd(2, 3)
    ins = Block([p0, p1])
    outs = Block([np.full((n, 4), GUARD + 1, dtype=np.uint64) for n in (13, 16, 2)])
    host = np.full((16, 4), GUARD, dtype=np.uint64)
    sizes = lambda *xs: (ctypes.c_size_t * len(xs))(*xs)
    ptrs = lambda *xs: (ctypes.c_void_p * len(xs))(*xs)
    pp, pl, ps = ptrs(ins.ptr(0), ins.ptr(1)), sizes(21, 9), sizes(8, 4)

    def call(h=outs.ptr(0), h_len=13, xg=outs.ptr(1), N=16, sums=outs.ptr(2), count=2, polys=pp, lens=pl, srcs=ps, mus=mu.ctypes.data, on_device=1):
        return lambda: _lib.check(L.snarkvm_hip_fr_selector_fold(h, h_len, xg, N, sums, count, polys, lens, srcs, mus, on_device))

    for bad in (dict(polys=None), dict(lens=None), dict(srcs=None), dict(mus=None), dict(polys=ptrs(ins.ptr(0), None)), dict(srcs=sizes(8, 0)), dict(N=0),
                dict(N=(1 << 28) + 8), dict(N=28), dict(srcs=sizes(8, 3)), dict(h_len=12), dict(h_len=(1 << 29) + 1), dict(lens=sizes(21, (1 << 29) + 1)),
                dict(h=ins.ptr(0) + 32 * 20), dict(xg=ins.ptr(1)), dict(sums=ins.ptr(0) + 32 * 5),           # an output over a member
                dict(h=outs.ptr(1) - 32 * 12), dict(sums=outs.ptr(0) + 32 * 12), dict(xg=outs.ptr(0)),       # an output over another output
                dict(xg=host.ctypes.data), dict(sums=host.ctypes.data), dict(polys=ptrs(ins.ptr(0), host.ctypes.data)),  # pointers that are not on one device
                dict(h=host.ctypes.data, xg=None, sums=None)):                                               # a host vector with on_device = 1
        _refused(call(**bad))
    big = 65536
    _refused(call(count=big, polys=(ctypes.c_void_p * big)(), lens=(ctypes.c_size_t * big)(), srcs=(ctypes.c_size_t * big)(*([1] * big)),
                  mus=np.zeros((big, 4), dtype=np.uint64).ctypes.data))
    assert (host == GUARD).all()
    assert all((v == GUARD + 1).all() for v in outs.results())
    for got, p in zip(ins.results(), (p0, p1)):
        assert np.array_equal(got, p)
    # successes that touch nothing and need no device pointer: no output given; only an empty h
    call(h=None, xg=None, sums=None)()
    call(h=outs.ptr(0), h_len=0, xg=None, sums=None, count=0, polys=None, lens=None, srcs=None, mus=None)()
    assert all((v == GUARD + 1).all() for v in outs.results())
    call()()  # and the call the refusals vary succeeds
    for got, want in zip(outs.results(), sel.expected([p0, p1], [8, 4], mu, 16, 13)):
        assert np.array_equal(got, want)
    ins.free(), outs.free()


# ---- runtime behaviour ---------------------------------------------------------------------------------------------------------------------------
def test_inside_a_scope_and_a_repeat_grows_no_workspace():
    """enqueued in a scope with a transform of xg behind it: the results are there after scope_end and equal the call outside a scope; repeats, on
    device and on host memory, grow no workspace"""
    from oracle import cpu as oracle

    lg = 11
    n = N = 1 << lg
    polys = [sel.mixed(2 * n + 2 - k, 20 + k) for k in range(3)]
    mus = sel.rnd(3, 21)
    h_len = n + 2
    want = sel.expected(polys, [n] * 3, mus, N, h_len)
    want_xg = oracle.ntt(want[1])
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    seen = []
    for attempt in range(3):
        ins = Block(polys)
        outs = Block([np.zeros((h_len, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)])
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(outs.mem.ptr)))
        try:
            plugin.fr_selector_fold_device(outs.ptr(0), h_len, outs.ptr(1), N, outs.ptr(2), [ins.ptr(j) for j in range(3)], [len(p) for p in polys], [n] * 3, mus)
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(outs.ptr(1)), lg, 0, 0, 0))
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        h, xg, sums = outs.results()
        assert np.array_equal(h, want[0]) and np.array_equal(xg, want_xg) and np.array_equal(sums, want[2]), attempt
        seen.append(h.tobytes() + xg.tobytes() + sums.tobytes())
        ins.free(), outs.free()
    assert seen[0] == seen[1] == seen[2]
    assert not stats[:4].any(), stats
    fold(polys, [n] * 3, mus, N, h_len, on_device=0)
    L.snarkvm_hip_alloc_stats(None, 1)
    for got, w in zip(fold(polys, [n] * 3, mus, N, h_len, on_device=0), want):
        assert np.array_equal(got, w)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import msm, plugin, poly
from snarkvm_amd.devmem import HipMem
from tests.helpers import selector_cases as sel

assert msm.num_devices() == 2, msm.num_devices()
n, N = 64, 128
polys = [sel.mixed(L, L) for L in (3 * n + 5, 2 * n, 7)]
mus = sel.rnd(3, 2)
h_len = 2 * n + 5
want = sel.expected(polys, [n] * 3, mus, N, h_len)
flat = np.concatenate(polys)
offs = np.concatenate([[0], np.cumsum([len(p) for p in polys])])
for device in (0, 1, 1, 0):
    ins = HipMem.from_numpy(flat, device)
    outs = HipMem.from_numpy(np.full((h_len + N + 3 + 1, 4), sel.GUARD, dtype=np.uint64), device)
    plugin.fr_selector_fold_device(outs.ptr, h_len, outs.ptr + 32 * h_len, N, outs.ptr + 32 * (h_len + N), [ins.ptr + 32 * int(o) for o in offs[:3]],
                                   [len(p) for p in polys], [n] * 3, mus)
    now = outs.download(dtype=np.uint64).reshape(-1, 4)
    assert np.array_equal(now[:h_len], want[0]) and np.array_equal(now[h_len : h_len + N], want[1]), device
    assert np.array_equal(now[h_len + N : h_len + N + 3], want[2]) and (now[-1] == sel.GUARD).all(), device
    ins.free(), outs.free()
h, xg, sums = poly.selector_fold(polys, [n] * 3, mus, N, h_len)
assert np.array_equal(h, want[0]) and np.array_equal(xg, want[1]) and np.array_equal(sums, want[2])
print("SELECTOR_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "SELECTOR_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the chain: known answers held by the reference (tests/golden/varuna_circuit0.json) ------------------------------------------------------------
def _poly(values, device=-1):
    mem = HipMem.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4) if len(values) else np.zeros((1, 4), dtype=np.uint64), device)
    return DevicePoly(mem.ptr, len(values), mem)


def _assignment(w, x, input_size):
    """assignment_device over uploaded w and x -> (DevicePoly z, host copy)"""
    d_w, d_x = _poly(w), _poly(x)
    out = HipMem(32 * (len(w) + input_size + 1))
    out.upload(np.full((1, 4), GUARD, dtype=np.uint64), 32 * (len(w) + input_size))
    n = matrices.assignment_device(d_w, len(w), d_x, input_size, out)
    assert n == len(w) + input_size
    now = out.download(dtype=np.uint64).reshape(-1, 4)
    assert (now[n] == GUARD).all()
    return DevicePoly(out.ptr, n, out), now[:n].copy()


def _z_expected(w, x, input_size):
    from oracle import cpu as oracle

    z = oracle.mul_by_vanishing(w, input_size)
    z[: len(x)] = oracle.fr_vec_op("add", z[: len(x)], x)
    return z


def _run_chain(circuits_host, alpha, eta_b, eta_c, lg_n, mask=None):
    """circuits_host: the dicts of sel.chain_expected -> the device chain's results, checked against the oracle's"""
    regs, circuits = [], []
    for c in circuits_host:
        ts = [RegisteredMatrix(t) for t in c["transposes"]]
        regs += ts
        circuits.append(LinevalCircuit(ts, c["lg_r"], c["lg_c"], sel.mont([c["circuit_combiner"]])[0], sel.mont(c["instance_combiners"]),
                                       [_poly(z) for z in c["assignments"]]))
    d_mask = None if mask is None else _poly(mask)
    h_1, xg_1, g_1, sums = matrices.lineval_sumcheck_witness(circuits, alpha[0], eta_b[0], eta_c[0], lg_n, mask=d_mask)
    want_h, want_xg, want_sums = sel.chain_expected(circuits_host, alpha, eta_b, eta_c, lg_n, mask)
    h, xg, g = h_1.download(), xg_1.download(), g_1.download()
    assert xg_1.n == 1 << lg_n and g_1.n == xg_1.n - 1 and g_1.ptr == xg_1.ptr + 32
    assert np.array_equal(xg, want_xg) and np.array_equal(g, want_xg[1:])
    assert h_1.n >= want_h.shape[0] and np.array_equal(h[: want_h.shape[0]], want_h) and not h[want_h.shape[0] :].any()
    assert len(sums) == len(want_sums)
    for got, want in zip(sums, want_sums):
        assert got.shape == want.shape and np.array_equal(got, want)
    for r in regs:
        r.close()
    return h, xg, g, sums


def test_round_three_of_the_fixture(golden):
    """assignment_device: z_lde from w_lde; lineval_sumcheck_witness: h_1, g_1 of the fixture exactly, the sums equal the sums of the products over
    C computed in Python"""
    from oracle import cpu as oracle

    fx = sel.fixture_round3(golden["varuna"])
    x = oracle.ntt(sel.mont([1, 8, 32, 128]), direction=oracle.INVERSE)
    d_z, z = _assignment(sel.mont(fx["w_lde"]), x, 4)
    assert util.fr_mont_to_ints(z) == fx["z_lde"]
    transposes = [matrices.transpose(sel.sparse(fx["matrices"][name], 7), 8, 4) for name in "ABC"]
    alpha, eta_b, eta_c = (sel.mont([fx[k]]) for k in ("alpha", "eta_b", "eta_c"))
    circuit = {"transposes": transposes, "lg_r": 3, "lg_c": 3, "circuit_combiner": 1, "instance_combiners": [1], "assignments": [z]}
    h, xg, g, sums = _run_chain([circuit], alpha, eta_b, eta_c, 3)
    assert sel.trimmed_ints(h) == fx["h_1"] and sel.trimmed_ints(g) == fx["g_1"]
    dom, zs = fx["domain"], fx["z_lde"]
    for m, t in enumerate(transposes):
        m_poly = util.fr_mont_to_ints(sel.m_at_alpha(t, 3, 3, alpha))
        at = lambda poly, w: sum(c * pow(w, i, R) for i, c in enumerate(poly)) % R
        assert util.fr_mont_to_ints(sums[0][0, m : m + 1]) == [sum(at(m_poly, w) * at(zs, w) for w in dom) % R]


def _random_circuit(seed, lg_c, instances, extra=0):
    """a circuit of sc.random_circuit at |R| = |C| = 2^lg_c with `instances` assignments w (X^16 - 1) + x of |C| + extra coefficients"""
    mats = sc.random_circuit(seed, lg_r=lg_c, lg_c=lg_c, lg_k=(lg_c, lg_c, lg_c))
    size = 1 << lg_c
    ws = [sel.mixed(size - 16 + extra, seed + 10 * i) for i in range(instances)]
    xs = [sel.rnd(16, seed + 10 * i + 1) for i in range(instances)]
    return {"transposes": [matrices.transpose(m, size, 16) for m in mats], "lg_r": lg_c, "lg_c": lg_c, "circuit_combiner": 3 + seed,
            "instance_combiners": [5 + seed + i for i in range(instances)], "w": ws, "x": xs}


def _with_assignments(c):
    c = dict(c)
    zs = [_assignment(w, x, 16) for w, x in zip(c["w"], c["x"])]
    for (_, z), w, x in zip(zs, c["w"], c["x"]):
        assert np.array_equal(z, _z_expected(w, x, 16))
    c["assignments"] = [z for _, z in zs]
    return c


def test_chain_of_a_random_circuit_with_two_instances():
    c = _with_assignments(_random_circuit(5, 9, 2))
    alpha, eta_b, eta_c = sel.rnd(3, 31)[0:1], sel.rnd(3, 31)[1:2], sel.rnd(3, 31)[2:3]
    h, _, _, sums = _run_chain([c], alpha, eta_b, eta_c, 9)
    assert h.any() and sums[0].shape == (2, 3, 4) and sums[0].any()


def test_chain_of_two_circuits_with_different_variable_domains():
    """|C| = 2^9 and 2^10 into N = 2^10: the selector of the smaller circuit tiles its remainder twice"""
    cs = [_with_assignments(_random_circuit(6, 9, 1)), _with_assignments(_random_circuit(7, 10, 2))]
    alpha, eta_b, eta_c = sel.rnd(3, 32)[0:1], sel.rnd(3, 32)[1:2], sel.rnd(3, 32)[2:3]
    _, xg, _, sums = _run_chain(cs, alpha, eta_b, eta_c, 10)
    assert [s.shape for s in sums] == [(1, 3, 4), (2, 3, 4)] and not np.array_equal(xg[:512], xg[512:])


def test_chain_with_a_long_assignment_and_a_mask_polynomial():
    """an assignment of |C| + 3 coefficients (the product domain becomes 4 |C|) and a mask polynomial of 3 N - 2 coefficients (third.rs:207-213)"""
    c = _with_assignments(_random_circuit(8, 9, 1, extra=3))
    assert len(c["assignments"][0]) == 512 + 3
    mask = sel.mixed(3 * 512 - 2, 40)
    alpha, eta_b, eta_c = sel.rnd(3, 33)[0:1], sel.rnd(3, 33)[1:2], sel.rnd(3, 33)[2:3]
    h, _, _, _ = _run_chain([c], alpha, eta_b, eta_c, 9, mask=mask)
    assert len(h) == 2 * 512 - 2 and h[513:].any()
