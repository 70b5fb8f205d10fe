"""`snarkvm_hip_fr_witness_evals` and `snarkvm_hip_fr_rowcheck_fold` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_witness_evals_kernel,
fr_rowcheck_fold_kernel): host and device operands, member counts across the launch boundary, exact violation counts, skipped outputs, refusals,
one size past the cap of the launch grid, inside a scope, on two logical devices, and the drivers of rounds 1 and 2 built on them
(snarkvm_amd/matrices.py: witness_poly_device, rowcheck_witness) against the committed Varuna fixture and against the oracle's restatement of the
reference's own route (second.rs:104-122: the doubled domain, long division, per-instance scaling).

Every comparison is bit-exact.  Expected values: tests/helpers/rowcheck_cases.py (per-element Python integers; the C++ oracle; never the coset
route); the host replay of the kernels must give the same bytes as the device.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, matrices, plugin, poly
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import DevicePoly, RegisteredMatrix, RowcheckCircuit
from tests import util
from tests.helpers import rowcheck_cases as rc
from tests.helpers import selector_cases as sel

pytestmark = pytest.mark.gpu

R = rc.R
CHUNK = rc.CHUNK
FILL = 0x5A5A5A5A5A5A5A5A
GRID_CAP = 8192 * 256  # the cap as it stands in fr_call.hip.h: fr_grid, 8192 workgroups of 256 threads


class Block:
    """vectors in ONE device block, a guard element in front of the first and behind every one"""

    def __init__(self, vectors, device=-1):
        self.lens = [len(v) for v in vectors]
        self.off, at = [], 1
        for n in self.lens:
            self.off.append(at)
            at += n + 1
        self.host = np.full((at, 4), rc.GUARD, dtype=np.uint64)
        for o, v in zip(self.off, vectors):
            self.host[o : o + len(v)] = v
        self.mem = HipMem.from_numpy(self.host, device)

    def ptr(self, j):
        return self.mem.ptr + 32 * self.off[j]

    def results(self):
        now = self.mem.download(dtype=np.uint64).reshape(-1, 4)
        inside = np.zeros(len(now), dtype=bool)
        for o, n in zip(self.off, self.lens):
            inside[o : o + n] = True
        assert (now[~inside] == rc.GUARD).all(), "a guard was written"
        return [now[o : o + n] for o, n in zip(self.off, self.lens)]

    def free(self):
        self.mem.free()


def fold(arrays, mus, n, want="ov", on_device=1, device=-1):
    """-> (out, violations list) through snarkvm_hip_fr_rowcheck_fold, None for the outputs not wanted; members are checked to be unchanged"""
    k = len(arrays[0])
    if not on_device:
        pa, pb, pc = rc.pointer_lists(arrays, n)
        out = rc.guarded(n) if "o" in want else None
        viol = rc.guarded(k, 1) if "v" in want else None
        mu = np.ascontiguousarray(mus, dtype=np.uint64).reshape(-1, 4) if k and mus is not None else sel.ZERO.copy()
        _lib.check(_lib.lib().snarkvm_hip_fr_rowcheck_fold(out[1:].ctypes.data if out is not None else None, viol[1:].ctypes.data if viol is not None else None, n, k,
                                                           pa, pb, pc, mu.ctypes.data if len(mu) else None, 0))
        return (None if out is None else rc.unguard(out, n).copy(), None if viol is None else [int(x) for x in rc.unguard(viol, k)[:, 0]])
    flat = [v for vs in arrays for v in vs]
    ins = Block(flat, device)
    outs = Block([np.full((n, 4), FILL, dtype=np.uint64)], device)
    ptrs = [[ins.ptr(j * k + m) for m in range(k)] for j in range(3)]
    counts = plugin.fr_rowcheck_fold_device(outs.ptr(0) if "o" in want else None, n, ptrs[0], ptrs[1], ptrs[2], mus if "o" in want else None, violations="v" in want)
    res = outs.results()[0]
    for got, v in zip(ins.results(), flat):
        assert np.array_equal(got, v), "a member was written"
    if "o" not in want:
        assert (res == FILL).all(), "a skipped output was written"
    ins.free(), outs.free()
    return (res.copy() if "o" in want else None, None if counts is None else [int(x) for x in counts])


def check(arrays, ints, mus, mu_ints, n, want="ov", on_device=1, twin=True):
    out, viol = fold(arrays, mus, n, want, on_device)
    if "o" in want:
        assert np.array_equal(out, rc.expected_fold(ints, mu_ints, n))
    if "v" in want:
        assert viol == rc.expected_violations(ints)
    if twin:
        t_out, t_viol = rc.selftest_fold(arrays, mus, n, want)
        assert (out is None and t_out is None) or out.tobytes() == t_out.tobytes()
        assert viol == t_viol
    return out, viol


# ---- the cases of the host file, on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", rc.SIZES)
def test_fold_and_counts(n, on_device):
    for count in rc.COUNTS:
        if count == 0 and n == 0:
            continue
        arrays, ints = rc.members(n, count, n + count)
        mus, mu_ints = rc.multipliers(count, count)
        if count == 0 and on_device:
            outs = Block([np.full((n, 4), FILL, dtype=np.uint64)])
            plugin.fr_rowcheck_fold_device(outs.ptr(0), n, [], [], [], mus)
            assert not outs.results()[0].any()  # no member: zero-filled
            outs.free()
            continue
        if count == 0:
            out, _ = poly.rowcheck_fold([], [], [], mus)
            assert out.shape == (0, 4)
            continue
        check(arrays, ints, mus, mu_ints, n, on_device=on_device)


@pytest.mark.parametrize("on_device", [0, 1])
def test_repeated_device_vectors_special_operands_and_skipped_outputs(on_device):
    n = 257
    arrays = tuple([rc.special(n, 3 * k + j) for k in range(3)] for j in range(3))
    ints = tuple([util.fr_mont_to_ints(v) for v in vs] for vs in arrays)
    check(arrays, ints, rc.mont(rc.MULTIPLIERS), rc.MULTIPLIERS, n, on_device=on_device)
    arrays, ints = rc.members(n, CHUNK + 1, 11)
    mus, mu_ints = rc.multipliers(CHUNK + 1, 11)
    check(arrays, ints, mus, mu_ints, n, want="o", on_device=on_device)
    check(arrays, ints, mus, mu_ints, n, want="v", on_device=on_device)
    if on_device:  # ONE device vector as a, b and c of two members: members may repeat and overlap each other
        v = rc.mixed(n, 4)
        vi = util.fr_mont_to_ints(v)
        ins, outs = Block([v]), Block([np.zeros((n, 4), dtype=np.uint64)])
        counts = plugin.fr_rowcheck_fold_device(outs.ptr(0), n, [ins.ptr(0)] * 2, [ins.ptr(0)] * 2, [ins.ptr(0)] * 2, rc.mont([3, 4]))
        assert util.fr_mont_to_ints(outs.results()[0]) == [7 * (x * x - x) % R for x in vi]
        assert [int(c) for c in counts] == [sum(1 for x in vi if x * x % R != x)] * 2
        ins.free(), outs.free()
    else:
        out, viol = poly.rowcheck_fold(*arrays, mus)
        assert np.array_equal(out, rc.expected_fold(ints, mu_ints, n)) and [int(c) for c in viol] == rc.expected_violations(ints)


@pytest.mark.parametrize("on_device", [0, 1])
def test_violation_counts_are_exact_per_member(on_device):
    """none; one at index 0; one at n - 1; one in a member of the second launch; every element of one member"""
    n, count = 257, CHUNK + 3
    arrays, ints = rc.valid_members(n, count, 7)
    mus, mu_ints = rc.multipliers(count, 8)
    out, viol = check(arrays, ints, mus, mu_ints, n, on_device=on_device)
    assert viol == [0] * count and not out.any()

    def spoil(k, i):
        ints[2][k][i] = (ints[2][k][i] + 1) % R
        arrays[2][k][i] = rc.mont([ints[2][k][i]])[0]

    spoil(2, 0), spoil(5, n - 1), spoil(CHUNK + 1, 100)
    for i in range(n):
        spoil(1, i)
    want = [0] * count
    want[2] = want[5] = want[CHUNK + 1] = 1
    want[1] = n
    _, viol = check(arrays, ints, mus, mu_ints, n, on_device=on_device)
    assert viol == want


def test_one_size_past_the_cap_of_the_launch_grid():
    """n = 2^21 + 77 elements: the grid-stride loops of both kernels take a second trip; violations in the first and in the second trip"""
    n = GRID_CAP + 77
    a, b = rc.rnd(n, 70), rc.rnd(n, 71)
    c = oracle.fr_vec_op("mul", a, b)
    spoiled = [5, GRID_CAP - 1, GRID_CAP, n - 1]
    c[spoiled] = oracle.fr_vec_op("add", c[spoiled], np.tile(rc.mont([1]), (len(spoiled), 1)))
    mu = rc.rnd(2, 72)
    ins, outs = Block([a, b, c]), Block([np.zeros((n, 4), dtype=np.uint64)])
    counts = plugin.fr_rowcheck_fold_device(outs.ptr(0), n, [ins.ptr(0)] * 2, [ins.ptr(1)] * 2, [ins.ptr(2), ins.ptr(0)], mu)
    want = oracle.fr_vec_op("add", oracle.fr_vec_op("scale", oracle.fr_vec_op("mul_sub", a, b, c), mu[0:1]), oracle.fr_vec_op("scale", oracle.fr_vec_op("mul_sub", a, b, a), mu[1:2]))
    assert np.array_equal(outs.results()[0], want)
    assert int(counts[0]) == len(spoiled) and int(counts[1]) == int((oracle.fr_vec_op("mul", a, b) != a).any(axis=1).sum())
    # the gather of round 1 at the same size: input_size = n / 3 does not divide 2^k, ratio 3
    n3 = n - n % 3
    w = rc.rnd(n3 - n3 // 3 - 5, 73)
    d_w = HipMem.from_numpy(w)
    plugin.fr_witness_evals_device(outs.ptr(0), n3, d_w.ptr, len(w), ins.ptr(0), n3 // 3)
    assert np.array_equal(outs.results()[0][:n3], rc.expected_witness_evals(w, a[:n3], n3 // 3))
    ins.free(), outs.free(), d_w.free()


@pytest.mark.parametrize("on_device", [0, 1])
def test_witness_evals(on_device):
    for n in (8, 48, 256):
        x = rc.mixed(n, n)
        for ratio in (1, 2, 4, n):
            input_size = n // ratio
            room = n - input_size
            for w_len in sorted({0, min(1, room), max(room - 1, 0), room}):
                w = rc.mixed(w_len, ratio + w_len) if w_len else np.zeros((0, 4), dtype=np.uint64)
                want = rc.expected_witness_evals(w, x, input_size)
                assert want.tobytes() == rc.selftest_witness(w, x, input_size).tobytes()
                if not on_device:
                    assert np.array_equal(poly.witness_evals(w, x, input_size), want), (n, ratio, w_len)
                    continue
                blk = Block([w, x, np.full((n, 4), FILL, dtype=np.uint64)])
                plugin.fr_witness_evals_device(blk.ptr(2), n, blk.ptr(0), w_len, blk.ptr(1), input_size)
                got_w, got_x, got = blk.results()
                assert np.array_equal(got, want) and np.array_equal(got_w, w) and np.array_equal(got_x, x), (n, ratio, w_len)
                plugin.fr_witness_evals_device(blk.ptr(1), n, blk.ptr(0), w_len, blk.ptr(1), input_size)  # in place
                assert np.array_equal(blk.results()[1], want), (n, ratio, w_len)
                blk.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(_lib.HipError) as e:
        fn()
    assert e.value.code == rc.INVALID_VALUE and e.value.message, e.value


def test_refusals_leave_every_output_untouched():
    L = _lib.lib()
    n = 9
    arrays, ints = rc.members(n, 2, 5)
    flat = [v for vs in arrays for v in vs]
    mu = rc.rnd(2, 3)
    ins = Block(flat)
    outs = Block([np.full((n, 4), FILL, dtype=np.uint64)])
    host = np.full((16, 4), rc.GUARD, dtype=np.uint64)
    viol = rc.guarded(2, 1)
    ptrs = lambda *xs: (ctypes.c_void_p * len(xs))(*xs)
    pa, pb, pc = ptrs(ins.ptr(0), ins.ptr(1)), ptrs(ins.ptr(2), ins.ptr(3)), ptrs(ins.ptr(4), ins.ptr(5))

    def call(o=outs.ptr(0), v=viol[1:].ctypes.data, n=n, count=2, a=pa, b=pb, c=pc, mus=mu.ctypes.data, on_device=1):
        return lambda: _lib.check(L.snarkvm_hip_fr_rowcheck_fold(o, v, n, count, a, b, c, mus, on_device))

    for bad in (dict(n=(1 << 28) + 1), dict(a=None), dict(b=None), dict(c=None), dict(mus=None), dict(a=ptrs(ins.ptr(0), None)), dict(c=ptrs(None, ins.ptr(5))),
                dict(o=ins.ptr(0) + 32 * (n - 1)), dict(o=ins.ptr(3) - 32 * (n - 1)), dict(o=ins.ptr(5)),   # out over a member
                dict(o=host.ctypes.data), dict(b=ptrs(ins.ptr(2), host.ctypes.data))):                     # pointers that are not on one device
        _refused(call(**bad))
    big = 65536
    _refused(call(count=big, a=(ctypes.c_void_p * big)(), b=(ctypes.c_void_p * big)(), c=(ctypes.c_void_p * big)(), mus=np.zeros((big, 4), dtype=np.uint64).ctypes.data))
    # the gather: the refusals of the header
    x, w = ins.ptr(0), ins.ptr(2)

    def gather(o=outs.ptr(0), n=8, w=w, w_len=4, x=x, input_size=4, on_device=1):
        return lambda: _lib.check(L.snarkvm_hip_fr_witness_evals(o, n, w, w_len, x, input_size, on_device))

    for bad in (dict(input_size=0), dict(input_size=3), dict(n=(1 << 28) + 4), dict(w_len=5), dict(o=None), dict(x=None), dict(w=None), dict(o=x + 32), dict(o=w - 32 * 7),
                dict(x=host.ctypes.data), dict(w=host.ctypes.data)):
        _refused(gather(**bad))
    assert (host == rc.GUARD).all() and (viol == rc.GUARD).all()
    assert (outs.results()[0] == FILL).all()
    for got, v in zip(ins.results(), flat):
        assert np.array_equal(got, v)
    # successes that touch nothing and need no device: no output given; n == 0
    call(o=None, v=None)()
    call(n=0, v=None)()
    gather(n=0, w_len=0)()
    assert (outs.results()[0] == FILL).all()
    call()()  # and the call the refusals vary succeeds
    assert np.array_equal(outs.results()[0], rc.expected_fold(ints, util.fr_mont_to_ints(mu), n))
    assert [int(c) for c in rc.unguard(viol, 2)[:, 0]] == rc.expected_violations(ints)
    ins.free(), outs.free()


# ---- round 1 -------------------------------------------------------------------------------------------------------------------------------------
def _poly(values, device=-1):
    mem = HipMem.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4) if len(values) else np.zeros((1, 4), dtype=np.uint64), device)
    return DevicePoly(mem.ptr, len(values), mem)


def _witness_poly(private, x_poly, lg_v):
    """matrices.witness_poly_device over uploaded operands -> the coefficients, the guard behind them checked"""
    V, X = 1 << lg_v, len(x_poly)
    d_w, d_x = _poly(private), _poly(x_poly)
    out = HipMem.from_numpy(np.full((V - X + 1, 4), rc.GUARD, dtype=np.uint64))
    assert matrices.witness_poly_device(d_w, len(private), d_x, X, lg_v, out) == V - X
    now = out.download(dtype=np.uint64).reshape(-1, 4)
    assert (now[V - X] == rc.GUARD).all()
    return now[: V - X].copy()


def _w_expected(private, x_poly, lg_v):
    V, X = 1 << lg_v, len(x_poly)
    evals = rc.expected_witness_evals(private, oracle.ntt(rc.pad(x_poly, V)), X)
    q, rem = oracle.poly_divide(oracle.ntt(evals, direction=oracle.INVERSE), rc.vanishing(X))
    assert rem.shape[0] == 0
    return rc.pad(q, V - X)


def test_witness_poly_device_gives_w_lde_of_the_fixture(golden):
    fx = rc.fixture_rounds12(golden["varuna"])
    x_poly = oracle.ntt(rc.mont(fx["public"]), direction=oracle.INVERSE)
    w = _witness_poly(rc.mont(fx["private"]), x_poly, 3)
    assert util.fr_mont_to_ints(w) == fx["w_lde"]


def test_witness_poly_device_at_larger_sizes():
    """|V| = 2^10 with |X| = 16 and a full and a short witness; the stats of a repeated call do not grow"""
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    x_poly = rc.rnd(16, 5)
    for attempt, w_len in enumerate((1024 - 16, 1024 - 16, 700)):
        private = rc.mixed(w_len, 6 + w_len)
        if attempt == 1:
            L.snarkvm_hip_alloc_stats(None, 1)
        assert np.array_equal(_witness_poly(private, x_poly, 10), _w_expected(private, x_poly, 10))
        if attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats


# ---- round 2 -------------------------------------------------------------------------------------------------------------------------------------
def _device_circuits(circuits_host, device=-1):
    """the dicts of rc.reference_h0 -> RowcheckCircuit list over uploaded copies (the driver consumes them), and the blocks that own them"""
    out, keep = [], []
    for c in circuits_host:
        blk = Block([v for triple in c["z"] for v in triple], device)
        keep.append(blk)
        z = [tuple(blk.ptr(3 * i + j) for j in range(3)) for i in range(len(c["z"]))]
        out.append(RowcheckCircuit(c["lg_r"], rc.mont([c["circuit_combiner"]])[0], rc.mont(c["instance_combiners"]), z))
    return out, keep


def test_round_two_of_the_fixture_from_x_and_w(golden):
    """x, w -> assignment_device -> RegisteredMatrix.mul_device (A, B, C) -> rowcheck_witness equals the fixture's h_0: z = public ++ private is the
    variable vector the three matrices multiply; the assignment polynomial of round 3 comes out of the same w"""
    fx = rc.fixture_rounds12(golden["varuna"])
    x_poly = oracle.ntt(rc.mont(fx["public"]), direction=oracle.INVERSE)
    w = _witness_poly(rc.mont(fx["private"]), x_poly, 3)
    d_w, d_x = _poly(w), _poly(x_poly)
    d_z = HipMem(32 * 8)
    assert matrices.assignment_device(d_w, 4, d_x, 4, d_z) == 8
    assert util.fr_mont_to_ints(d_z.download(dtype=np.uint64).reshape(-1, 4)) == [int(v) for v in golden["varuna"]["polynomials"]["z_lde"]]
    d_vars = _poly(rc.mont(fx["public"] + fx["private"]))
    regs = [RegisteredMatrix(sel.sparse(fx["matrices"][name], 7)) for name in "ABC"]
    zs = HipMem(32 * 8 * 3)
    for m, reg in enumerate(regs):
        reg.mul_device(zs.ptr + 32 * 8 * m, 8, d_vars)
    got = zs.download(dtype=np.uint64).reshape(3, 8, 4)
    for m, name in enumerate("ABC"):
        assert util.fr_mont_to_ints(got[m]) == fx["z"][name]
    one = rc.mont([1])
    h_0 = matrices.rowcheck_witness([RowcheckCircuit(3, one[0], one, [tuple(zs.ptr + 32 * 8 * m for m in range(3))])], 3)
    assert h_0.n == 8 and h_0.violations == [0] and h_0.members == [(0, 0)]
    assert rc.trimmed_ints(h_0.download()) == fx["h_0"]
    for r in regs:
        r.close()


@pytest.fixture(scope="module")
def two_circuits():
    """|R| = 2^9 with 3 instances and 2^10 with 2, random combiners, z_c = z_a z_b; the reference's route on the oracle, computed once"""
    circuits = [rc.random_circuit(1, 9, 3), rc.random_circuit(2, 10, 2)]
    want = rc.reference_h0(circuits, 10)
    want.setflags(write=False)
    return circuits, want


def test_rowcheck_witness_of_two_circuits_against_the_reference_route(two_circuits):
    circuits, want = two_circuits
    dev, keep = _device_circuits(circuits)
    h_0 = matrices.rowcheck_witness(dev, 10)
    assert h_0.n == 1024 and h_0.members == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)] and h_0.violations == [0] * 5
    got = h_0.download()
    assert np.array_equal(got, want) and got[:1023].any() and not got[1023].any()
    # one circuit below the maximal domain: zero-padded to |R_max|, scaled by |R| / |R_max|
    dev, keep2 = _device_circuits(circuits[:1])
    assert np.array_equal(matrices.rowcheck_witness(dev, 10).download(), rc.reference_h0(circuits[:1], 10))
    for blk in keep + keep2:
        blk.free()


def test_a_violated_row_raises_and_names_the_member(two_circuits):
    circuits, _ = two_circuits
    bad = [dict(c, z=[tuple(v.copy() for v in t) for t in c["z"]]) for c in circuits]
    bad[1]["z"][1][2][700] = oracle.fr_vec_op("add", bad[1]["z"][1][2][700:701], rc.mont([1]))[0]
    with pytest.raises(ValueError, match="non-zero remainder"):
        rc.reference_h0(bad, 10)
    dev, keep = _device_circuits(bad)
    with pytest.raises(ValueError, match=r"Failed to divide by vanishing polynomial - non-zero remainder \(circuit 1, instance 1: 1 rows") as e:
        matrices.rowcheck_witness(dev, 10)
    assert "circuit 1, instance 1" in str(e.value)
    for blk in keep:
        blk.free()


def test_inside_a_scope_beside_a_transform_and_a_repeat_grows_no_workspace(two_circuits):
    """in the caller's scope every call is only enqueued: the counts arrive with scope_end and ensure_divisible() runs after it; the bytes equal the
    call outside a scope; repeated calls grow no workspace"""
    circuits, want = two_circuits
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    side = rc.rnd(1 << 11, 9)
    want_side = oracle.ntt(side)
    seen = []
    for attempt in range(3):
        dev, keep = _device_circuits(circuits)
        d_side = HipMem.from_numpy(side)
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(d_side.ptr)))
        try:
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(d_side.ptr), 11, 0, 0, 0))
            h_0 = matrices.rowcheck_witness(dev, 10)
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        assert h_0.ensure_divisible() is h_0 and h_0.violations == [0] * 5
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        got = h_0.download()
        assert np.array_equal(got, want) and np.array_equal(d_side.download(dtype=np.uint64).reshape(-1, 4), want_side), attempt
        seen.append(got.tobytes())
        for blk in keep:
            blk.free()
        d_side.free()
    assert seen[0] == seen[1] == seen[2]
    assert not stats[:4].any(), stats
    # a violated row inside the caller's scope: reported by ensure_divisible() once the scope has ended
    bad = [dict(c, z=[tuple(v.copy() for v in t) for t in c["z"]]) for c in circuits]
    bad[0]["z"][2][2][0] = oracle.fr_vec_op("add", bad[0]["z"][2][2][0:1], rc.mont([1]))[0]  # z_c of circuit 0, instance 2, row 0
    dev, keep = _device_circuits(bad)
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(keep[0].mem.ptr)))
    try:
        h_0 = matrices.rowcheck_witness(dev, 10)
    finally:
        _lib.check(L.snarkvm_hip_scope_end())
    assert h_0.violations == [0, 0, 1, 0, 0]
    with pytest.raises(ValueError, match="circuit 0, instance 2"):
        h_0.ensure_divisible()
    for blk in keep:
        blk.free()


MULTI_SCRIPT = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from snarkvm_amd import matrices, msm, plugin, poly
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import RowcheckCircuit
from tests.helpers import rowcheck_cases as rc

assert msm.num_devices() == 2, msm.num_devices()
n = 300
arrays, ints = rc.members(n, rc.CHUNK + 2, 4)
mus, mu_ints = rc.multipliers(rc.CHUNK + 2, 4)
want, want_v = rc.expected_fold(ints, mu_ints, n), rc.expected_violations(ints)
flat = np.concatenate([v for vs in arrays for v in vs])
k = rc.CHUNK + 2
circuit = rc.random_circuit(3, 9, 2)
want_h = rc.reference_h0([circuit], 9)
x = rc.rnd(64, 1)
w = rc.rnd(48, 2)
for device in (0, 1, 1, 0):
    ins = HipMem.from_numpy(flat, device)
    out = HipMem.from_numpy(np.full((n + 1, 4), rc.GUARD, dtype=np.uint64), device)
    ptrs = [[ins.ptr + 32 * n * (j * k + m) for m in range(k)] for j in range(3)]
    counts = plugin.fr_rowcheck_fold_device(out.ptr, n, ptrs[0], ptrs[1], ptrs[2], mus)
    now = out.download(dtype=np.uint64).reshape(-1, 4)
    assert np.array_equal(now[:n], want) and (now[n] == rc.GUARD).all() and [int(c) for c in counts] == want_v, device
    d_x, d_w = HipMem.from_numpy(x, device), HipMem.from_numpy(w, device)
    plugin.fr_witness_evals_device(d_x.ptr, 64, d_w.ptr, 48, d_x.ptr, 16)
    assert np.array_equal(d_x.download(dtype=np.uint64).reshape(-1, 4), rc.expected_witness_evals(w, x, 16)), device
    zs = HipMem.from_numpy(np.concatenate([v for t in circuit["z"] for v in t]), device)
    z = [tuple(zs.ptr + 32 * 512 * (3 * i + j) for j in range(3)) for i in range(2)]
    h_0 = matrices.rowcheck_witness([RowcheckCircuit(9, rc.mont([circuit["circuit_combiner"]])[0], rc.mont(circuit["instance_combiners"]), z)], 9, device=device)
    assert np.array_equal(h_0.download(), want_h), device
    for m in (ins, out, d_x, d_w, zs):
        m.free()
out, viol = poly.rowcheck_fold(*arrays, mus)
assert np.array_equal(out, want) and [int(c) for c in viol] == want_v
print("ROWCHECK_MULTI_OK")
'''


def test_two_logical_devices():
    env = dict(os.environ, SNARKVM_HIP_DEVICES="0,0")
    r = subprocess.run([sys.executable, "-c", MULTI_SCRIPT % util.ROOT], capture_output=True, text=True, env=env, timeout=300, cwd=util.ROOT)
    assert "ROWCHECK_MULTI_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
