"""`snarkvm_hip_fr_reduce` / `snarkvm_hip_fr_support` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_reduce_kernel,
fr_support_kernel and their second launches), and what is built on them: `Evaluations.evaluate` and `KZG10.commit_resident`.

Every Fr comparison is bit-exact against Python big-int sums of the oracle's `to_bigint` values (tests/helpers/reduce_cases.py); support
triples against numpy on the host copy.  Lengths: one element, one wave and one workgroup less one / exact / plus one, several workgroups
with a ragged last one (4099), three elements past the grid cap the library reports (the stride loop runs), and 2^20 + 3.
"""
import ctypes

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, fft, kzg10, plugin, poly
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.helpers import reduce_cases as rc
from tests.test_gpu_fr_lincomb import Arena
from tests.test_gpu_parity import _srs

pytestmark = pytest.mark.gpu

INVALID_VALUE = 1  # hipErrorInvalidValue
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 4099]


def reduce_on(op, a, b, on_device):
    """one call over host arrays or over one device arena with guard elements (checked afterwards)"""
    n = len(a)
    if not on_device:
        out = np.full((2, 4), rc.GUARD, dtype=np.uint64)
        _lib.check(_lib.lib().snarkvm_hip_fr_reduce(op, out.ctypes.data, a.ctypes.data, None if b is None else b.ctypes.data, n, 0))
        assert (out[1] == rc.GUARD).all()
        return out[:1]
    arena = Arena([a] if b is None or b is a else [a, b], 0)
    pa = arena.ptr(0)
    pb = None if b is None else (pa if b is a else arena.ptr(1))
    got = plugin.fr_reduce_device(op, pa, pb, n)
    arena.result()
    return got


def support_on(v, on_device):
    n = len(v)
    if not on_device:
        return poly.support(v)
    arena = Arena([v], 0)
    got = plugin.fr_support_device(arena.ptr(0), n)
    arena.result()
    return tuple(int(x) for x in got)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_modes(n, on_device):
    a, b = np.ascontiguousarray(rc.mixed(n, 1)), np.ascontiguousarray(rc.mixed(n, 3))
    assert np.array_equal(reduce_on(rc.SUM, a, None, on_device), rc.expected(rc.SUM, a)), "sum"
    assert np.array_equal(reduce_on(rc.DOT, a, b, on_device), rc.expected(rc.DOT, a, b)), "dot"
    assert np.array_equal(reduce_on(rc.DOT, a, a, on_device), rc.expected(rc.DOT, a, a)), "a == b"
    v = a.copy()
    if n > 2:
        v[0] = v[n - 1] = 0
    assert support_on(v, on_device) == rc.expected_support(v)


def test_python_layer_on_host_arrays():
    a, b = rc.mixed(300, 1), rc.mixed(300, 3)
    assert np.array_equal(poly.inner_product(a, b), rc.expected(rc.DOT, a, b))
    assert np.array_equal(poly.vec_sum(a), rc.expected(rc.SUM, a))


def _big_case(n):
    a, b = rc.rnd(n, 1), rc.rnd(n, 2)
    xs, ys = rc.to_ints(a), rc.to_ints(b)
    arena = Arena([a, b], 0)
    got_sum = plugin.fr_reduce_device(rc.SUM, arena.ptr(0), None, n)
    got_dot = plugin.fr_reduce_device(rc.DOT, arena.ptr(0), arena.ptr(1), n)
    # support of the same buffer with a zeroed head and tail
    head, tail = 3, 5
    arena.mem.fill(32 * arena.offs[0], 0, 32 * head)
    arena.mem.fill(32 * (arena.offs[0] + n - tail), 0, 32 * tail)
    got_sup = plugin.fr_support_device(arena.ptr(0), n)
    assert np.array_equal(got_sum, rc.from_int(sum(xs)))
    assert np.array_equal(got_dot, rc.from_int(sum(x * y for x, y in zip(xs, ys))))
    nonzero = int(a[head : n - tail].any(axis=1).sum())
    assert tuple(int(x) for x in got_sup) == (n - tail, head, nonzero)
    now = arena.mem.download(dtype=np.uint64).reshape(-1, 4)
    assert (now[n] == rc.GUARD).all() and np.array_equal(now[n + 1 : 2 * n + 1], b) and (now[2 * n + 1 :] == rc.GUARD).all()


def test_three_past_the_grid_cap():
    """more elements than the capped grid has threads: every thread of the stride loop takes a second element and three a third"""
    g = rc.geometry(1 << 30)
    assert g["blocks"] == g["cap"]
    _big_case(g["cap"] * g["threads"] + 3)


def test_two_to_the_twenty_plus_three():
    _big_case((1 << 20) + 3)


@pytest.mark.parametrize("n", [257, 4099])
def test_support_placements(n):
    g = rc.geometry(n)
    assert g["blocks"] >= 2
    second = (g["threads"], min(2 * g["threads"], n) - 1)  # first and last element of the second workgroup's range
    mem = HipMem(32 * (n + 1))
    mem.upload(np.full((1, 4), rc.GUARD, dtype=np.uint64), 32 * n)
    for name, v in rc.support_cases(n, second).items():
        mem.upload(np.ascontiguousarray(v))
        got = tuple(int(x) for x in plugin.fr_support_device(mem.ptr, n))
        assert got == rc.expected_support(v), name
        assert poly.support(v) == rc.expected_support(v), name
    assert (mem.download(32, 32 * n, dtype=np.uint64) == rc.GUARD).all()


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("count", [1, 3, 8])
def test_strided(n, count):
    for stride in (n, n + 5):
        total = (count - 1) * stride + n
        a, b = np.ascontiguousarray(rc.mixed(total, 1)), np.ascontiguousarray(rc.mixed(total, 3))
        for y in range(count):  # every member its own support
            a[y * stride : y * stride + y] = 0
            a[y * stride + n - 2 * y : y * stride + n] = 0
        xs, ys = rc.to_ints(a), rc.to_ints(b)
        arena = Arena([a, b], 0)
        members = [slice(y * stride, y * stride + n) for y in range(count)]
        got = plugin.fr_reduce_strided_device(rc.SUM, arena.ptr(0), None, n, count, stride)
        assert np.array_equal(got, np.concatenate([rc.from_int(sum(xs[m])) for m in members])), (stride, "sum")
        for b_shared in (False, True):
            got = plugin.fr_reduce_strided_device(rc.DOT, arena.ptr(0), arena.ptr(1), n, count, stride, b_shared)
            want = [rc.from_int(sum(x * y for x, y in zip(xs[m], ys[:n] if b_shared else ys[m]))) for m in members]
            assert np.array_equal(got, np.concatenate(want)), (stride, b_shared)
        got = plugin.fr_support_strided_device(arena.ptr(0), n, count, stride)
        assert [tuple(int(x) for x in row) for row in got] == [rc.expected_support(a[m]) for m in members], stride
        arena.result()


def test_strided_refusals():
    n = 64
    mem = HipMem.from_numpy(rc.rnd(3 * n, 1))
    L = _lib.lib()
    out = np.full((3, 4), rc.GUARD, dtype=np.uint64)
    for err in (L.snarkvm_hip_fr_reduce_strided(rc.SUM, out.ctypes.data, mem.ptr, None, n, 2, n - 1, 0),
                L.snarkvm_hip_fr_reduce_strided(rc.DOT, out.ctypes.data, mem.ptr, mem.ptr, n, 2, n - 1, 1),
                L.snarkvm_hip_fr_support_strided(out.ctypes.data, mem.ptr, n, 2, n - 1)):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(err)
        assert e.value.code == INVALID_VALUE
    assert (out == rc.GUARD).all()
    host = rc.rnd(n, 2)
    with pytest.raises(_lib.HipError):  # a host operand beside a device operand
        plugin.fr_reduce_device(rc.DOT, mem.ptr, host.ctypes.data, n)


def test_inside_a_scope_behind_a_transform():
    """ntt_device -> fr_reduce DOT of the transform with a second vector -> fr_support of it, all enqueued inside one scope: the values arrive at
    scope_end and are those of the oracle's transform; the same calls outside a scope give the same bytes; a repeat grows no workspace"""
    lg = 12
    n = 1 << lg
    x, y = rc.rnd(n, 1).copy(), rc.rnd(n, 2)
    x[n - 7 :] = 0
    transformed = oracle.ntt(x)
    want_dot, want_sup = rc.expected(rc.DOT, transformed, y), rc.expected_support(transformed)
    L = _lib.lib()
    stats = np.zeros(5, dtype=np.uint64)
    results = []
    arena = Arena([x, y], 0)
    for attempt in range(3):
        arena.mem.upload(x)  # the transform is in place
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(arena.mem.ptr)))
        try:
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(arena.ptr(0)), lg, 0, 0, 0))
            dot = plugin.fr_reduce_device(rc.DOT, arena.ptr(0), arena.ptr(1), n)
            sup = plugin.fr_support_device(arena.ptr(0), n)
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        assert np.array_equal(dot, want_dot), attempt
        assert tuple(int(v) for v in sup) == want_sup, attempt
        now = arena.mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[:n], transformed) and np.array_equal(now[n + 1 : 2 * n + 1], y)
        assert (now[n] == rc.GUARD).all() and (now[2 * n + 1 :] == rc.GUARD).all()
        results.append((dot.tobytes(), sup.tobytes()))
    assert not stats[:4].any(), stats
    assert results[0] == results[1] == results[2]


def test_a_repeated_host_call_grows_no_workspace():
    a, b = rc.mixed(1000, 1), rc.mixed(1000, 3)
    L = _lib.lib()
    reduce_on(rc.DOT, a, b, 0), support_on(a, 0)
    L.snarkvm_hip_alloc_stats(None, 1)
    got, sup = reduce_on(rc.DOT, a, b, 0), support_on(a, 0)
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert np.array_equal(got, rc.expected(rc.DOT, a, b)) and sup == rc.expected_support(a)


# ---- Evaluations::evaluate (fft/evaluations.rs:85-92) --------------------------------------------------------------------------
@pytest.mark.parametrize("lg", [3, 8, 12])
def test_evaluations_evaluate(lg):
    """equals the value of the interpolated polynomial at tau (the oracle's inverse transform and Horner evaluation), for a random tau and for
    tau a domain element (the one-hot branch of the Lagrange coefficients)"""
    n = 1 << lg
    evals = rc.rnd(n, 4)
    interpolated = oracle.ntt(evals, direction=oracle.INVERSE)
    one = util.ints_to_fr_mont([1])
    elems = oracle.distribute_powers(np.tile(one, (n, 1)), oracle.domain(lg)[0:1], one)
    domain = fft.EvaluationDomain.new(n)
    ev = fft.Evaluations.from_vec_and_domain(evals, domain)
    d_evals = HipMem.from_numpy(evals)
    d_coeffs = HipMem(32 * n)
    for tau in (rc.rnd(1, 9), elems[n // 3 : n // 3 + 1], elems[0:1]):
        want = oracle.poly_evaluate(interpolated, tau)
        assert np.array_equal(ev.evaluate(tau), want)
        assert np.array_equal(fft.Evaluations.evaluate_device(domain, d_evals, tau, d_coeffs), want)
        lag = oracle.lagrange_coefficients(lg, tau)
        assert np.array_equal(d_coeffs.download(dtype=np.uint64).reshape(-1, 4), lag)  # the coefficient vector stays in HBM
        assert np.array_equal(ev.evaluate_with_coeffs(lag), want)
        assert np.array_equal(fft.Evaluations.evaluate_with_coeffs_device(d_evals, d_coeffs, n), want)
    assert np.array_equal(ev.evaluate(elems[5:6]), evals[5:6])  # at a domain element: the evaluation itself


# ---- KZG10::commit on a device-resident buffer (kzg10/mod.rs:98-156) -----------------------------------------------------------
@pytest.fixture(scope="module")
def powers(golden):
    bases = _srs(golden, 1024)
    gamma = oracle.g1_gen_bases(util.g1_generator_affine(), 7, 8)
    pw = kzg10.Powers(bases, gamma)
    yield pw, bases
    pw.close()


def _buffer(size, first, last):
    """`size` elements, non-zero exactly on [first, last] (random there, ends forced non-zero)"""
    v = np.zeros((size, 4), dtype=np.uint64)
    v[first : last + 1] = rc.rnd(last + 1 - first, 6)
    return v


def _commitment_of(bases, coeffs):
    t = poly.trim(coeffs)
    return oracle.g1_to_affine(oracle.g1_msm(bases[: len(t)], oracle.fr_op("to_bigint", t)))


def test_commit_resident_trims_and_skips_leading_zeros(powers):
    pw, bases = powers
    v = _buffer(512, 7, 200)  # degree 200, 7 leading zero coefficients
    mem = HipMem.from_numpy(v)
    comm, rand = kzg10.KZG10.commit_resident(pw, mem, 512)
    assert util.affine_equal(oracle.g1_to_affine(comm), _commitment_of(bases, v)) and not rand.is_hiding()
    comm, _ = kzg10.KZG10.commit_resident(pw, mem.ptr, 512, degree_bound=200)  # a raw pointer; the bound is met exactly
    assert util.affine_equal(oracle.g1_to_affine(comm), _commitment_of(bases, v))
    with pytest.raises(kzg10.PCError, match="IncorrectDegreeBound"):
        kzg10.KZG10.commit_resident(pw, mem, 512, degree_bound=199)
    assert np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), v)


def test_commit_resident_zero_buffer_is_the_identity(powers):
    pw, _ = powers
    zeros = np.zeros((512, 4), dtype=np.uint64)
    mem = HipMem.from_numpy(zeros)
    comm, _ = kzg10.KZG10.commit_resident(pw, mem, 512)
    want, _ = kzg10.KZG10.commit(pw, poly.trim(zeros))
    assert np.array_equal(comm.view(np.uint8), want.view(np.uint8))
    assert oracle.g1_to_affine(comm)["infinity"][0]


def test_commit_resident_accepts_a_buffer_longer_than_the_powers(powers):
    import torch

    pw, bases = powers
    v = _buffer(2048, 0, 1000)  # degree 1000 in a 2048-element buffer: what a full-domain product leaves
    mem = HipMem.from_numpy(v)
    comm, _ = kzg10.KZG10.commit_resident(pw, mem, 2048)
    assert util.affine_equal(oracle.g1_to_affine(comm), _commitment_of(bases, v))
    with pytest.raises(kzg10.PCError, match="TooManyCoefficients"):  # commit_device goes by the buffer length
        kzg10.KZG10.commit_device(pw, torch.from_numpy(v.view(np.int64)).to("cuda:0"))
    over = HipMem.from_numpy(_buffer(2048, 3, 1024))  # degree 1024: 1025 coefficients > 1024 powers
    with pytest.raises(kzg10.PCError, match="TooManyCoefficients"):
        kzg10.KZG10.commit_resident(pw, over, 2048)
    edge = _buffer(2048, 0, 1023)  # degree 1023: exactly the powers
    comm, _ = kzg10.KZG10.commit_resident(pw, HipMem.from_numpy(edge), 2048)
    assert util.affine_equal(oracle.g1_to_affine(comm), _commitment_of(bases, edge))


def test_commit_resident_hiding_equals_commit(powers):
    pw, _ = powers
    blind = rc.rnd(4, 8)
    for v in (_buffer(512, 7, 200), np.zeros((64, 4), dtype=np.uint64)):
        mem = HipMem.from_numpy(v)
        got, r1 = kzg10.KZG10.commit_resident(pw, mem, len(v), 2, lambda k: blind[:k])
        want, r2 = kzg10.KZG10.commit(pw, poly.trim(v), 2, lambda k: blind[:k])
        assert util.affine_equal(oracle.g1_to_affine(got), oracle.g1_to_affine(want))
        assert np.array_equal(r1.blinding_polynomial, r2.blinding_polynomial) and r1.is_hiding()
    with pytest.raises(kzg10.PCError, match="MissingRng"):
        kzg10.KZG10.commit_resident(pw, mem, 64, 2)
