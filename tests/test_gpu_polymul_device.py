"""snarkvm_hip_polymul_device: `snarkvm_polymul` over operands that live in device memory (include/snarkvm_hip.h).

Every comparison is integer and bit-exact against the CPU restatement (oracle.polymul).  The domains are the smallest that reach
every branch of the transform plan (ntt.hip.h::ntt_make_plan: one pass up to 2^8, two up to 2^16, three up to 2^27) and both
addressing branches of the bounded load; the operand lengths sit on and around the first pass' inner stride, where a row of the
first stage group changes from "read" to "zero".
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, plugin, synthetic
from snarkvm_amd.devmem import HipMem

pytestmark = pytest.mark.gpu

INVALID_VALUE, MEMORY_ALLOCATION = 1, 2  # hipErrorInvalidValue, hipErrorMemoryAllocation
GUARD = 64  # elements behind every short operand that no call may touch

_pool = {}


def fr(n, seed):
    """n Fr elements in memory (Montgomery) form, a slice of one pool per seed"""
    size = 1 << 20
    if seed not in _pool:
        _pool[seed] = oracle.fr_op("from_bigint", synthetic.random_fr_integers(size, 0xD0 + seed))
    assert n <= size
    return _pool[seed][:n]


def upload(a, guard=0):
    """`a` followed by `guard` elements of a fixed non-zero pattern"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    if guard:
        a = np.concatenate([a, np.full((guard, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)])
    return HipMem.from_numpy(a) if len(a) else HipMem(32)


def fetch(mem, n, offset=0):
    return mem.download(32 * n, 32 * offset, dtype=np.uint64).reshape(-1, 4)


def device_product(lg, polys, evals=(), prefill=None):
    """upload, multiply into a fresh output vector (pre-filled with `prefill` when given), download"""
    n = 1 << lg
    dp = [upload(p) for p in polys]
    de = [upload(e) for e in evals]
    out = HipMem.from_numpy(np.full((n, 4), 7 if prefill is None else prefill, dtype=np.uint64))
    plugin.polymul_device(lg, out.ptr, [(m.ptr, len(p)) for m, p in zip(dp, polys)], [m.ptr for m in de])
    return fetch(out, n)


@pytest.mark.parametrize("lg", list(range(11)) + [16, 17, 18])
def test_every_small_domain(lg):
    """two coefficient operands of n/2 + n/2 and of 1 + n elements: single-stage-first and radix-4 stage groups, narrow and wide tiles,
    the single-pass addressing branch (lg <= 8)"""
    n = 1 << lg
    shapes = [(n // 2, n // 2)] + ([(1, n)] if n >= 2 else [(1, 1)])
    for la, lb in shapes:
        a, b = fr(la, 1), fr(lb, 2)
        assert np.array_equal(device_product(lg, [a, b]), oracle.polymul(lg, [a, b])), (lg, la, lb)


@pytest.mark.parametrize("lg,stride", [(10, 32), (17, 4096)])
def test_length_edges(lg, stride):
    """operand A ends on, just before and just behind a row of the first pass (inner stride 2^s), at both ends of the domain; B has 7
    elements, so the longer products wrap around X^n - 1"""
    n = 1 << lg
    radices = (ctypes.c_int32 * 4)()
    assert _lib.lib().snarkvm_hip_selftest_ntt_plan(lg, radices) >= 2 and 1 << (lg - radices[0]) == stride  # the plan this test was sized for
    b = fr(7, 2)
    for la in (0, 1, stride - 1, stride, stride + 1, n // 2, n // 2 + 1, n - 3, n):
        a = fr(la, 1)
        assert np.array_equal(device_product(lg, [a, b]), oracle.polymul(lg, [a, b])), (lg, la)


@pytest.mark.parametrize("npoly,neval", [(2, 0), (3, 0), (8, 0), (0, 1), (0, 2), (0, 4), (8, 4)])
def test_operand_mixes(npoly, neval):
    lg = 12
    n = 1 << lg
    polys = [fr(n // 2 + 11 * k, 1)[k:] for k in range(npoly)]
    evals = [fr(n + k, 3)[k:] for k in range(neval)]
    assert np.array_equal(device_product(lg, polys, evals), oracle.polymul(lg, polys, evals))


def test_one_polynomial_is_copied_and_the_tail_zeroed():
    lg = 12
    a = fr(1000, 1)
    got = device_product(lg, [a], prefill=0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(got[:1000], a) and not got[1000:].any()
    assert np.array_equal(got, oracle.polymul(lg, [a]))


def test_fifty_operands():
    """more factors than any pointer table of the kernels holds, and more transforms than one batched launch takes"""
    lg = 10
    polys = [fr(20 + k, 1)[k:] for k in range(50)]
    assert np.array_equal(device_product(lg, polys), oracle.polymul(lg, polys))


@pytest.mark.parametrize("lg", [9, 17])
def test_operands_stay_intact(lg):
    n = 1 << lg
    a, b, e = fr(n // 2, 1), fr(n // 2 + 1, 2), fr(n, 3)
    da, db, de = upload(a, GUARD), upload(b, GUARD), upload(e, GUARD)
    before = [m.download().copy() for m in (da, db, de)]
    out = HipMem(32 * n)
    plugin.polymul_device(lg, out.ptr, [(da.ptr, len(a)), (db.ptr, len(b))], [de.ptr])
    assert np.array_equal(fetch(out, n), oracle.polymul(lg, [a, b], [e]))
    for m, w in zip((da, db, de), before):
        assert np.array_equal(m.download(), w)


@pytest.mark.parametrize("lg", [9, 17])
def test_output_may_be_an_operand(lg):
    n = 1 << lg
    a, b, e = fr(n // 2, 1), fr(n // 2, 2), fr(n, 3)
    # v <- v * b with v a polynomial of n / 2 coefficients inside an n-element buffer whose tail is not zero
    v = upload(np.concatenate([a, fr(n // 2, 4)]))
    db = upload(b)
    plugin.polymul_device(lg, v.ptr, [(v.ptr, n // 2), (db.ptr, n // 2)])
    assert np.array_equal(fetch(v, n), oracle.polymul(lg, [a, b]))
    # the output is the second evaluation vector
    e2 = fr(n + 5, 4)[5:]
    de, de2, da = upload(e), upload(e2), upload(a)
    plugin.polymul_device(lg, de2.ptr, [(da.ptr, n // 2)], [de.ptr, de2.ptr])
    assert np.array_equal(fetch(de2, n), oracle.polymul(lg, [a], [e, e2]))
    assert np.array_equal(fetch(de, n), e) and np.array_equal(fetch(da, n // 2), a)


def test_partial_overlap_is_refused():
    lg = 9
    n = 1 << lg
    buf = upload(fr(n + 1, 1))
    db = upload(fr(n // 2, 2))
    before = buf.download().copy()
    with pytest.raises(_lib.HipError) as e:
        plugin.polymul_device(lg, buf.ptr + 32, [(buf.ptr, n // 2), (db.ptr, n // 2)])
    assert e.value.code == INVALID_VALUE and e.value.message
    assert np.array_equal(buf.download(), before) and np.array_equal(fetch(db, n // 2), fr(n // 2, 2))


def test_errors_leave_the_output_alone():
    lg = 9
    n = 1 << lg
    da, de = upload(fr(n + 1, 1)), upload(fr(n, 3))
    out = HipMem.from_numpy(np.full((n, 4), 7, dtype=np.uint64))
    L = _lib.lib()

    def call(lg_, polys, evals):
        pp = (ctypes.c_void_p * max(1, len(polys)))(*[p for p, _ in polys])
        pl = (ctypes.c_size_t * max(1, len(polys)))(*[k for _, k in polys])
        ep = (ctypes.c_void_p * max(1, len(evals)))(*[p for p, _ in evals])
        el = (ctypes.c_size_t * max(1, len(evals)))(*[k for _, k in evals])
        with pytest.raises(_lib.HipError) as e:
            _lib.check(L.snarkvm_hip_polymul_device(out.ptr, len(polys), pp, pl, len(evals), ep, el, lg_))
        assert e.value.message
        assert (fetch(out, n) == 7).all()
        return e.value.code

    assert call(29, [(da.ptr, 4), (da.ptr, 4)], []) == MEMORY_ALLOCATION
    assert call(lg, [(da.ptr, 4), (da.ptr, n + 1)], []) == INVALID_VALUE
    assert call(lg, [(da.ptr, 4)], [(de.ptr, n - 1)]) == INVALID_VALUE
    assert call(lg, [(da.ptr, 4), (None, 4)], []) == INVALID_VALUE
    assert call(lg, [(da.ptr, 4)], [(None, n)]) == INVALID_VALUE


def _three_products(lg, bufs):
    """o1 = a * b; o2 = o1 * c (reads the first product); o3 = a * evaluations e"""
    n = 1 << lg
    a, b, c, e, o1, o2, o3 = bufs
    plugin.polymul_device(lg, o1.ptr, [(a.ptr, n // 4), (b.ptr, n // 4)])
    plugin.polymul_device(lg, o2.ptr, [(o1.ptr, n), (c.ptr, n // 4)])
    plugin.polymul_device(lg, o3.ptr, [(a.ptr, n // 4)], [e.ptr])


def _three_products_data(lg):
    n = 1 << lg
    a, b, c, e = fr(n // 4, 1), fr(n // 4, 2), fr(n // 4, 3), fr(n, 4)
    o1 = oracle.polymul(lg, [a, b])
    return (a, b, c, e), (o1, oracle.polymul(lg, [o1, c]), oracle.polymul(lg, [a], [e]))


def _three_products_buffers(lg, operands):
    return [upload(x) for x in operands] + [HipMem(32 << lg) for _ in range(3)]


def test_inside_a_scope():
    lg = 14
    operands, want = _three_products_data(lg)
    bufs = _three_products_buffers(lg, operands)
    L = _lib.lib()
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(bufs[0].ptr)))
    try:
        _three_products(lg, bufs)
    finally:
        _lib.check(L.snarkvm_hip_scope_end())
    for m, w in zip(bufs[4:], want):
        assert np.array_equal(fetch(m, 1 << lg), w)


def test_four_threads_with_a_scope_each():
    lg = 14
    operands, want = _three_products_data(lg)
    sets = [_three_products_buffers(lg, operands) for _ in range(4)]
    L = _lib.lib()
    errors = []
    barrier = threading.Barrier(4)

    def worker(bufs):
        try:
            barrier.wait()
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(bufs[0].ptr)))
            try:
                _three_products(lg, bufs)
            finally:
                _lib.check(L.snarkvm_hip_scope_end())
        except Exception as ex:  # reported by the main thread
            errors.append(repr(ex))

    threads = [threading.Thread(target=worker, args=(s,)) for s in sets]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for bufs in sets:
        for m, w in zip(bufs[4:], want):
            assert np.array_equal(fetch(m, 1 << lg), w)


def test_a_repeated_call_grows_no_workspace():
    lg = 18
    n = 1 << lg
    da, db, out = upload(fr(n // 2, 1)), upload(fr(n // 2, 2)), HipMem(32 * n)
    L = _lib.lib()
    plugin.polymul_device(lg, out.ptr, [(da.ptr, n // 2), (db.ptr, n // 2)])
    L.snarkvm_hip_alloc_stats(None, 1)
    plugin.polymul_device(lg, out.ptr, [(da.ptr, n // 2), (db.ptr, n // 2)])
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats


@pytest.mark.parametrize("lg,lens", [(18, (1 << 16, 1 << 17, (1 << 16) + 1)), (20, (1 << 19, 1 << 19))])
def test_proof_sized_and_larger(lg, lens):
    polys = [fr(k, 1 + i) for i, k in enumerate(lens)]
    got = device_product(lg, polys)
    assert np.array_equal(got, oracle.polymul(lg, polys))
    assert np.array_equal(got, plugin.polymul(1 << lg, polys, []))
