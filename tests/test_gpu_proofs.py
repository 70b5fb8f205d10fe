"""Round-4 paths of the prover-shaped workload, all through the C ABI, all against the CPU oracle:

* the in-library coalescer (csrc/msm_batch.hip.h::msm_coalesced): concurrent callers of proof-sized registered MSMs - the
  reference's rayon fan-out, one `snarkvm_msm`-sized call per polynomial (sonic_pc/mod.rs:186-245) - are fused into groups;
  every caller still gets ITS result, bit-identical to the per-instance path;
* the deferred-synchronisation scope (snarkvm_hip_scope_begin / _end) and the batched NTT launches (one launch per pass for up to
  48 vectors);
* the lock-step replay of several proofs (snarkvm_amd/proofs.py::replay_lockstep, `VarunaSNARK::prove_batch`'s shape,
  varuna.rs:336): all 15 results of every proof against oracle/proof_replay.py, and against the per-proof replay.
"""
import ctypes
import threading

import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import proof_replay
from snarkvm_amd import _lib, kzg10, msm, proofs, synthetic
from snarkvm_amd.layout import G1_PROJECTIVE, G2_PROJECTIVE
from tests import util

pytestmark = pytest.mark.gpu


def _closed(G, s, start=1):
    return oracle.g1_to_affine(oracle.g1_mul(G, util.limbs(util.weighted_sum_mod_r(s, start=start), 4)))


@pytest.mark.parametrize("threads,calls", [(12, 6), (3, 10)])
def test_concurrent_callers_are_coalesced_bit_exactly(threads, calls):
    """`threads` host threads issue `calls` single-instance MSMs each over one registered vector at the same time (sizes around
    the fused-instance limits, host and device scalars in different threads): every result equals the closed form
    sum_i s_i (off + i + 1) G evaluated by the oracle."""
    import torch

    G = util.g1_generator_affine()
    n = 1 << 16
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    sizes = [1, 2, 77, 4096, 8191, 8192, 8193, 30000, 50000, 65536]
    pool = synthetic.random_fr_integers(n, 9090)
    d_pool = torch.from_numpy(pool.view(np.int64)).cuda()
    torch.cuda.synchronize()
    errors, done = [], []
    barrier = threading.Barrier(threads)

    def worker(t):
        try:
            barrier.wait()
            for k in range(calls):
                m = sizes[(3 * t + 5 * k) % len(sizes)]
                off = (17 * t + k) % (n - m + 1)
                lo = (t * 131 + k * 7) % (n - m + 1)
                if t % 2:
                    got = rb.msm(pool[lo : lo + m], offset=off)
                else:
                    got = rb.msm(device_ptr=d_pool.data_ptr() + 32 * lo, npoints=m, offset=off)
                if not util.affine_equal(oracle.g1_to_affine(got), _closed(G, pool[lo : lo + m], start=off + 1)):
                    errors.append((t, k, m, off))
            done.append(t)
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(threads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    rb.close()
    assert not errors, errors[:5]
    assert len(done) == threads


def test_batch_of_many_instances_fused_groups_and_parallel_finish():
    """One batch call with 150 proof-sized instances (more than one fused group, host finishes on several threads): each result
    against its closed form; an instance of zero pairs returns the point at infinity."""
    G = util.g1_generator_affine()
    n = 1 << 15
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=16, window_bits=16)
    pool = synthetic.random_fr_integers(n + 4096, 4711)
    sizes = [(1 + 37 * k * k) % n + 1 for k in range(149)] + [0]
    offs = [(k * 101) % (n - s + 1) for k, s in enumerate(sizes)]
    scal = [pool[k : k + s] for k, s in enumerate(sizes)]
    res = rb.msm_batch(scal, offsets=offs)
    for k, (s, o) in enumerate(zip(sizes, offs)):
        got = oracle.g1_to_affine(res[k : k + 1])
        if s == 0:
            assert int(got["infinity"][0]) == 1
        else:
            assert util.affine_equal(got, _closed(G, scal[k], start=o + 1)), k
    rb.close()


@pytest.mark.parametrize("lg", [9, 10, 13, 16, 17, 18])
def test_ntt_batched_launches_vs_oracle(lg):
    """snarkvm_hip_ntt_device_batch with runs of distinct vectors (one launch per pass per run), mixed directions / types, more
    than 48 vectors, and a vector listed twice in a row: every element of every result against oracle.ntt."""
    import torch

    L = _lib.lib()
    nv = 53 if lg <= 13 else 7
    n = 1 << lg
    xs = [oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 600 + 10 * lg + i)) for i in range(nv)]
    dev = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in xs]
    torch.cuda.synchronize()
    order = list(range(nv)) + [2, 2, 0]                  # vectors 2 and 0 are transformed again (2 twice in a row)
    dirs = [0] * (nv - 3) + [1, 1, 1] + [1, 1, 1]        # a forward run, then inverse ones
    kinds = [0] * (nv - 1) + [1] + [0, 0, 1]
    ptrs = (ctypes.c_void_p * len(order))(*[dev[i].data_ptr() for i in order])
    _lib.check(L.snarkvm_hip_ntt_device_batch(ptrs, ctypes.c_size_t(len(order)), ctypes.c_uint32(lg), 0, (ctypes.c_int * len(order))(*dirs),
                                              (ctypes.c_int * len(order))(*kinds)))
    want = [x.copy() for x in xs]
    for i, d, k in zip(order, dirs, kinds):
        want[i] = oracle.ntt(want[i], oracle.ORDER_NN, d, k)
    for i in range(nv):
        assert np.array_equal(dev[i].cpu().numpy().view(np.uint64).reshape(-1, 4), want[i]), (lg, i)


def test_scope_defers_synchronisation_not_results():
    """A chain of device-resident calls inside snarkvm_hip_scope_begin / _end (transforms, a pointwise product, a subtraction, the
    division by the vanishing polynomial, p / (X - z) with its host remainder) gives the oracle's values; an MSM issued inside the
    scope sees the scope's results; a second scope_begin on the same thread is refused."""
    import torch

    L = _lib.lib()
    lg = 12
    n = 1 << lg
    a0 = oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 1))
    b0 = oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 2))
    z = oracle.fr_op("from_bigint", synthetic.random_fr_integers(1, 3))
    da = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    db = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    dq = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    dr = torch.zeros(8 * n, dtype=torch.int64, device="cuda")
    da[: 4 * n] = torch.from_numpy(a0.view(np.int64).reshape(-1)).cuda()
    db[: 4 * n] = torch.from_numpy(b0.view(np.int64).reshape(-1)).cuda()
    torch.cuda.synchronize()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rem = np.zeros((1, 4), dtype=np.uint64)
    G = util.g1_generator_affine()
    bases = oracle.g1_gen_bases(G, 1, 2 * n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    _lib.check(L.snarkvm_hip_scope_begin(P(da)))
    err = L.snarkvm_hip_scope_begin(P(da))
    assert err.code != 0
    _lib._libc.free(err.message)
    ptrs = (ctypes.c_void_p * 2)(da.data_ptr(), db.data_ptr())
    _lib.check(L.snarkvm_hip_ntt_device_batch(ptrs, ctypes.c_size_t(2), ctypes.c_uint32(lg + 1), 0, None, None))
    _lib.check(L.snarkvm_hip_fr_mul_device(P(da), P(da), P(db), ctypes.c_size_t(2 * n)))
    _lib.check(L.snarkvm_hip_ntt_device(P(da), ctypes.c_uint32(lg + 1), 0, 1, 0))
    _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(P(dq), P(dr), P(da), ctypes.c_size_t(2 * n), ctypes.c_size_t(n), 1))
    _lib.check(L.snarkvm_hip_fr_divide_by_linear(P(db), ctypes.c_void_p(rem.ctypes.data), P(da), ctypes.c_size_t(2 * n), ctypes.c_void_p(z.ctypes.data), 1))
    got_msm = rb.msm_batch(device_ptrs=[dq.data_ptr()], npoints=[n], montgomery=True)  # leaves the scope's lane: waits for the scope's queued work first
    _lib.check(L.snarkvm_hip_scope_end())
    prod = oracle.polymul(lg + 1, [a0, b0])
    one = oracle.fr_op("from_bigint", np.array([[1, 0, 0, 0]], dtype=np.uint64))
    wq, wr = oracle.poly_divide(prod, [(0, oracle.fr_op("neg", one)[0]), (n, one[0])])
    host = lambda t, k: t[: 4 * k].cpu().numpy().view(np.uint64).reshape(-1, 4)  # noqa: E731
    assert np.array_equal(host(da, 2 * n), prod)
    assert np.array_equal(host(dq, wq.shape[0]), wq) and np.array_equal(host(dr, wr.shape[0]), wr)
    lq, _ = oracle.poly_divide(prod, [(0, oracle.fr_op("neg", z)[0]), (1, one[0])])
    assert np.array_equal(host(db, lq.shape[0]), lq)
    assert np.array_equal(rem, oracle.poly_evaluate(prod, z))
    want = oracle.g1_msm(bases[:n], oracle.fr_op("to_bigint", _pad(wq, n)))
    assert util.affine_equal(oracle.g1_to_affine(got_msm), oracle.g1_to_affine(want))
    rb.close()


def _pad(v, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    out[: v.shape[0]] = v
    return out


def _check_against_oracle(keys, shape, salt, got):
    want = proof_replay.expected_results(keys.pool_host, keys.g1_host, keys.g2_host, keys.point, shape.lg_r, shape.lg_k, shape.lg_g2, shape.nmax, salt)
    assert len(got) == 15
    for j in range(14):
        ga = kzg10.to_affine(np.frombuffer(got[j], dtype=G1_PROJECTIVE))
        assert util.affine_equal(ga, want[j]), (salt, j)
    assert oracle.g2_to_affine(np.frombuffer(got[14], dtype=G2_PROJECTIVE)).tobytes() == want[14].tobytes(), (salt, "g2")


def test_lockstep_replay_every_result_vs_oracle():
    """Three proofs of a reduced shape (|R| = 2^12, |K| = 2^13, G2 2^10) replayed in lock step - arithmetic and arbitrary salts -
    and one by one: all 14 commitments and the G2 result of every proof against the oracle's restatement of the data flow; the
    two replays agree."""
    shape = proofs.ProofShape(lg_r=12, lg_k=13, lg_g2=10)
    keys = proofs.ProverKeys(shape, seed=5)
    ws = proofs.LockstepWorkspace(keys, 3)
    for salts in ([0, 1, 2], [7, 0, 3]):
        got = proofs.replay_lockstep(ws, salts, collect=True)
        for s, g in zip(salts, got):
            _check_against_oracle(keys, shape, s, g)
    single = proofs.ProofBatch(keys, workers=1)
    _, one_by_one = single.run([7, 0, 3], collect=True)
    lock = proofs.replay_lockstep(ws, [7, 0, 3], collect=True)
    for a, b in zip(one_by_one, lock):
        assert proofs.normalize_results(a) == proofs.normalize_results(b)
    keys.close()


def test_concurrent_replays_meet_in_the_coalescer_vs_oracle():
    """Six caller threads replay eight proofs of the reduced shape concurrently (their commit rounds are fused by the coalescer):
    every result of two of them against the oracle, all of them against a serial replay."""
    shape = proofs.ProofShape(lg_r=12, lg_k=13, lg_g2=10)
    keys = proofs.ProverKeys(shape, seed=6)
    salts = list(range(8))
    batch = proofs.ProofBatch(keys, workers=6)
    _, got = batch.run(salts, collect=True)
    for s in (0, 7):
        _check_against_oracle(keys, shape, s, got[s])
    _, serial = proofs.ProofBatch(keys, workers=1).run(salts, collect=True)
    for a, b in zip(got, serial):
        assert proofs.normalize_results(a) == proofs.normalize_results(b)
    keys.close()


# ---- round 5: one proof at a time in one scope, asynchronous commitments, scopes under thread pressure, workspace growth --------

def test_single_proof_scope_replay_every_result_vs_oracle():
    """configs[3]: `replay_single` (one SNARKVM_HIP_SCOPE_ASYNC_MSM scope per proof, the round's independent transforms as batches, the
    commitments only enqueued and finished by scope_end, the G2 MSM underneath) for three proofs of the reduced shape: all 15
    results of each against the oracle; the same with synchronous commitments; both equal the serial replay."""
    shape = proofs.ProofShape(lg_r=12, lg_k=13, lg_g2=10)
    keys = proofs.ProverKeys(shape, seed=8)
    ws = proofs.SingleProofWorkspace(keys)
    ref = proofs.ProofWorkspace(keys)
    for salt in (0, 5, 2):
        got_async, got_sync, got_await, got_in_stream, serial = [], [], [], [], []
        proofs.replay_single(ws, salt, got_async, async_msm=True)
        proofs.replay_single(ws, salt, got_sync, async_msm=False)
        proofs.replay_single(ws, salt, got_await, async_msm=True, await_rounds=True)  # snarkvm_hip_scope_collect after every commitment round
        # ... and with those awaited rounds on the scope's own stream (snarkvm_hip_scope_set_flags: SNARKVM_HIP_SCOPE_MSM_IN_STREAM after the G2 MSM)
        proofs.replay_single(ws, salt, got_in_stream, async_msm=True, await_rounds=True, msm_in_stream=True)
        proofs.replay(ref, salt, serial)
        _check_against_oracle(keys, shape, salt, got_async)
        assert proofs.normalize_results(got_async) == proofs.normalize_results(got_sync) == proofs.normalize_results(got_await) == proofs.normalize_results(serial)
        assert proofs.normalize_results(got_in_stream) == proofs.normalize_results(serial)
    keys.close()


def test_async_msm_scope_outputs_arrive_at_scope_end_and_inputs_may_be_reused():
    """Inside an SNARKVM_HIP_SCOPE_ASYNC_MSM scope: five commitments of one scalar buffer that is overwritten (on the scope's stream)
    between the calls - each MSM must see the contents of ITS moment; single, batch and two-range (`_ex`) entry points, and one host-scalar call in the middle (synchronous: flushes what is pending).  Outputs are
    written by scope_end."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    n = 1 << 13
    bases = oracle.g1_gen_bases(G, 1, 2 * n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    src = [synthetic.random_fr_integers(n, 7000 + i) for i in range(5)]
    d_src = [torch.from_numpy(x.view(np.int64).reshape(-1).copy()).cuda() for x in src]
    buf = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    outs = np.zeros(5, dtype=G1_PROJECTIVE)
    host_out = np.zeros(1, dtype=G1_PROJECTIVE)
    sizes = [n, 4097, n - 3, 1, 2500]
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(buf.data_ptr()), 1))
    assert L.snarkvm_hip_scope_stream()
    stream = torch.cuda.ExternalStream(L.snarkvm_hip_scope_stream())
    for i in range(5):
        with torch.cuda.stream(stream):
            buf.copy_(d_src[i])
        o = ctypes.c_void_p(outs[i : i + 1].ctypes.data)
        if i % 3 == 0:
            _lib.check(L.snarkvm_hip_msm_registered(o, rb._h, 3, sizes[i], ctypes.c_void_p(buf.data_ptr()), 1, 0))
        elif i % 3 == 1:
            _lib.check(L.snarkvm_hip_msm_registered_ex(o, rb._h, 3, sizes[i] - 2, n, 2, ctypes.c_void_p(buf.data_ptr()), 1, 0, 0))
        else:
            ptrs = (ctypes.c_void_p * 1)(buf.data_ptr())
            _lib.check(L.snarkvm_hip_msm_registered_batch(o, rb._h, 1, (ctypes.c_size_t * 1)(3), (ctypes.c_size_t * 1)(sizes[i]), ptrs, 1, 0, 0))
        if i == 2:  # a host-scalar call: takes the synchronous path, after the scope's pending work
            assert not outs[3:].view(np.uint8).any()
            _lib.check(L.snarkvm_hip_msm_registered(ctypes.c_void_p(host_out.ctypes.data), rb._h, 0, 100, ctypes.c_void_p(src[0].ctypes.data), 0, 0))
            assert outs[:3].view(np.uint8).any(axis=None)
    _lib.check(L.snarkvm_hip_scope_end())
    assert L.snarkvm_hip_scope_stream() is None
    for i in range(5):
        s = src[i][: sizes[i]]
        if i % 3 == 1:
            want = oracle.g1_add(oracle.g1_msm(bases[3 : 3 + sizes[i] - 2], s[: sizes[i] - 2]), oracle.g1_msm(bases[n : n + 2], s[sizes[i] - 2 :]))
        else:
            want = oracle.g1_msm(bases[3 : 3 + sizes[i]], s)
        assert util.affine_equal(oracle.g1_to_affine(outs[i : i + 1]), oracle.g1_to_affine(want)), i
    assert util.affine_equal(oracle.g1_to_affine(host_out), oracle.g1_to_affine(oracle.g1_msm(bases[:100], src[0][:100])))
    rb.close()


def test_a_thread_that_ends_inside_a_scope_gives_its_lanes_back():
    """Scopes hold lanes, a bounded resource (12 of a GPU's 16), and only the thread that began a scope can end it.  Twenty threads, one after the
    other, open an asynchronous scope, enqueue a transform and an MSM (which takes a second lane) and END WITHOUT scope_end: the thread-exit
    clean-up must return the lanes - otherwise the seventh thread would wait in scope_begin forever.  Afterwards a scope on the main thread
    works and delivers a correct result."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    lg = 10
    n = 1 << lg
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    x = synthetic.random_fr_integers(n, 8200)
    d = torch.from_numpy(x.view(np.int64).reshape(-1).copy()).cuda()
    scratch = d.clone()
    torch.cuda.synchronize()
    lost = np.zeros(20, dtype=G1_PROJECTIVE)  # outputs of the abandoned scopes: never written, must stay valid anyway
    errors = []

    def leaver(t):
        try:
            _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(d.data_ptr()), 1))
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(scratch.data_ptr()), ctypes.c_uint32(lg), 0, t & 1, 0))
            _lib.check(L.snarkvm_hip_msm_registered(ctypes.c_void_p(lost[t : t + 1].ctypes.data), rb._h, 0, n, ctypes.c_void_p(d.data_ptr()), 1, 0))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    for t in range(20):
        th = threading.Thread(target=leaver, args=(t,), daemon=True)
        th.start()
        th.join(timeout=60)
        assert not th.is_alive(), f"thread {t} is stuck in scope_begin: the lanes of the threads that ended inside their scopes were not returned"
    assert not errors, errors[:3]
    out = np.zeros(1, dtype=G1_PROJECTIVE)
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(d.data_ptr()), 1))
    _lib.check(L.snarkvm_hip_msm_registered(ctypes.c_void_p(out.ctypes.data), rb._h, 0, n, ctypes.c_void_p(d.data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_scope_end())
    assert util.affine_equal(oracle.g1_to_affine(out), oracle.g1_to_affine(oracle.g1_msm(bases, x)))
    rb.close()


def test_many_threads_inside_scopes_issue_msms_without_deadlock():
    """Round-4 review: scope_begin pins a lane; an MSM inside the scope needed another one; eight such threads held all eight lanes
    and waited for a ninth forever.  Twelve threads open scopes (plain and asynchronous ones alternating), run a transform and an
    MSM over its output, and end the scope, three times each - bounded by a timeout; every result against the oracle."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    lg, T = 10, 12
    n = 1 << lg
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    xs = [oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 8100 + t)) for t in range(T)]
    dev = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in xs]
    torch.cuda.synchronize()
    outs = np.zeros((T, 3), dtype=G1_PROJECTIVE)
    errors = []
    start = threading.Barrier(T)

    def worker(t):
        try:
            start.wait()
            for k in range(3):
                _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(dev[t].data_ptr()), t & 1))
                _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(dev[t].data_ptr()), ctypes.c_uint32(lg), 0, k & 1, 0))
                _lib.check(L.snarkvm_hip_msm_registered_ex(ctypes.c_void_p(outs[t, k : k + 1].ctypes.data), rb._h, 0, n, 0, 0, ctypes.c_void_p(dev[t].data_ptr()), 1, 1, 0))
                _lib.check(L.snarkvm_hip_scope_end())
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th), "threads inside scopes are stuck (lane pool exhausted)"
    assert not errors, errors[:3]
    for t in range(T):
        v = xs[t]
        for k in range(3):
            v = oracle.ntt(v, oracle.ORDER_NN, k & 1, 0)
            want = oracle.g1_msm(bases, oracle.fr_op("to_bigint", v))
            assert util.affine_equal(oracle.g1_to_affine(outs[t, k : k + 1]), oracle.g1_to_affine(want)), (t, k)
    rb.close()


def test_divide_by_linear_host_operands_inside_a_scope_return_the_remainder():
    """Round-4 advice: with on_device = 0 inside a scope the 32-byte remainder was parked until scope_end while the call itself had
    already waited - the caller read stale bytes.  The value must be there when the call returns."""
    import torch

    L = _lib.lib()
    n = 777
    p = oracle.fr_op("from_bigint", synthetic.random_fr_integers(n, 31))
    z = oracle.fr_op("from_bigint", synthetic.random_fr_integers(1, 32))
    q = np.zeros((n - 1, 4), dtype=np.uint64)
    rem = np.zeros((1, 4), dtype=np.uint64)
    anchor = torch.zeros(8, dtype=torch.int64, device="cuda")
    _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(anchor.data_ptr())))
    _lib.check(L.snarkvm_hip_fr_divide_by_linear(ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(rem.ctypes.data), ctypes.c_void_p(p.ctypes.data), ctypes.c_size_t(n),
                                                  ctypes.c_void_p(z.ctypes.data), 0))
    got_inside = rem.copy()
    _lib.check(L.snarkvm_hip_scope_end())
    one = oracle.fr_op("from_bigint", np.array([[1, 0, 0, 0]], dtype=np.uint64))
    wq, _ = oracle.poly_divide(p, [(0, oracle.fr_op("neg", z)[0]), (1, one[0])])
    assert np.array_equal(got_inside, oracle.poly_evaluate(p, z))
    assert np.array_equal(q[: wq.shape[0]], wq)


def test_second_batch_of_a_shape_allocates_nothing_and_is_not_slower():
    """The "tables1" cliff of round 4 (93.6 vs 37 ms per step on the driver's box): a 2-instance batch whose second lane had to grow its
    workspace behind the first lane's running MSM.  After ONE batch of a shape, every later batch of that shape must not allocate
    (snarkvm_hip_alloc_stats); and the later batches must not be slower than a WARM reference - batches 3-5 (best of three) against batch 2, which
    allocates nothing either (round 5 compared with batch 1, the one that allocates: that clause could never fail for the reason it exists);
    results identical."""
    import time

    import torch

    L = _lib.lib()
    if L.snarkvm_hip_num_devices() > 1:
        pytest.skip("several logical devices: device-resident instances are dealt round-robin over them, a later batch may meet a lane for the first time")
    G = util.g1_generator_affine()
    n = 1 << 20
    d_bases = torch.empty(n * 104, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.snarkvm_hip_g1_generate_bases_device(ctypes.c_void_p(d_bases.data_ptr()), ctypes.c_uint64(1), ctypes.c_size_t(n)))
    rb12 = msm.RegisteredBases(device_ptr=d_bases.data_ptr(), npoints=n, tables=13, window_bits=20)
    rb1 = msm.RegisteredBases(device_ptr=d_bases.data_ptr(), npoints=n, tables=1)
    sc = synthetic.random_fr_integers(n, 515)
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    rb12.msm_batch(device_ptrs=[d_sc.data_ptr()] * 3, npoints=[n] * 3)  # lanes sized for the windowed geometry
    rb1.msm(device_ptr=d_sc.data_ptr(), npoints=n)                      # one lane grows to the table-less geometry (round 4's warm-up)
    stats = (ctypes.c_uint64 * 5)()
    times, res = [], []
    for _ in range(5):
        _lib.check(L.snarkvm_hip_synchronize())
        L.snarkvm_hip_alloc_stats(stats, 1)
        t0 = time.perf_counter()
        res.append(rb1.msm_batch(device_ptrs=[d_sc.data_ptr()] * 2, npoints=[n] * 2))
        times.append(time.perf_counter() - t0)
        L.snarkvm_hip_alloc_stats(stats, 0)
        if len(times) > 1:
            assert stats[0] == 0 and stats[2] == 0, f"batch {len(times)} of the same shape allocated: {list(stats)}"
    # (a cliff is persistent: every later batch would be slow; the best of three keeps a single hiccup of the box out of the verdict)
    assert min(times[2:]) <= 1.3 * times[1], times
    want = _closed(G, sc)
    for r in res:
        for k in range(2):
            assert util.affine_equal(oracle.g1_to_affine(r[k : k + 1]), want)
    rb12.close()
    rb1.close()


def test_scope_collect_delivers_one_call_and_leaves_the_others_pending():
    """snarkvm_hip_scope_collect(out): inside an asynchronous scope two MSM calls are enqueued; collecting the SECOND one writes its output (the
    first one's may be written too if its results had already arrived while the call waited - it is owed by scope_end at the latest; a call
    that has not been issued yet is never touched); collect(NULL) then delivers the rest, the scope is still open (a further transform and MSM
    go through), scope_end delivers those.  Every result against the oracle."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    lg = 12
    n = 1 << lg
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    xs = [synthetic.random_fr_integers(n, 9300 + i) for i in range(3)]
    dev = [torch.from_numpy(x.view(np.int64).reshape(-1).copy()).cuda() for x in xs]
    torch.cuda.synchronize()
    outs = np.zeros(3, dtype=G1_PROJECTIVE)
    o = [ctypes.c_void_p(outs[i : i + 1].ctypes.data) for i in range(3)]
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(dev[0].data_ptr()), 3))
    _lib.check(L.snarkvm_hip_msm_registered(o[0], rb._h, 0, n, ctypes.c_void_p(dev[0].data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_msm_registered(o[1], rb._h, 0, n - 5, ctypes.c_void_p(dev[1].data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_scope_collect(o[1]))
    assert outs[1:2].view(np.uint8).any() and not outs[2:3].view(np.uint8).any()
    _lib.check(L.snarkvm_hip_scope_collect(None))
    assert outs[0:1].view(np.uint8).any()
    _lib.check(L.snarkvm_hip_msm_registered(o[2], rb._h, 7, n - 7, ctypes.c_void_p(dev[2].data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_scope_end())
    want = [oracle.g1_msm(bases, xs[0]), oracle.g1_msm(bases[: n - 5], xs[1][: n - 5]), oracle.g1_msm(bases[7:n], xs[2][: n - 7])]
    for i in range(3):
        assert util.affine_equal(oracle.g1_to_affine(outs[i : i + 1]), oracle.g1_to_affine(want[i])), i
    # a long scope that collects after every call: staging areas and events are handed out again each time (60 calls through 7 MSM lanes)
    many = np.zeros(60, dtype=G1_PROJECTIVE)
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(dev[0].data_ptr()), 3))
    for k in range(60):
        ok = ctypes.c_void_p(many[k : k + 1].ctypes.data)
        _lib.check(L.snarkvm_hip_msm_registered(ok, rb._h, k, n - 64, ctypes.c_void_p(dev[k % 3].data_ptr()), 1, 0))
        _lib.check(L.snarkvm_hip_scope_collect(ok if k % 2 else None))
        assert many[k : k + 1].view(np.uint8).any()
    _lib.check(L.snarkvm_hip_scope_end())
    for k in (0, 1, 2, 29, 59):
        assert util.affine_equal(oracle.g1_to_affine(many[k : k + 1]), oracle.g1_to_affine(oracle.g1_msm(bases[k : k + n - 64], xs[k % 3][: n - 64]))), k
    # snarkvm_hip_scope_set_flags: the first MSM goes to a further stream, the next ones onto the scope's own stream (SNARKVM_HIP_SCOPE_MSM_IN_STREAM),
    # behind a transform of their scalars that only the scope's stream orders; collecting the last in-stream MSM delivers it whatever the others' state
    assert L.snarkvm_hip_scope_set_flags(7).code != 0  # no open scope
    mixed = np.zeros(3, dtype=G1_PROJECTIVE)
    m = [ctypes.c_void_p(mixed[i : i + 1].ctypes.data) for i in range(3)]
    work = dev[1].clone()
    torch.cuda.synchronize()
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(dev[0].data_ptr()), 3))
    assert L.snarkvm_hip_scope_set_flags(16).code != 0  # unknown flag: the scope keeps its flags
    _lib.check(L.snarkvm_hip_msm_registered(m[0], rb._h, 0, n, ctypes.c_void_p(dev[0].data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_scope_set_flags(3 | 4))
    _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(work.data_ptr()), lg, 0, 0, 0))
    _lib.check(L.snarkvm_hip_msm_registered(m[1], rb._h, 0, n, ctypes.c_void_p(work.data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(work.data_ptr()), lg, 0, 1, 0))  # back to xs[1], behind the MSM on the same stream
    _lib.check(L.snarkvm_hip_msm_registered(m[2], rb._h, 0, n, ctypes.c_void_p(work.data_ptr()), 1, 0))
    _lib.check(L.snarkvm_hip_scope_collect(m[2]))
    assert mixed[2:3].view(np.uint8).any()
    _lib.check(L.snarkvm_hip_scope_end())
    want = [oracle.g1_msm(bases, xs[0]), oracle.g1_msm(bases, oracle.ntt(xs[1], oracle.ORDER_NN, oracle.FORWARD, oracle.STANDARD)), oracle.g1_msm(bases, xs[1])]
    for i in range(3):
        assert util.affine_equal(oracle.g1_to_affine(mixed[i : i + 1]), oracle.g1_to_affine(want[i])), i
    rb.close()


def test_a_bad_request_among_coalesced_callers_fails_alone():
    """Round-4 review: one failing ticket failed every caller of its coalesced batch.  Eight threads issue proof-sized MSMs at the same time; two of
    them pass a range that exceeds the registered bases (validated BEFORE the ticket is queued) and one a device pointer the library does not own:
    exactly those calls return an error, every other caller gets its own correct result."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    n = 1 << 13
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    pool = synthetic.random_fr_integers(n, 9400)
    d_pool = torch.from_numpy(pool.view(np.int64).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    T, rounds = 8, 6
    outs = np.zeros((T, rounds), dtype=G1_PROJECTIVE)
    codes = np.zeros((T, rounds), dtype=np.int64)
    start = threading.Barrier(T)

    def worker(t):
        start.wait()
        for k in range(rounds):
            o = ctypes.c_void_p(outs[t, k : k + 1].ctypes.data)
            if t in (2, 5):      # range exceeds the registered bases
                err = L.snarkvm_hip_msm_registered(o, rb._h, n - 100, 4096, ctypes.c_void_p(d_pool.data_ptr()), 1, 0)
            elif t == 7:         # "device" scalars that are host memory
                err = L.snarkvm_hip_msm_registered(o, rb._h, 0, 4096, ctypes.c_void_p(pool.ctypes.data), 1, 0)
            else:
                err = L.snarkvm_hip_msm_registered(o, rb._h, 0, 4096 + t, ctypes.c_void_p(d_pool.data_ptr() + 32 * k), 1, 0)
            codes[t, k] = err.code
            if err.message:
                _lib._libc.free(err.message)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for t in range(T):
        if t in (2, 5, 7):
            assert (codes[t] != 0).all(), (t, codes[t])
        else:
            assert (codes[t] == 0).all(), (t, codes[t])
            for k in range(rounds):
                want = oracle.g1_msm(bases[: 4096 + t], pool[k : k + 4096 + t])
                assert util.affine_equal(oracle.g1_to_affine(outs[t, k : k + 1]), oracle.g1_to_affine(want)), (t, k)
    rb.close()


# ---- round 6: the same proof through the reference's OWN three symbols on host buffers ---------------------------------------------

def test_ffi_only_replay_every_result_vs_oracle_stateless_and_cached():
    """`replay_ffi`: the proof's data flow with every hot-path step issued through snarkvm_ntt / snarkvm_polymul / snarkvm_msm on HOST buffers - what an
    unmodified snarkVM build gets - the commitments of a round from caller threads, every MSM over a slice of one long-lived base vector.  All 15 results
    of three proofs against the oracle, stateless and with the opt-in base cache switched on through its API form (snarkvm_hip_set_base_cache: the vector is
    registered at its second sighting, later calls are hits and meet in the coalescer); both equal the resident replay; the call counts are the reference's."""
    L = _lib.lib()
    shape = proofs.ProofShape(lg_r=12, lg_k=13, lg_g2=10)
    keys = proofs.ProverKeys(shape, seed=31)
    host = proofs.FfiProofHost(keys, threads=4)
    ref = proofs.ProofWorkspace(keys)
    try:
        for tables in (0, 16):
            _lib.check(L.snarkvm_hip_set_base_cache(tables))
            for salt in (0, 4, 1, 4):
                got, serial, t = [], [], {}
                proofs.replay_ffi(host, salt, got, t)
                proofs.replay(ref, salt, serial)
                _check_against_oracle(keys, shape, salt, got)
                assert proofs.normalize_results(got) == proofs.normalize_results(serial), (tables, salt)
                assert (t["ntt_calls"], t["polymul_calls"], t["msm_calls"]) == (20, 5, 14)
                assert t["ntt"] > 0 and t["msm"] > 0 and t["polymul"] > 0
        with pytest.raises(_lib.HipError):
            _lib.check(L.snarkvm_hip_set_base_cache(3))
    finally:
        _lib.check(L.snarkvm_hip_set_base_cache(0))
        host.close()
        keys.close()


def test_sync_msm_on_a_borrowed_scope_lane_does_not_clobber_pending_planes():
    """Round-5 advisor: inside an ASYNC_MSM scope with MSM_IN_STREAM the enqueued MSMs keep their bit planes in the scope lane's pinned area from offset 0 until the
    flush has read them.  A later MSM that does NOT qualify for enqueueing (here: profiling switched on in the middle of the scope) takes the synchronous path on the
    SAME (borrowed) lane and stages at offset 0 too - it must first deliver what is pending.  Every result against the oracle."""
    import torch

    L = _lib.lib()
    G = util.g1_generator_affine()
    n = 1 << 14
    bases = oracle.g1_gen_bases(G, 1, n)
    rb = msm.RegisteredBases(bases, tables=17, window_bits=15)
    sc = [synthetic.random_fr_integers(n, 8100 + i) for i in range(3)]
    d_sc = [torch.from_numpy(x.view(np.int64).reshape(-1).copy()).cuda() for x in sc]
    torch.cuda.synchronize()
    outs = np.zeros(3, dtype=G1_PROJECTIVE)
    _lib.check(L.snarkvm_hip_scope_begin_ex(ctypes.c_void_p(d_sc[0].data_ptr()), 1 | 2 | 4))
    try:
        for i in range(2):  # enqueued on the scope's own lane: planes parked in its pinned area
            _lib.check(L.snarkvm_hip_msm_registered(ctypes.c_void_p(outs[i : i + 1].ctypes.data), rb._h, 0, n - i, ctypes.c_void_p(d_sc[i].data_ptr()), 1, 0))
        assert not outs.view(np.uint8).any()  # nothing delivered yet
        L.snarkvm_hip_set_profiling(1)  # -> msm_scope_enqueue declines, the coalescer declines: the synchronous path on the borrowed lane
        _lib.check(L.snarkvm_hip_msm_registered(ctypes.c_void_p(outs[2:3].ctypes.data), rb._h, 5, n - 5, ctypes.c_void_p(d_sc[2].data_ptr()), 1, 0))
        L.snarkvm_hip_set_profiling(0)
    finally:
        L.snarkvm_hip_set_profiling(0)
        _lib.check(L.snarkvm_hip_scope_end())
    want = [oracle.g1_msm(bases[: n], sc[0]), oracle.g1_msm(bases[: n - 1], sc[1][: n - 1]), oracle.g1_msm(bases[5:n], sc[2][: n - 5])]
    for i in range(3):
        assert util.affine_equal(oracle.g1_to_affine(outs[i : i + 1]), oracle.g1_to_affine(want[i])), i
    rb.close()
