"""Fr NTT and polymul parity holes below 2^27: every element of every order, type and direction through all three NTT entry
points up to 2^26, the closing-twiddle cache under pressure, and every operand mix `snarkvm_polymul` accepts.

References: the CPU oracle (oracle.ntt / oracle.polymul), closed forms that depend only on the pinned root of unity, schoolbook
multiplication (pyref.poly_mul_naive) and Schwartz-Zippel at random points.  Bit-reversed orders are derived from the checked NN
result with a numpy permutation, so no second oracle transform is needed.  Large arrays are dropped as soon as they have been
used (a 2^26 vector is 2 GiB)."""
import concurrent.futures
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, fft, plugin
from snarkvm_amd.devmem import HipMem
from tests import util
from tests.test_gpu_ntt_large import bitrev_perm, dense, evaluate, limbs, on_device, powers, scale_powers_in_place

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pyref.R_MOD
NN, NR, RN, RR = oracle.ORDER_NN, oracle.ORDER_NR, oracle.ORDER_RN, oracle.ORDER_RR
FWD, INV = oracle.FORWARD, oracle.INVERSE
STD, COSET = oracle.STANDARD, oracle.COSET
KINDS = [(FWD, STD), (FWD, COSET), (INV, STD), (INV, COSET)]
ORDERS = {NR: (False, True), RN: (True, False), RR: (True, True)}  # order -> (input bit-reversed, output bit-reversed)
ERR_INVALID = 1  # hipErrorInvalidValue


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def on_host(x, lg, order, d, t):
    """snarkvm_ntt on a copy of x"""
    y = x.copy()
    plugin.NTT(1 << lg, y, order, d, t)
    return y


def run_batch(lg, inputs, entries, order, check):
    """snarkvm_hip_ntt_device_batch over one device copy of every input; entries: (input index, direction, type) in list order.
    check(i, got) is called for every input in turn, so only one result is on the host at a time."""
    bufs = []
    try:
        for x in inputs:  # a repeated input is copied on the device (2 GiB host uploads dominate at 2^26)
            same = next((b for y, b in zip(inputs, bufs) if y is x), None)
            if same is None:
                bufs.append(HipMem.from_numpy(x))
            else:
                bufs.append(HipMem(same.nbytes))
                bufs[-1].copy_from(0, same.ptr, same.nbytes)
        plugin.NTT_device_batch(lg, [bufs[i].ptr for i, _, _ in entries], [d for _, d, _ in entries], [t for _, _, t in entries], ntt_order=order)
        for i, b in enumerate(bufs):
            got = b.download(dtype=np.uint64).reshape(-1, 4)
            b.free()
            check(i, got)
            del got
    finally:
        for b in bufs:
            b.free()


def coset_shift(x):
    """x_i g^i: (NN, INV, STD) after (NN, FWD, COSET)"""
    return scale_powers_in_place(x.copy(), pyref.FR_GENERATOR, 1)


# ------------------------------------------------------------------------------------------ A. NTT: orders x types x directions
def check_orders(lg, x, want):
    """NR / RN / RR x all four transforms through snarkvm_ntt, snarkvm_hip_ntt_device and snarkvm_hip_ntt_device_batch.
    want[(d, t)]: the checked NN result of x."""
    perm = bitrev_perm(lg)
    xr = x[perm]
    wr = {k: want[k][perm] for k in KINDS}
    for d, t in KINDS:
        for order, (rin, rout) in ORDERS.items():
            inp, exp = (xr if rin else x), (wr if rout else want)[d, t]
            assert np.array_equal(on_host(inp, lg, order, d, t), exp), ("snarkvm_ntt", lg, order, d, t)
            assert np.array_equal(on_device(inp, lg, [(order, d, t)]), exp), ("ntt_device", lg, order, d, t)
    # one batch per order: the four transforms of four vectors, then a fifth vector listed twice (forward coset, then inverse
    # standard).  Only RR has a closed form for the pair without a further transform: P G P P Fc P x = P D P x, D = diag(g^i).
    for order, (rin, rout) in ORDERS.items():
        inp = xr if rin else x
        entries = [(0, FWD, STD), (1, FWD, COSET), (2, INV, STD), (3, INV, COSET)]
        inputs = [inp] * 4
        if order == RR:
            entries = [(4, FWD, COSET)] + entries + [(4, INV, STD)]
            inputs = inputs + [inp]

        def check(i, got):
            if i == 4:
                exp = coset_shift(x)[perm]
            else:
                exp = (wr if rout else want)[KINDS[i]]
            assert np.array_equal(got, exp), ("ntt_device_batch", lg, order, i)

        run_batch(lg, inputs, entries, order, check)
    del xr, wr, perm


@pytest.mark.parametrize("lg", [0, 1, 2, 7, 8, 9, 16, 17, 18, 20, 23, 24])
def test_ntt_orders_all_entry_points(lg):
    x = dense(lg, 0x0D00 + lg)
    want = {(d, t): oracle.ntt(x, NN, d, t) for d, t in KINDS}
    for d, t in KINDS:
        assert np.array_equal(on_host(x, lg, NN, d, t), want[d, t]), (lg, d, t)
    check_orders(lg, x, want)


@pytest.mark.parametrize("lg", [1, 2, 7, 8, 9, 16])
def test_ntt_batch_non_nn_order_listed_twice(lg):
    """a non-NN batch of small vectors (lg <= 8: one pass; > 8: the per-vector fallback of a batchable size) where one vector
    is listed twice with non-commuting transforms, for every order: expectation from two oracle transforms"""
    xs = [dense(lg, 0x0B00 + 8 * lg + i) for i in range(3)]
    entries = [(0, FWD, COSET), (1, INV, STD), (2, FWD, STD), (0, INV, COSET), (1, FWD, COSET)]
    for order in ORDERS:
        want = [x.copy() for x in xs]
        for i, d, t in entries:
            want[i] = oracle.ntt(want[i], order, d, t)

        def check(i, got):
            assert np.array_equal(got, want[i]), (lg, order, i)

        run_batch(lg, xs, entries, order, check)


@pytest.mark.parametrize("lg", [25, 26])
def test_ntt_2_25_2_26_every_transform_and_order(lg):
    """every element of all four NN transforms against the oracle (a round trip passes transforms that are wrong the same way
    in both directions), then every order through every entry point from those results.  2^26: the first pass composes its
    twiddles (its table would be 2 GiB, over the cache cap), the pass before the last uses a folded table."""
    x = dense(lg, 0x2500 + lg)
    want = {}
    for d, t in KINDS:
        got = on_device(x, lg, [(NN, d, t)])
        want[d, t] = oracle.ntt(x, NN, d, t)
        assert np.array_equal(got, want[d, t]), (lg, d, t)
        del got
    check_orders(lg, x, want)


@pytest.mark.parametrize("lg", range(1, 27))
def test_sparse_input_closed_form(lg):
    """x_0 = c0, x_m = c1 (m odd): every output element of all four transforms against c0 A^k a + c1 B^k b (as at 2^27 / 2^28 in
    test_gpu_ntt_large); host entry point at even lg, device entry point at odd lg"""
    n = 1 << lg
    rng = random.Random(0x5900 + lg)
    c0, c1 = rng.randrange(1, R), rng.randrange(1, R)
    m = rng.randrange(n // 4, n) | 1
    w = pow(pyref.FR_TWO_ADIC_ROOT, 1 << (pyref.FR_TWO_ADICITY - lg), R)
    wi, ninv, g = pow(w, -1, R), pow(n, -1, R), pyref.FR_GENERATOR
    gi = pow(g, -1, R)
    cases = {
        (FWD, STD): ((1, c0), (pow(w, m, R), c1)),
        (FWD, COSET): ((1, c0), (pow(w, m, R), c1 * pow(g, m, R))),
        (INV, STD): ((1, c0 * ninv), (pow(wi, m, R), c1 * ninv)),
        (INV, COSET): ((gi, c0 * ninv), (gi * pow(wi, m, R), c1 * ninv)),
    }
    for (d, t), ((a, ca), (b, cb)) in cases.items():
        x = np.zeros((n, 4), dtype=np.uint64)
        x[0], x[m] = limbs(c0)[0], limbs(c1)[0]
        if lg % 2 == 0:
            got = on_host(x, lg, NN, d, t)
        else:
            got = on_device(x, lg, [(NN, d, t)])
        del x
        e1 = powers(n, a, ca)
        e2 = powers(n, b, cb)
        want = oracle.fr_vec_op("add", e1, e2)
        del e1, e2
        assert np.array_equal(got, want), (lg, d, t)
        del got, want


def test_ntt_null_buffer_is_invalid_value():
    """snarkvm_ntt rejects a null buffer at a valid size (lg 27 has been valid since the 2^27 / 2^28 plans) with hipErrorInvalidValue"""
    for lg in (14, 27):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(_lib.lib().snarkvm_ntt(None, ctypes.c_uint32(lg), 0, 0, 0))
        assert e.value.code == ERR_INVALID and "null" in e.value.message, lg


# ------------------------------------------------------------------------------------------ A. twiddle-cache pressure
# The cap (SNARKVM_HIP_NTT_TW_MB) is read once per process, so every cap runs in a subprocess of its own.  The first pass of a
# plan with >= 2 passes has a + s = lg: its table holds 2^lg entries of 32 B.  2^20 (6+7+7): 32 MiB; 2^21 (7+7+7): 64 MiB;
# 2^22 (7+7+8): 128 MiB; 2^24 (8+8+8): 512 MiB.  The pass before the last (folded): 2^13 ... 2^16 entries, <= 2 MiB.
#   0:   nothing is materialised, every pass composes, no last pass ends with the bare reduction
#   40:  the 2^20 table (forward or inverse, not both) and the small folded ones fit; 2^21 - 2^24 first passes compose while
#        their pass before the last reads a folded table
#   700: one 2^24 table fits, not two: 2^24 forward and inverse evict each other; while one is held, the other composes
PRESSURE_LGS = (16, 18, 20, 21, 22, 24)


def tw_pressure_run():
    """body of one subprocess: 8 threads issue a shuffled mix of NTTs (all four transforms, host / device / batch entry points),
    every result against the oracle; then a sequential pass alternating directions so that tables are evicted and rebuilt"""
    oracle.set_threads(min(16, os.cpu_count() or 1))
    xs = {lg: dense(lg, 0x7100 + lg) for lg in PRESSURE_LGS}
    want = {(lg, d, t): oracle.ntt(xs[lg], NN, d, t) for lg in PRESSURE_LGS for d, t in KINDS}
    jobs = []
    for lg in PRESSURE_LGS:
        for k, (d, t) in enumerate(KINDS):
            jobs.append(("host", lg, NN if k % 2 else NR, d, t))
            jobs.append(("device", lg, RN if (lg + k) % 3 == 0 else NN, d, t))
        jobs.append(("batch", lg, NN, None, None))
        jobs.append(("batch", lg, RR, None, None))
    random.Random(0x71).shuffle(jobs)

    def expect(lg, order, d, t):
        w = want[lg, d, t]
        return w[bitrev_perm(lg)] if ORDERS.get(order, (False, False))[1] else w

    def job(spec):
        kind, lg, order, d, t = spec
        x = xs[lg]
        inp = x[bitrev_perm(lg)] if ORDERS.get(order, (False, False))[0] else x
        if kind == "host":
            assert np.array_equal(on_host(inp, lg, order, d, t), expect(lg, order, d, t)), spec
        elif kind == "device":
            assert np.array_equal(on_device(inp, lg, [(order, d, t)]), expect(lg, order, d, t)), spec
        else:
            # NN: the first two entries travel as one batched launch per pass, then two single runs
            entries = [(0, FWD, STD), (1, FWD, STD), (2, INV, COSET), (3, FWD, COSET)]

            def check(i, got):
                assert np.array_equal(got, expect(lg, order, *entries[i][1:])), (spec, i)

            run_batch(lg, [inp] * 4, entries, order, check)
        return spec

    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        done = list(ex.map(job, jobs))
    assert len(done) == len(jobs)
    for _ in range(2):
        for lg in (24, 20, 22):
            for d in (FWD, INV, FWD):
                assert np.array_equal(on_device(xs[lg], lg, [(NN, d, STD)]), want[lg, d, STD]), ("sequential", lg, d)
    print("tw_pressure ok")


@pytest.mark.parametrize("cap_mb", [0, 40, 700])
def test_twiddle_cache_pressure(cap_mb):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_fr_parity import tw_pressure_run; tw_pressure_run()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SNARKVM_HIP_NTT_TW_MB=str(cap_mb)), capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1] == "tw_pressure ok"


# ------------------------------------------------------------------------------------------ B. polymul
def rand_poly(rng, length):
    """random coefficients, the leading one non-zero (a trimmed DensePolynomial)"""
    return [rng.randrange(R) for _ in range(length - 1)] + [rng.randrange(1, R)] if length else []


def fr(ints):
    return util.ints_to_fr_mont(ints) if ints else np.zeros((0, 4), dtype=np.uint64)


def log2_ceil(k):
    return max(0, (k - 1).bit_length())


def test_polymul_n_random_vs_naive():
    """mul_polynomials_n_random (dense.rs:643-690) restated: 1 - 8 polynomials of degree < 256 plus up to 3 evaluation vectors
    (FFTs of polynomials over the product's domain, added while they fit); the trimmed product equals schoolbook multiplication,
    and the full-length snarkvm_polymul result equals the oracle's"""
    max_degree = 1 << 8
    seen = set()
    for case in range(24):
        rng = random.Random(0xD643 + case)
        num_polys, num_evals = 1 + case % 8, case % 4
        a = rand_poly(rng, max_degree // 2 + 1)
        polys, naive = [a], a
        mul_degree = len(a)
        for _ in range(1, num_polys):
            deg = rng.randrange(max_degree)
            mul_degree += deg + 1
            p = rand_poly(rng, deg + 1)
            polys.append(p)
            naive = pyref.poly_mul_naive(naive, p)
        dom = fft.EvaluationDomain.new(mul_degree)
        lg = dom.log_size_of_group
        evals, eval_degree = [], mul_degree
        for _ in range(num_evals):
            e = rand_poly(rng, mul_degree // 8 + 1)
            eval_degree += len(e) + 1
            if eval_degree < dom.size:
                evals.append(oracle.ntt(np.vstack([fr(e), np.zeros((dom.size - len(e), 4), dtype=np.uint64)])))
                naive = pyref.poly_mul_naive(naive, e)
        pm = fft.PolyMultiplier()
        for p in polys:
            pm.add_polynomial(fr(p))
        for e in evals:
            pm.add_evaluation(e)
        got = pm.multiply()
        assert util.fr_mont_to_ints(got) == naive, (case, len(polys), len(evals))
        pf = [fr(p) for p in polys]
        assert np.array_equal(plugin.polymul(dom.size, pf, evals), oracle.polymul(lg, pf, evals)), case
        seen.add((len(polys), len(evals)))
    # the mix covers the single-polynomial copy, k >= 3 polynomial operands and three evaluation vectors
    assert (1, 0) in seen and max(p for p, _ in seen) == 8 and max(e for _, e in seen) == 3, sorted(seen)


def test_polymul_corner_cases():
    """mul_polynomials_corner_cases (dense.rs:692-708): a single polynomial comes back as it is"""
    a = fr(rand_poly(random.Random(70), 71))
    pm = fft.PolyMultiplier()
    pm.add_polynomial(a)
    assert np.array_equal(pm.multiply(), a)


def test_poly_multiplier_semantics():
    rng = random.Random(0x5E)
    a, b = fr(rand_poly(rng, 40)), fr(rand_poly(rng, 30))
    # the domain is the next power of two of sum(deg + 1) = 70: 128; an evaluation vector over 64 or 256 points: None
    for size in (64, 256):
        pm = fft.PolyMultiplier()
        pm.add_polynomial(a)
        pm.add_polynomial(b)
        pm.add_evaluation(dense(log2_ceil(size), size))
        assert pm.multiply() is None, size
    # evaluations alone: the domain has size 1 (no polynomial adds to the degree), as in the reference
    e = dense(0, 1)
    pm = fft.PolyMultiplier()
    pm.add_evaluation(e)
    assert np.array_equal(pm.multiply(), e)
    pm = fft.PolyMultiplier()
    pm.add_evaluation(dense(2, 2))
    pm.add_evaluation(dense(2, 3))
    assert pm.multiply() is None
    # untrimmed inputs: the domain counts their full length (5 -> 8), the result has its trailing zeros trimmed
    pm = fft.PolyMultiplier()
    pm.add_polynomial(fr([1, 2, 0, 0]))
    pm.add_polynomial(fr([3]))
    got = pm.multiply()
    assert util.fr_mont_to_ints(got) == [3, 6]
    assert fft.PolyMultiplier().multiply().shape == (0, 4)


def check_polymul(lg, polys, evals):
    got = plugin.polymul(1 << lg, polys, evals)
    want = oracle.polymul(lg, polys, evals)
    assert np.array_equal(got, want), (lg, [p.shape[0] for p in polys], len(evals))
    return got


def test_polymul_2_16_eight_operands():
    """5 polynomials then 3 evaluation vectors (the ABI's order): operands 3 - 7 reuse the two operand buffers"""
    lg, n = 16, 1 << 16
    polys = [dense(13, 0x1600 + i)[: 4000 + 97 * i] for i in range(5)]
    evals = [dense(lg, 0x1610 + i) for i in range(3)]
    check_polymul(lg, polys, evals)
    assert sum(p.shape[0] for p in polys) < n


def test_polymul_2_20_six_operands():
    lg = 20
    full = dense(lg, 0x2000)  # length exactly n: the product wraps
    polys = [full, dense(16, 0x2001), dense(10, 0x2002)[:777], dense(18, 0x2003)]
    evals = [dense(lg, 0x2010 + i) for i in range(2)]
    got = check_polymul(lg, polys, evals)
    assert got.any()
    # a polynomial of length 0 among them: the zero polynomial, so the product is zero
    polys[2] = np.zeros((0, 4), dtype=np.uint64)
    got = check_polymul(lg, polys, evals)
    assert not got.any()


def test_polymul_2_22_four_operands():
    lg = 22
    polys = [dense(20, 0x2200 + i) for i in range(3)]
    evals = [dense(lg, 0x2210)]
    check_polymul(lg, polys, evals)


def test_polymul_2_24_two_operands():
    """the product bench.py times"""
    lg = 24
    check_polymul(lg, [dense(23, 0x2400), dense(23, 0x2401)[:-5]], [])


@pytest.mark.parametrize("lg", [25, 26])
def test_polymul_four_operands_schwartz_zippel(lg):
    polys = [dense(lg - 2, 0x5200 + 4 * lg + i) for i in range(4)]
    polys[3] = polys[3][:-3]
    prod = plugin.polymul(1 << lg, polys, [])
    rng = random.Random(lg)
    for _ in range(3):  # a wrong product agrees at a random point with probability < 2^26 / r
        z = rng.randrange(2, R)
        want = 1
        for p in polys:
            want = want * evaluate(p, z) % R
        assert evaluate(prod, z) == want
    assert not prod[sum(p.shape[0] - 1 for p in polys) + 1 :].any()


@pytest.mark.parametrize("lg", [10, 20])
def test_polymul_evaluations_only(lg):
    """pcount = 0: operand 0 is an evaluation vector and must not be transformed; the product is iNTT(prod e_k)"""
    evals = [dense(lg, 0xE000 + 8 * lg + i) for i in range(5)]
    for k in (2, 3, 5):
        got = check_polymul(lg, [], evals[:k])
        prod = evals[0]
        for e in evals[1:k]:
            prod = oracle.fr_vec_op("mul", prod, e)
        assert np.array_equal(got, oracle.ntt(prod, NN, INV, STD)), k
    # the single evaluation vector: zero-pad (nothing to pad at full length) and inverse transform
    assert np.array_equal(check_polymul(lg, [], evals[:1]), oracle.ntt(evals[0], NN, INV, STD))


def test_polymul_cyclic_wrap():
    """a product longer than the domain wraps cyclically (the caller chooses lg): the product modulo X^n - 1"""
    rng = random.Random(0xC1C)
    lg, n = 10, 1 << 10
    ps = [rand_poly(rng, k) for k in (700, 600, 400)]
    naive = ps[0]
    for p in ps[1:]:
        naive = pyref.poly_mul_naive(naive, p)
    folded = [0] * n
    for i, c in enumerate(naive):
        folded[i % n] = (folded[i % n] + c) % R
    got = check_polymul(lg, [fr(p) for p in ps], [])
    assert util.fr_mont_to_ints(got) == folded
    # larger: three polynomials of n / 2 and one evaluation vector at 2^16
    check_polymul(16, [dense(15, 0xC100 + i) for i in range(3)], [dense(16, 0xC110)])


def raw_polymul(out, polys, plens, evals, elens, lg):
    pp = (ctypes.c_void_p * max(1, len(polys)))(*[p.ctypes.data for p in polys])
    pl = (ctypes.c_size_t * max(1, len(plens)))(*plens)
    ep = (ctypes.c_void_p * max(1, len(evals)))(*[e.ctypes.data for e in evals])
    el = (ctypes.c_size_t * max(1, len(elens)))(*elens)
    return _lib.lib().snarkvm_polymul(_p(out), ctypes.c_size_t(len(polys)), pp, pl, ctypes.c_size_t(len(evals)), ep, el, ctypes.c_uint32(lg))


def test_polymul_argument_errors_leave_out_alone():
    lg, n = 8, 1 << 8
    long_p, short_p, ev = dense(9, 1), dense(6, 2), dense(lg, 3)
    sentinel = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    cases = [
        ([long_p, short_p], [n + 1, short_p.shape[0]], [], []),  # a polynomial longer than n
        ([short_p, long_p], [short_p.shape[0], n + 1], [ev], [n]),
        ([short_p], [short_p.shape[0]], [ev], [n - 1]),  # an evaluation vector of the wrong length
        ([], [], [ev, long_p], [n, n + 1]),
        ([], [], [ev], [n - 1]),  # the single-evaluation corner case checks the length too
    ]
    for polys, plens, evals, elens in cases:
        out = sentinel.copy()
        with pytest.raises(_lib.HipError) as e:
            _lib.check(raw_polymul(out, polys, plens, evals, elens, lg))
        assert e.value.code == ERR_INVALID, (plens, elens)
        assert np.array_equal(out, sentinel), (plens, elens)
        # the next call on the same thread gives a correct product
        check_polymul(lg, [short_p, short_p[:50]], [ev])


def test_polymul_concurrent_callers_with_ntts():
    """8 threads: polymuls of 4 - 6 operands at 2^14 - 2^20 interleaved with NTTs; the lanes' operand buffers and events and the
    shared twiddle cache together"""
    rng = random.Random(0xCC)
    jobs = []
    for j in range(24):
        lg = 14 + j % 7
        if j % 3 == 2:
            x = dense(lg, 0xCC00 + j)
            d, t = KINDS[j % 4]
            jobs.append(("ntt", lg, x, (d, t), oracle.ntt(x, NN, d, t)))
            continue
        k = 4 + j % 3
        ne = j % 3
        polys = [dense(lg - 3, 0xCD00 + 16 * j + i)[: (1 << (lg - 3)) - rng.randrange(8)] for i in range(k - ne)]
        evals = [dense(lg, 0xCE00 + 16 * j + i) for i in range(ne)]
        jobs.append(("polymul", lg, polys, evals, oracle.polymul(lg, polys, evals)))

    def run(job):
        kind, lg, a, b, want = job
        if kind == "ntt":
            got = on_device(a, lg, [(NN, *b)]) if lg % 2 else on_host(a, lg, NN, *b)
        else:
            got = plugin.polymul(1 << lg, a, b)
        assert np.array_equal(got, want), (kind, lg)
        return kind

    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        done = list(ex.map(run, jobs * 2))
    assert len(done) == 2 * len(jobs)
