"""Fr NTT and polymul on 2^27 and 2^28 domains (the SRS maximum) on the device, against the CPU oracle.

Memory: a 2^28 vector is 8 GiB; every test keeps at most about four of them alive on the host and frees as it goes.  Inputs are
dense but cheap to make: a random 2^20 vector tiled to the domain size, times c g^i (oracle distribute_powers) - no period survives."""
import concurrent.futures
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, plugin, synthetic
from snarkvm_amd.devmem import HipMem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pyref.R_MOD
NN, NR, RN = oracle.ORDER_NN, oracle.ORDER_NR, oracle.ORDER_RN
FWD, INV = oracle.FORWARD, oracle.INVERSE
STD, COSET = oracle.STANDARD, oracle.COSET
ERR_TOO_LARGE = 2  # hipErrorMemoryAllocation


def limbs(v):
    """a field element (Python int) -> (1, 4) memory Montgomery limbs"""
    return np.array([pyref.to_limbs(pyref.fr_to_mont(v % R), 4)], dtype=np.uint64)


def value(row):
    return pyref.fr_from_mont(pyref.from_limbs(np.asarray(row).reshape(4)))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def scale_powers_in_place(v, g, c):
    """v[i] *= c g^i (oracle distribute_powers, in place: no second copy of a big vector)"""
    gl, cl = limbs(g), limbs(c)  # alive until the call returns
    oracle.lib().oracle_fr_distribute_powers(_p(v), ctypes.c_size_t(v.shape[0]), _p(gl), _p(cl))
    return v


def powers(n, g, c):
    """(n, 4): c g^i"""
    v = np.empty((n, 4), dtype=np.uint64)
    v[:] = limbs(1)
    return scale_powers_in_place(v, g, c)


def dense(lg, seed):
    base = oracle.fr_op("from_bigint", synthetic.random_fr_integers(1 << min(lg, 20), seed))
    v = np.tile(base, (1 << max(lg - 20, 0), 1))
    del base
    rng = random.Random(seed)
    return scale_powers_in_place(v, rng.randrange(2, R), rng.randrange(1, R))


def bitrev_perm(lg):
    i = np.arange(1 << lg, dtype=np.uint32)
    for sh, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF)):
        i = ((i >> np.uint32(sh)) & np.uint32(m)) | ((i & np.uint32(m)) << np.uint32(sh))
    i = (i >> np.uint32(16)) | (i << np.uint32(16))
    return (i >> np.uint32(32 - lg)).astype(np.int64)


def on_device(x, lg, steps):
    """upload x, apply snarkvm_hip_ntt_device (order, direction, type) for every step in place, download"""
    assert x.shape == (1 << lg, 4)
    buf = HipMem.from_numpy(x)
    try:
        for order, d, t in steps:
            _lib.check(_lib.lib().snarkvm_hip_ntt_device(ctypes.c_void_p(buf.ptr), ctypes.c_uint32(lg), order, d, t))
        return buf.download(dtype=np.uint64).reshape(-1, 4)
    finally:
        buf.free()


def fr_sum(x):
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = oracle.fr_vec_op("add", x[:h], x[h:])
    return x


def evaluate(poly, z):
    """poly(z) through oracle.poly_evaluate over 16 chunks at once (the calls release the GIL), combined with Python integers"""
    n = poly.shape[0]
    chunk = max(1, -(-n // 16))
    starts = list(range(0, n, chunk))
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda s: value(oracle.poly_evaluate(poly[s : s + chunk], limbs(z))), starts))
    return sum(p * pow(z, s, R) for p, s in zip(parts, starts)) % R


@pytest.mark.parametrize("lg", [27])
def test_ntt_2_27_against_oracle(lg):
    x = dense(lg, 0x2701)
    y = on_device(x, lg, [(NN, FWD, STD)])
    want = oracle.ntt(x)
    assert np.array_equal(y, want), "forward standard"
    del want
    # inverse standard by round trip
    assert np.array_equal(on_device(y, lg, [(NN, INV, STD)]), x), "inverse standard round trip"
    # NR / RN against a numpy bit reversal of the NN result
    perm = bitrev_perm(lg)
    got = on_device(x, lg, [(NR, FWD, STD)])
    assert np.array_equal(got, y[perm]), "NR"
    del got
    xr = x[perm]
    del perm
    got = on_device(xr, lg, [(RN, FWD, STD)])
    del xr
    assert np.array_equal(got, y), "RN"
    del got, y
    # inverse coset against the oracle, forward coset by round trip
    got = on_device(x, lg, [(NN, INV, COSET)])
    want = oracle.ntt(x, NN, INV, COSET)
    assert np.array_equal(got, want), "inverse coset"
    del want
    assert np.array_equal(on_device(got, lg, [(NN, FWD, COSET)]), x), "forward coset round trip"


def test_ntt_2_28_against_oracle():
    lg = 28
    x = dense(lg, 0x2801)
    y = on_device(x, lg, [(NN, FWD, STD)])
    assert value(y[0]) == value(fr_sum(x)[0]), "X[0] = sum x"
    want = oracle.ntt(x)
    assert np.array_equal(y, want), "forward standard"
    del want
    assert np.array_equal(on_device(y, lg, [(NN, INV, STD)]), x), "inverse standard after forward"
    del y
    assert np.array_equal(on_device(x, lg, [(NN, INV, STD), (NN, FWD, STD)]), x), "forward standard after inverse"
    assert np.array_equal(on_device(x, lg, [(NN, FWD, COSET), (NN, INV, COSET)]), x), "inverse coset after forward"
    assert np.array_equal(on_device(x, lg, [(NN, INV, COSET), (NN, FWD, COSET)]), x), "forward coset after inverse"


@pytest.mark.parametrize("lg", [27, 28])
def test_sparse_input_closed_form(lg):
    """x_0 = c0, x_m = c1 (m odd): every output element of all four transforms against c0 A^k a + c1 B^k b"""
    n = 1 << lg
    rng = random.Random(lg)
    c0, c1 = rng.randrange(1, R), rng.randrange(1, R)
    m = rng.randrange(n // 4, n) | 1
    dom = oracle.domain(lg)
    w = value(dom[0])
    assert w == pow(pyref.FR_TWO_ADIC_ROOT, 1 << (pyref.FR_TWO_ADICITY - lg), R)
    wi, ninv, gi, g = value(dom[1]), value(dom[2]), value(dom[3]), pyref.FR_GENERATOR
    cases = {
        (FWD, STD): ((1, c0), (pow(w, m, R), c1)),
        (FWD, COSET): ((1, c0), (pow(w, m, R), c1 * pow(g, m, R))),
        (INV, STD): ((1, c0 * ninv), (pow(wi, m, R), c1 * ninv)),
        (INV, COSET): ((gi, c0 * ninv), (gi * pow(wi, m, R), c1 * ninv)),
    }
    for (d, t), ((a, ca), (b, cb)) in cases.items():
        buf = HipMem(32 * n)
        try:
            buf.fill(0, 0, 32 * n)
            buf.upload(limbs(c0), 0)
            buf.upload(limbs(c1), 32 * m)
            _lib.check(_lib.lib().snarkvm_hip_ntt_device(ctypes.c_void_p(buf.ptr), ctypes.c_uint32(lg), NN, d, t))
            e1 = powers(n, a, ca)
            e2 = powers(n, b, cb)
            want = oracle.fr_vec_op("add", e1, e2)
            del e1, e2
            got = buf.download(dtype=np.uint64).reshape(-1, 4)
        finally:
            buf.free()
        assert np.array_equal(got, want), (lg, d, t)
        del got, want


@pytest.mark.parametrize("lg", [27, 28])
def test_polymul(lg):
    n = 1 << lg
    half = n // 2
    a = dense(lg - 1, 0x5A00 + lg)
    b = dense(lg - 1, 0x5B00 + lg)
    prod = plugin.polymul(n, [a, b], [])
    rng = random.Random(lg)
    for _ in range(3):  # Schwartz-Zippel: a wrong product agrees at a random point with probability < 2^28 / r
        z = rng.randrange(2, R)
        assert evaluate(prod, z) == evaluate(a, z) * evaluate(b, z) % R
    del prod, b
    # a monomial times a dense polynomial: exactly a shift
    t = rng.randrange(1, 1 << 20)
    mono = np.zeros((t + 1, 4), dtype=np.uint64)
    mono[t] = limbs(1)[0]
    got = plugin.polymul(n, [mono, a], [])
    assert not got[:t].any() and np.array_equal(got[t : t + half], a) and not got[t + half :].any()
    del got, a
    # one evaluation vector alone: zero-padded inverse transform, as snarkvm_ntt computes it
    e = dense(lg, 0x5C00 + lg)
    got = plugin.polymul(n, [], [e])
    plugin.NTT(n, e, NN, INV, STD)
    assert np.array_equal(got, e)


def test_batch_2_27_equals_single_calls():
    lg = 27
    xs = [dense(lg, 0xBA00 + i) for i in range(2)]
    bufs = [HipMem.from_numpy(x) for x in xs]
    try:
        ptrs = [b.ptr for b in bufs]
        plugin.NTT_device_batch(lg, ptrs, directions=[FWD, INV], types=[STD, COSET])  # mixed: two single-vector runs
        plugin.NTT_device_batch(lg, ptrs, directions=[INV, INV], types=[STD, STD])  # one batched launch per pass
        got = [b.download(dtype=np.uint64).reshape(-1, 4) for b in bufs]
    finally:
        for b in bufs:
            b.free()
    assert np.array_equal(got[0], on_device(xs[0], lg, [(NN, FWD, STD), (NN, INV, STD)]))
    assert np.array_equal(got[1], on_device(xs[1], lg, [(NN, INV, COSET), (NN, INV, STD)]))


CHAIN = [(NN, FWD, STD), (NN, FWD, COSET), (NN, INV, STD), (NN, INV, COSET)]


def chain_digest(lg):
    """sha256 of the four transforms applied one after the other to a dense vector (a transform is a bijection: any difference
    in any of them reaches the end)"""
    return hashlib.sha256(on_device(dense(lg, 0x7E00 + lg), lg, CHAIN).tobytes()).hexdigest()


@pytest.mark.parametrize("lg", [27, 28])
def test_tuning_paths_are_bit_identical(lg):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_ntt_large import chain_digest; print(chain_digest({lg}))"
    want = chain_digest(lg)
    for tuning in ("ntt_full_tw=0", "ntt_fold=0,ntt_min_tiles=262144"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SNARKVM_HIP_TUNING=tuning), capture_output=True, text=True, timeout=600,
                           cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip().splitlines()[-1] == want, tuning


def test_lg_29_is_rejected_and_leaves_the_buffer_alone():
    x = oracle.fr_op("from_bigint", synthetic.random_fr_integers(16, 0x29))
    buf = HipMem.from_numpy(x)
    L = _lib.lib()
    try:
        for fn, args in ((L.snarkvm_hip_ntt_device, (ctypes.c_void_p(buf.ptr), ctypes.c_uint32(29), 0, 0, 0)),
                         (L.snarkvm_hip_ntt_device_batch, ((ctypes.c_void_p * 1)(buf.ptr), ctypes.c_size_t(1), ctypes.c_uint32(29), 0, None, None))):
            with pytest.raises(_lib.HipError) as e:
                _lib.check(fn(*args))
            assert e.value.code == ERR_TOO_LARGE and "28" in e.value.message
        assert np.array_equal(buf.download(dtype=np.uint64).reshape(-1, 4), x)
    finally:
        buf.free()
    h = x.copy()
    with pytest.raises(_lib.HipError) as e:
        _lib.check(L.snarkvm_ntt(_p(h), ctypes.c_uint32(29), 0, 0, 0))
    assert e.value.code == ERR_TOO_LARGE
    assert np.array_equal(h, x)
    out = np.zeros((16, 4), dtype=np.uint64)
    pp = (ctypes.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    pl = (ctypes.c_size_t * 2)(1, 1)
    with pytest.raises(_lib.HipError) as e:
        _lib.check(L.snarkvm_polymul(_p(out), ctypes.c_size_t(2), pp, pl, ctypes.c_size_t(0), None, None, ctypes.c_uint32(29)))
    assert e.value.code == ERR_TOO_LARGE and not out.any()
