"""The Fr vector passes of a Varuna round (snarkvm_amd/csrc/poly.hip.h, api_poly.hip) at prover sizes, on device memory and strided.

Four groups, every result bit for bit against oracle/cpu.py's restatement of the same reference function (Fr results are unique
Montgomery residues: no tolerances):

  A  past every launch cap: the grid-stride loops take a second trip, the inversion and the powers kernel run with T at its cap and
     unequal per-thread counts
  B  p / (X - z) across its three regimes: scan with C = 8, scan with C = 16, chunk recursion again beyond 2^20
  C  the `_strided` entry points on an arena with stride > n and a sentinel in the gaps
  D  `on_device = 1` single calls at sizes that straddle a workgroup, aliased outputs, and the edge operands 0, 1, r - 1, ...

Device memory moves through snarkvm_amd.devmem.HipMem: no torch in this module."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import cpu as oracle
from oracle import pyref
from snarkvm_amd import _lib, poly
from snarkvm_amd.devmem import HipMem
from tests import util

pytestmark = pytest.mark.gpu

FR_BYTES = 32
OPS = ("add", "sub", "mul", "mul_sub", "scale", "sub_scalar", "axpy", "rsub_scalar")
NEEDS_B = {"add", "sub", "mul", "mul_sub", "axpy"}
NEEDS_S = {"scale", "sub_scalar", "axpy", "rsub_scalar"}

# the caps as they stand in fr_call.hip.h (fr_grid 8192 x 256 threads, powers T = 2^17), api_fr.hip (fr_mul_device / fr_convert_device 4096 x 256) and api_poly.hip (inversion T = 2^17)
T_CAP = 1 << 17
N_TWO_TRIPS = (1 << 21) + (1 << 20) + 12345       # in (2^21, 2^22), not a multiple of 256: a partial second trip of every grid-stride loop
N_T_CAPPED = (1 << 22) + 3 * (1 << 17) + 77        # T at its cap, 35 or 36 elements per thread, ragged tail
BIG = (N_TWO_TRIPS, N_T_CAPPED)
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def zeros(n):
    return np.zeros((n, 4), dtype=np.uint64)


R_LIMBS = np.array(pyref.to_limbs(pyref.R_MOD, 4), dtype=np.uint64)


@functools.lru_cache(maxsize=4)
def _rnd_cached(n, seed):
    """253-bit draws, those below r kept (58 %).  Every residue below r is some element's memory image, so the draws are used as they are: uniform
    Fr elements, as from_bigint(random) would give, without a field product per element - this module draws 10^8 of them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, 4), dtype=np.uint64)
    filled = 0
    while filled < n:
        c = rng.integers(0, 1 << 64, size=(max(1024, 2 * (n - filled)), 4), dtype=np.uint64, endpoint=False)
        c[:, 3] &= np.uint64((1 << 61) - 1)
        c = c[c[:, 3] < R_LIMBS[3]]  # (a top limb equal to r's is dropped too: 2^-60 of the draws)
        take = min(n - filled, c.shape[0])
        out[filled : filled + take] = c[:take]
        filled += take
    out.setflags(write=False)
    return out


def rnd(n, seed):
    """n uniform Fr elements, memory form (a fresh writable copy)"""
    return _rnd_cached(n, seed).copy()


def one():
    return util.ints_to_fr_mont([1])


def neg(x):
    return oracle.fr_op("neg", x)


def pad(x, n):
    """the oracle trims like a DensePolynomial; the device writes every coefficient"""
    out = zeros(n)
    out[: x.shape[0]] = x
    return out


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return HipMem.from_numpy(a) if a.size else HipMem(FR_BYTES)


def dev_empty(n, fill=0xA5):
    m = HipMem(FR_BYTES * max(n, 1))
    m.fill(0, fill, m.nbytes)
    return m


def from_dev(m, n, off=0):
    return m.download(FR_BYTES * n, FR_BYTES * off, np.uint64).reshape(-1, 4)


def ptr(m, off=0):
    """device pointer `off` elements into a HipMem (None -> NULL)"""
    return ctypes.c_void_p(m.ptr + FR_BYTES * off) if m is not None else ctypes.c_void_p()


def hptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else ctypes.c_void_p()


def sz(n):
    return ctypes.c_size_t(n)


def L():
    return _lib.lib()


def linear_divisor(z):
    return [(0, neg(np.asarray(z, dtype=np.uint64).reshape(1, 4))[0]), (1, one()[0])]


def vanishing_divisor(D):
    return [(0, neg(one())[0]), (D, one()[0])]


def want_vec_op(op, a, b, c, s):
    if op in ("add", "sub", "mul"):
        return oracle.fr_vec_op(op, a, b)
    if op == "mul_sub":
        return oracle.fr_vec_op(op, a, b, c)
    if op in ("scale", "sub_scalar"):
        return oracle.fr_vec_op(op, a, s)
    if op == "axpy":
        return oracle.fr_vec_op(op, a, b, s)
    return neg(oracle.fr_vec_op("sub_scalar", a, s))  # rsub_scalar: the oracle has no s - a


def vec_op_host(op, a, b, c, s):
    out = np.empty_like(a)
    _lib.check(L().snarkvm_hip_fr_vec_op(poly.VEC_OPS[op], hptr(out), hptr(a), hptr(b if op in NEEDS_B else None), hptr(c if op == "mul_sub" else None),
                                         hptr(s if op in NEEDS_S else None), sz(a.shape[0]), 0))
    return out


def vec_op_dev(op, dout, da, db, dc, s, n):
    _lib.check(L().snarkvm_hip_fr_vec_op(poly.VEC_OPS[op], ptr(dout), ptr(da), ptr(db if op in NEEDS_B else None), ptr(dc if op == "mul_sub" else None),
                                         hptr(s if op in NEEDS_S else None), sz(n), 1))


def divide_by_linear(a, z, with_quotient, on_device):
    """(quotient of n - 1 coefficients or None, remainder) through the raw ABI, host or device operands"""
    n = a.shape[0]
    rem = np.full((1, 4), SENTINEL, dtype=np.uint64)
    wq = with_quotient and n > 1
    if on_device:
        da, dq = to_dev(a), (dev_empty(n - 1) if wq else None)
        _lib.check(L().snarkvm_hip_fr_divide_by_linear(ptr(dq), hptr(rem), ptr(da) if n else ctypes.c_void_p(), sz(n), hptr(z), 1))
        assert np.array_equal(from_dev(da, n), a)  # the input stays as it was
        return (from_dev(dq, n - 1) if wq else None), rem
    q = np.full((n - 1, 4), SENTINEL, dtype=np.uint64) if wq else None
    _lib.check(L().snarkvm_hip_fr_divide_by_linear(hptr(q), hptr(rem), hptr(a), sz(n), hptr(z), 0))
    return q, rem


def check_divide_by_linear(a, z, on_device, label):
    n = a.shape[0]
    wq, _ = oracle.poly_divide(a, linear_divisor(z))
    want_val = oracle.poly_evaluate(a, z)
    q, rem = divide_by_linear(a, z, True, on_device)
    if n > 1:
        assert np.array_equal(q, pad(wq, n - 1)), label
    assert np.array_equal(rem, want_val), label
    _, val = divide_by_linear(a, z, False, on_device)
    assert np.array_equal(val, want_val), label


def batch_inverse(v, coeff, on_device):
    if on_device:
        dv = to_dev(v)
        _lib.check(L().snarkvm_hip_fr_batch_inversion_and_mul(ptr(dv), sz(v.shape[0]), hptr(coeff), 1))
        return from_dev(dv, v.shape[0])
    out = v.copy()
    _lib.check(L().snarkvm_hip_fr_batch_inversion_and_mul(hptr(out), sz(v.shape[0]), hptr(coeff), 0))
    return out


def distribute_powers(v, g, c, on_device):
    if on_device:
        dv = to_dev(v)
        _lib.check(L().snarkvm_hip_fr_distribute_powers(ptr(dv), sz(v.shape[0]), hptr(g), hptr(c), 1))
        return from_dev(dv, v.shape[0])
    out = v.copy()
    _lib.check(L().snarkvm_hip_fr_distribute_powers(hptr(out), sz(v.shape[0]), hptr(g), hptr(c), 0))
    return out


def lagrange(lg, tau, on_device):
    n = 1 << lg
    if on_device:
        dout = dev_empty(n)
        _lib.check(L().snarkvm_hip_fr_lagrange_coefficients(ptr(dout), ctypes.c_uint32(lg), hptr(tau), 1))
        return from_dev(dout, n)
    out = np.full((n, 4), SENTINEL, dtype=np.uint64)
    _lib.check(L().snarkvm_hip_fr_lagrange_coefficients(hptr(out), ctypes.c_uint32(lg), hptr(tau), 0))
    return out


def divide_by_vanishing(a, D, on_device):
    """(quotient of max(len - D, 0), remainder of min(len, D) coefficients), untrimmed"""
    n = a.shape[0]
    qlen, rlen = max(n - D, 0), min(n, D)
    if on_device:
        da, dq, dr = to_dev(a), (dev_empty(qlen) if qlen else None), dev_empty(rlen)
        _lib.check(L().snarkvm_hip_fr_divide_by_vanishing(ptr(dq), ptr(dr), ptr(da), sz(n), sz(D), 1))
        assert np.array_equal(from_dev(da, n), a)
        return (from_dev(dq, qlen) if qlen else zeros(0)), from_dev(dr, rlen)
    q = np.full((qlen, 4), SENTINEL, dtype=np.uint64)
    r = np.full((rlen, 4), SENTINEL, dtype=np.uint64)
    _lib.check(L().snarkvm_hip_fr_divide_by_vanishing(hptr(q) if qlen else ctypes.c_void_p(), hptr(r), hptr(a), sz(n), sz(D), 0))
    return q, r


def mul_by_vanishing(a, D, on_device):
    n = a.shape[0]
    if on_device:
        da, dout = to_dev(a), dev_empty(n + D)
        _lib.check(L().snarkvm_hip_fr_mul_by_vanishing(ptr(dout), ptr(da), sz(n), sz(D), 1))
        assert np.array_equal(from_dev(da, n), a)
        return from_dev(dout, n + D)
    out = np.full((n + D, 4), SENTINEL, dtype=np.uint64)
    _lib.check(L().snarkvm_hip_fr_mul_by_vanishing(hptr(out), hptr(a), sz(n), sz(D), 0))
    return out


def fr_pow(g, k):
    """g^k by square and multiply with the oracle's field product"""
    acc, base = one(), np.asarray(g, dtype=np.uint64).reshape(1, 4)
    while k:
        if k & 1:
            acc = oracle.fr_op("mul", acc, base)
        base = oracle.fr_op("mul", base, base)
        k >>= 1
    return acc


# ---- A. past every cap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BIG)
def test_vec_ops_past_the_grid_cap(n):
    """fr_vec_op_kernel's `i += st`: 8192 x 256 threads cover 2^21 elements per trip."""
    assert n > 8192 * 256
    a, b, c, s = rnd(n, 1), rnd(n, 2), rnd(n, 3), rnd(1, 4)
    da, db, dc, dout = to_dev(a), to_dev(b), to_dev(c), dev_empty(n)
    for op in OPS:
        want = want_vec_op(op, a, b, c, s)
        assert np.array_equal(vec_op_host(op, a, b, c, s), want), (op, "host")
        vec_op_dev(op, dout, da, db, dc, s, n)
        assert np.array_equal(from_dev(dout, n), want), (op, "device")
    for d, h in ((da, a), (db, b), (dc, c)):
        assert np.array_equal(from_dev(d, n), h)


@pytest.mark.parametrize("n", BIG)
def test_mul_device_and_convert_device_past_their_cap(n):
    """fr_mul_device / fr_convert_device: 4096 x 256 threads, three to five trips at these sizes."""
    assert n > 2 * 4096 * 256
    a, b = rnd(n, 5), rnd(n, 6)
    da, db, dout = to_dev(a), to_dev(b), dev_empty(n)
    _lib.check(L().snarkvm_hip_fr_mul_device(ptr(dout), ptr(da), ptr(db), sz(n)))
    assert np.array_equal(from_dev(dout, n), oracle.fr_op("mul", a, b))
    ints = oracle.fr_op("to_bigint", a)
    _lib.check(L().snarkvm_hip_fr_convert_device(ptr(dout), ptr(da), sz(n), 1))
    assert np.array_equal(from_dev(dout, n), ints)
    _lib.check(L().snarkvm_hip_fr_convert_device(ptr(db), ptr(dout), sz(n), 0))
    assert np.array_equal(from_dev(db, n), oracle.fr_op("from_bigint", ints))
    assert np.array_equal(from_dev(da, n), a)


def inversion_zero_positions(n):
    """zeros where the per-thread chains of fr_batch_inverse_kernel begin, end and differ in length"""
    T = min((n + 31) // 32, T_CAP)
    full = (n // T) * T  # first index of the ragged last stride (== n when every thread owns the same count)
    tail = n - full
    pos = {0, 1, 63, 64, T - 1, T, 7, 7 + T, 7 + 2 * T, full - T, full - 1, n - 1, n - 2}  # first stride, a run of zeros down one chain, last full stride, last element
    if tail:
        pos |= {full, full + tail // 2, full - T + tail - 1, full - T + tail}  # tail elements only threads < tail own, and the last elements of threads on either side of that edge
    return sorted(p for p in pos if 0 <= p < n), T, tail


@pytest.mark.parametrize("n", BIG)
def test_batch_inversion_past_the_thread_cap(n):
    """`cnt = (n - t + T - 1) / T` with unequal counts and `scratch[i - T]` across more than 32 strides."""
    pos, T, tail = inversion_zero_positions(n)
    if n == N_T_CAPPED:
        assert T == T_CAP and tail == 77 and n // T == 35
    v = rnd(n, 20)
    v[pos] = 0
    for coeff in (rnd(1, 21), one()):
        want = oracle.batch_inversion_and_mul(v, coeff)
        assert not want[pos].any()
        assert np.array_equal(batch_inverse(v, coeff, 0), want), "host"
        assert np.array_equal(batch_inverse(v, coeff, 1), want), "device"


@pytest.mark.parametrize("n", BIG)
def test_distribute_powers_past_the_thread_cap(n):
    """`step = g^T` with T capped at 2^17 and 35 / 36 elements per thread."""
    v, g, c = rnd(n, 40), rnd(1, 41), rnd(1, 42)
    want = oracle.distribute_powers(v, g, c)
    assert np.array_equal(distribute_powers(v, g, c, 0), want), "host"
    assert np.array_equal(distribute_powers(v, g, c, 1), want), "device"


@pytest.mark.parametrize("lg", [22, 23])
def test_lagrange_coefficients_at_and_past_the_thread_cap(lg):
    """lg = 22: T = 2^22 / 32 is exactly the cap; lg = 23: 64 elements per thread and four trips of the fill / one-hot / s - x kernels."""
    n = 1 << lg
    tau = rnd(1, 50 + lg)
    want = oracle.lagrange_coefficients(lg, tau)
    for on_device in (0, 1):
        assert np.array_equal(lagrange(lg, tau, on_device), want), on_device
    # tau in the domain: the one-hot branch
    k = n * 3 // 4 + 5
    tau_in = fr_pow(oracle.domain(lg)[0:1], k)
    want = oracle.lagrange_coefficients(lg, tau_in)
    assert np.array_equal(want[k], one()[0]) and int(want.any(axis=1).sum()) == 1
    for on_device in (0, 1):
        got = lagrange(lg, tau_in, on_device)
        assert np.array_equal(np.nonzero(got.any(axis=1))[0], [k]) and np.array_equal(got[k], one()[0]), on_device
        assert np.array_equal(got, want), on_device


@pytest.mark.parametrize("n", BIG + (3 * (1 << 21) + 12345,))
def test_vanishing_polynomial_passes_at_domain_2_21(n):
    """X^D - 1 with D = 2^21: coefficient classes of 1 and 2 (first size), 2 and 3 (second), 3 and 4 (third) members, a ragged class each."""
    D = 1 << 21
    a = rnd(n, 60)
    wq, wr = oracle.poly_divide(a, vanishing_divisor(D))
    wm = oracle.mul_by_vanishing(a, D)
    for on_device in (0, 1):
        q, r = divide_by_vanishing(a, D, on_device)
        assert np.array_equal(q, pad(wq, n - D)) and np.array_equal(r, pad(wr, D)), on_device
        assert np.array_equal(mul_by_vanishing(a, D, on_device), wm), on_device


# ---- B. division by X - z across its three regimes -----------------------------------------------------------------------------
DIV_SIZES = [(1 << 19) - 1, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 * (1 << 19) + 12345]


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", DIV_SIZES)
def test_divide_by_linear_regimes(n, on_device):
    """fr_suffix_horner: scan with C = 8 up to 2^19, C = 16 up to 2^20 (257 workgroups would be one too many at 2^19 + 1), chunk recursion beyond;
    evaluate-only always takes the recursion."""
    check_divide_by_linear(rnd(n, 100 + (n & 0xFFFF)), rnd(1, 5), on_device, n)


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", [(1 << 19) + 1, (1 << 20) + 1])
def test_divide_by_linear_special_points_and_exact_division(n, on_device):
    a = rnd(n, 77)
    for z in (zeros(1), one(), neg(one())):
        check_divide_by_linear(a, z, on_device, (n, z.tolist()))
    if n == (1 << 19) + 1:
        # exact: (X - z) * q = [0, q] - z * [q, 0] has the quotient q and remainder zero
        z, q = rnd(1, 6), rnd(n - 1, 8)
        prod = oracle.fr_vec_op("sub", np.concatenate([zeros(1), q]), oracle.fr_vec_op("scale", np.concatenate([q, zeros(1)]), z))
        got_q, rem = divide_by_linear(prod, z, True, on_device)
        assert np.array_equal(got_q, q) and not rem.any()
        assert not oracle.poly_evaluate(prod, z).any()


# ---- C. the strided forms ------------------------------------------------------------------------------------------------------
class Arena:
    """`count` rows `stride` elements apart in one device block, the sentinel everywhere else."""

    def __init__(self, rows, n, count, stride):
        self.n, self.count, self.stride = n, count, stride
        self.size = max(count * stride, (count - 1) * stride + n, 1)
        self.image = np.full((self.size, 4), SENTINEL, dtype=np.uint64)
        if rows is not None:
            for y in range(count):
                self.image[y * stride : y * stride + n] = rows[y]
        self.mem = to_dev(self.image)

    def read(self):
        return from_dev(self.mem, self.size)

    def assert_unchanged(self, label=None):
        assert np.array_equal(self.read(), self.image), label

    def assert_rows(self, want_rows, n=None, label=None):
        """every member equals its expected row, every other byte is what was uploaded"""
        n = self.n if n is None else n
        want = self.image.copy()
        for y in range(self.count):
            want[y * self.stride : y * self.stride + n] = want_rows[y]
        got = self.read()
        for y in range(self.count):
            assert np.array_equal(got[y * self.stride : y * self.stride + n], want_rows[y]), (label, "member", y)
        assert np.array_equal(got, want), (label, "gaps")


def rows_of(n, count, seed):
    return rnd(n * count, seed).reshape(count, n, 4)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n,count,stride", [(1, 3, 1), (33, 5, 40), (70001, 7, 70016), ((1 << 21) + 777, 2, (1 << 21) + 1024)])
def test_vec_op_strided(n, count, stride, in_place):
    a, b, c, s = rows_of(n, count, 11), rows_of(n, count, 12), rows_of(n, count, 13), rnd(1, 14)
    B, C = Arena(b, n, count, stride), Arena(c, n, count, stride)
    for op in OPS:
        A = Arena(a, n, count, stride)
        out = A if in_place else Arena(None, n, count, stride)
        _lib.check(L().snarkvm_hip_fr_vec_op_strided(poly.VEC_OPS[op], ptr(out.mem), ptr(A.mem), ptr(B.mem if op in NEEDS_B else None),
                                                     ptr(C.mem if op == "mul_sub" else None), hptr(s if op in NEEDS_S else None), sz(n), sz(count), sz(stride)))
        out.assert_rows([want_vec_op(op, a[y], b[y], c[y], s) for y in range(count)], label=op)
        if not in_place:
            A.assert_unchanged(op)
    B.assert_unchanged()
    C.assert_unchanged()


@pytest.mark.parametrize("count", [1, 2, 9])
@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 1 << 17, (1 << 19) + 1, (1 << 20) + 1])
def test_divide_by_linear_strided(n, count):
    """count > 1 crossed with the chunk recursion, the scan with C = 8 and C = 16 and the recursion again: per-member scratch slices, remainders as
    count x 32 host bytes, and the evaluate-only form (quotients = NULL)."""
    stride = n + 13
    a, z = rows_of(n, count, 200 + count), rnd(1, 15)
    P, Q = Arena(a, n, count, stride), Arena(None, n, count, stride)
    want_q = [pad(oracle.poly_divide(a[y], linear_divisor(z))[0], n - 1) for y in range(count)]
    want_rem = np.concatenate([oracle.poly_evaluate(a[y], z) for y in range(count)])
    for quotients in (Q, None):
        rem = np.full((count + 1, 4), SENTINEL, dtype=np.uint64)
        _lib.check(L().snarkvm_hip_fr_divide_by_linear_strided(ptr(Q.mem if quotients else None), hptr(rem), ptr(P.mem), sz(n), hptr(z), sz(count), sz(stride)))
        assert np.array_equal(rem[:count], want_rem), ("remainders", quotients is not None)
        assert (rem[count] == SENTINEL).all()
        P.assert_unchanged()
        Q.assert_rows(want_q, n - 1)  # written by the first call, left alone by the evaluate-only one


def test_divide_by_linear_strided_of_nothing_zeroes_the_remainders():
    count = 3
    rem = np.full((count + 1, 4), SENTINEL, dtype=np.uint64)
    z = rnd(1, 16)
    _lib.check(L().snarkvm_hip_fr_divide_by_linear_strided(ctypes.c_void_p(), hptr(rem), ctypes.c_void_p(), sz(0), hptr(z), sz(count), sz(8)))
    assert not rem[:count].any() and (rem[count] == SENTINEL).all()
    assert not oracle.poly_evaluate(zeros(0), z).any()


@pytest.mark.parametrize("count", [1, 4])
@pytest.mark.parametrize("n", [1000, 1024, 1025, 2048, 3 * 1024 + 17])
def test_divide_by_vanishing_strided(n, count):
    D = 1024
    stride = n + 9
    qlen, rlen = max(n - D, 0), min(n, D)
    a = rows_of(n, count, 300 + count)
    P, Q, R = Arena(a, n, count, stride), Arena(None, n, count, stride), Arena(None, n, count, stride)
    _lib.check(L().snarkvm_hip_fr_divide_by_vanishing_strided(ptr(Q.mem), ptr(R.mem), ptr(P.mem), sz(n), sz(D), sz(count), sz(stride)))
    want = [oracle.poly_divide(a[y], vanishing_divisor(D)) for y in range(count)]
    Q.assert_rows([pad(q, qlen) for q, _ in want], qlen, "quotients")
    R.assert_rows([pad(r, rlen) for _, r in want], rlen, "remainders")
    P.assert_unchanged()


def strided_calls(n, count, stride, out, a, b, z):
    """the three strided entry points over the same arenas: (name, thunk returning the RustError)"""
    rem = zeros(max(count, 1))
    return [
        ("vec_op", lambda: L().snarkvm_hip_fr_vec_op_strided(poly.VEC_OPS["add"], ptr(out.mem), ptr(a.mem), ptr(b.mem), None, None, sz(n), sz(count), sz(stride))),
        ("divide_by_linear", lambda: L().snarkvm_hip_fr_divide_by_linear_strided(ptr(out.mem), hptr(rem), ptr(a.mem), sz(n), hptr(z), sz(count), sz(stride))),
        ("divide_by_vanishing", lambda: L().snarkvm_hip_fr_divide_by_vanishing_strided(ptr(out.mem), ptr(b.mem), ptr(a.mem), sz(n), sz(2), sz(count), sz(stride))),
    ]


@pytest.mark.parametrize("count,stride", [(0, 4), (65536, 4), (2, 3)])
def test_strided_argument_rules(count, stride):
    """check_strided: 1 <= count <= 65535, and stride >= n once there is a second member; a refused call writes nothing."""
    n = 4
    rows = max(count, 2)  # arenas as large as the refused call would have touched
    z = rnd(1, 17)
    a, b, out = Arena(None, n, rows, 4), Arena(None, n, rows, 4), Arena(None, n, rows, 4)
    for name, call in strided_calls(n, count, stride, out, a, b, z):
        with pytest.raises(_lib.HipError) as e:
            _lib.check(call())
        assert e.value.code != 0, name
    out.assert_unchanged()
    b.assert_unchanged()
    # the same calls with count = 2 and stride = n are accepted
    for name, call in strided_calls(n, 2, 4, Arena(None, n, 2, 4), Arena(rows_of(n, 2, 18), n, 2, 4), Arena(rows_of(n, 2, 19), n, 2, 4), z):
        _lib.check(call())


def test_divide_by_linear_strided_refuses_overlapping_arenas():
    """the quotient arena may not touch the (count - 1) * stride + n elements of the poly arena; one element past that span it may."""
    n, count, stride = 2049, 2, 2060
    span = (count - 1) * stride + n
    a, z = rows_of(n, count, 400), rnd(1, 18)
    image = np.full((3 * span, 4), SENTINEL, dtype=np.uint64)
    for y in range(count):
        image[span + y * stride : span + y * stride + n] = a[y]  # the polys sit in the middle third
    buf = to_dev(image)
    rem = zeros(count)

    def call(q_off):
        return L().snarkvm_hip_fr_divide_by_linear_strided(ptr(buf, q_off), hptr(rem), ptr(buf, span), sz(n), hptr(z), sz(count), sz(stride))

    for q_off in (1, span - n + 1, span - 1, span, span + 1, span + n - 1, span + stride, 2 * span - 1):
        with pytest.raises(_lib.HipError):
            _lib.check(call(q_off))
        assert np.array_equal(from_dev(buf, 3 * span), image), q_off
    want_q = [pad(oracle.poly_divide(a[y], linear_divisor(z))[0], n - 1) for y in range(count)]
    want_rem = np.concatenate([oracle.poly_evaluate(a[y], z) for y in range(count)])
    for q_off in (2 * span, 0):  # just behind and just in front of the span
        _lib.check(call(q_off))
        want = image.copy()
        for y in range(count):
            want[q_off + y * stride : q_off + y * stride + n - 1] = want_q[y]
        assert np.array_equal(from_dev(buf, 3 * span), want), q_off
        assert np.array_equal(rem, want_rem)
        buf.upload(image)


# ---- D. device-resident single calls and edge operands -------------------------------------------------------------------------
SMALL = [1, 31, 33, 1025, 70001]


@pytest.mark.parametrize("n", SMALL)
def test_device_resident_vec_ops_and_aliases(n):
    a, b, c, s = rnd(n, 1), rnd(n, 2), rnd(n, 3), rnd(1, 4)
    for op in OPS:
        want = want_vec_op(op, a, b, c, s)
        assert np.array_equal(poly.vec_op(op, a, b if op in NEEDS_B else None, c if op == "mul_sub" else None, s if op in NEEDS_S else None), want), op
        for alias in ("none", "a", "b"):
            da, db, dc = to_dev(a), to_dev(b), to_dev(c)
            dout = {"none": dev_empty(n), "a": da, "b": db}[alias]
            vec_op_dev(op, dout, da, db, dc, s, n)
            assert np.array_equal(from_dev(dout, n), want), (op, alias)
            for d, h in ((da, a), (db, b), (dc, c)):
                if d is not dout:
                    assert np.array_equal(from_dev(d, n), h), (op, alias)


@pytest.mark.parametrize("n", SMALL)
def test_device_resident_mul_and_convert(n):
    a, b = rnd(n, 5), rnd(n, 6)
    want = oracle.fr_op("mul", a, b)
    assert np.array_equal(poly.vec_op("mul", a, b), want)
    for alias in ("none", "a", "b"):
        da, db = to_dev(a), to_dev(b)
        dout = {"none": dev_empty(n), "a": da, "b": db}[alias]
        _lib.check(L().snarkvm_hip_fr_mul_device(ptr(dout), ptr(da), ptr(db), sz(n)))
        assert np.array_equal(from_dev(dout, n), want), alias
    ints = oracle.fr_op("to_bigint", a)
    for to_bigint, src, want in ((1, a, ints), (0, ints, oracle.fr_op("from_bigint", ints))):
        dsrc, dout = to_dev(src), dev_empty(n)
        _lib.check(L().snarkvm_hip_fr_convert_device(ptr(dout), ptr(dsrc), sz(n), to_bigint))
        assert np.array_equal(from_dev(dout, n), want) and np.array_equal(from_dev(dsrc, n), src), to_bigint
        _lib.check(L().snarkvm_hip_fr_convert_device(ptr(dsrc), ptr(dsrc), sz(n), to_bigint))  # in place
        assert np.array_equal(from_dev(dsrc, n), want), to_bigint
    assert np.array_equal(oracle.fr_op("from_bigint", ints), a)


@pytest.mark.parametrize("n", SMALL)
def test_device_resident_division_inversion_powers(n):
    a, z = rnd(n, 10 + n), rnd(1, 5)
    check_divide_by_linear(a, z, 1, n)
    q, rem = divide_by_linear(a, z, True, 1)
    hq, hrem = poly.divide_by_linear(a, z)
    assert np.array_equal(poly.trim(q) if n > 1 else zeros(0), hq) and np.array_equal(rem, hrem) and np.array_equal(poly.evaluate(a, z), rem)

    v = rnd(n, 20 + n)
    for k in (0, 5, 17, n - 1, n // 2):
        if n > 3 and k < n:
            v[k] = 0
    coeff = rnd(1, 21)
    got = batch_inverse(v, coeff, 1)
    assert np.array_equal(got, oracle.batch_inversion_and_mul(v, coeff)) and np.array_equal(got, poly.batch_inversion_and_mul(v, coeff))

    g, c = rnd(1, 41), rnd(1, 42)
    got = distribute_powers(a, g, c, 1)
    assert np.array_equal(got, oracle.distribute_powers(a, g, c)) and np.array_equal(got, poly.distribute_powers_and_mul_by_const(a, g, c))


@pytest.mark.parametrize("n", SMALL)
def test_device_resident_vanishing_passes(n):
    D = 8 if n < 1000 else 1024  # 1, 31, 33: below, 3 folds + 7, 4 folds + 1; 1025 = D + 1; 70001: 68 folds and a ragged class
    a = rnd(n, 60 + n)
    q, r = divide_by_vanishing(a, D, 1)
    wq, wr = oracle.poly_divide(a, vanishing_divisor(D))
    assert np.array_equal(q, pad(wq, max(n - D, 0))) and np.array_equal(r, pad(wr, min(n, D)))
    hq, hr = poly.divide_by_vanishing_poly(a, D)
    assert np.array_equal(poly.trim(q), hq) and np.array_equal(poly.trim(r), hr)
    m = mul_by_vanishing(a, D, 1)
    assert np.array_equal(m, oracle.mul_by_vanishing(a, D)) and np.array_equal(poly.trim(m), poly.mul_by_vanishing_poly(a, D))


@pytest.mark.parametrize("lg", [0, 1, 5, 6, 10, 16])
def test_device_resident_lagrange_coefficients(lg):
    """the domain sizes next to 1, 31, 33, 1025 and 70001: this pass only exists on powers of two"""
    n = 1 << lg
    k = n * 3 // 4
    for tau in (rnd(1, 50 + lg), fr_pow(oracle.domain(lg)[0:1], k)):
        got = lagrange(lg, tau, 1)
        assert np.array_equal(got, oracle.lagrange_coefficients(lg, tau))
        assert np.array_equal(got, poly.evaluate_all_lagrange_coefficients(n, tau))
    assert np.array_equal(got[k], one()[0]) and int(got.any(axis=1).sum()) == 1


def edge_elements():
    """0, 1, 2, r - 1, r - 2, (r - 1) / 2, (r + 1) / 2 as memory images twice: the plain integer (the residue x / 2^256) and its Montgomery image x * 2^256"""
    r = pyref.R_MOD
    vals = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2]
    return np.concatenate([util.ints_to_fr(vals), util.ints_to_fr_mont(vals)])


def test_edge_operands_every_ordered_pair():
    E = edge_elements()
    k = E.shape[0]
    a, b = np.repeat(E, k, axis=0), np.tile(E, (k, 1))
    c = np.roll(np.repeat(E, k, axis=0), 5, axis=0)
    n = k * k
    da, db, dc, dout = to_dev(a), to_dev(b), to_dev(c), dev_empty(n)
    for op in ("add", "sub", "mul", "mul_sub"):
        want = want_vec_op(op, a, b, c, None)
        assert np.array_equal(vec_op_host(op, a, b, c, None), want), op
        vec_op_dev(op, dout, da, db, dc, None, n)
        assert np.array_equal(from_dev(dout, n), want), op
    _lib.check(L().snarkvm_hip_fr_mul_device(ptr(dout), ptr(da), ptr(db), sz(n)))
    assert np.array_equal(from_dev(dout, n), oracle.fr_op("mul", a, b))
    for i in range(k):  # every element as the broadcast scalar against every element (axpy: against every pair)
        s = E[i : i + 1].copy()
        for op in ("scale", "sub_scalar", "axpy", "rsub_scalar"):
            want = want_vec_op(op, a, b, c, s)
            assert np.array_equal(vec_op_host(op, a, b, c, s), want), (op, i)
            vec_op_dev(op, dout, da, db, dc, s, n)
            assert np.array_equal(from_dev(dout, n), want), (op, i)
    assert np.array_equal(from_dev(da, n), a) and np.array_equal(from_dev(db, n), b) and np.array_equal(from_dev(dc, n), c)


def test_edge_operands_convert_device():
    E = edge_elements()  # every element is below r: a valid residue and a valid canonical integer
    k = E.shape[0]
    want_int, want_mont = oracle.fr_op("to_bigint", E), oracle.fr_op("from_bigint", E)
    for to_bigint, want in ((1, want_int), (0, want_mont)):
        dsrc, dout = to_dev(E), dev_empty(k)
        _lib.check(L().snarkvm_hip_fr_convert_device(ptr(dout), ptr(dsrc), sz(k), to_bigint))
        assert np.array_equal(from_dev(dout, k), want) and np.array_equal(from_dev(dsrc, k), E), to_bigint
        _lib.check(L().snarkvm_hip_fr_convert_device(ptr(dsrc), ptr(dsrc), sz(k), to_bigint))  # in place
        assert np.array_equal(from_dev(dsrc, k), want), to_bigint
    # round trip on the device: from_bigint(to_bigint(x)) == x
    d = to_dev(E)
    _lib.check(L().snarkvm_hip_fr_convert_device(ptr(d), ptr(d), sz(k), 1))
    _lib.check(L().snarkvm_hip_fr_convert_device(ptr(d), ptr(d), sz(k), 0))
    assert np.array_equal(from_dev(d, k), E)
    assert np.array_equal(oracle.fr_op("from_bigint", want_int), E)
