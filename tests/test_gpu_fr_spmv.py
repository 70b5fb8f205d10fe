"""`snarkvm_hip_fr_spmv` on the device (include/snarkvm_hip.h; csrc/poly.hip.h: fr_spmv_seg_kernel, fr_spmv_fix_kernel): the product of a registered
sparse matrix with host and device vectors, batches, refusals, inside a scope between `fr_lagrange_coefficients` and `ntt_device`, and the two
places of the Varuna prover it serves on the committed fixture (snarkvm_amd/matrices.py: z_m, m_at_alpha_evals_device).

Every comparison is bit-exact.  Expected values are Python big-int sums of the oracle's `to_bigint` values (tests/helpers/spmv_cases.py); the host
replay of the kernels (`snarkvm_hip_selftest_fr_spmv`) must give the same bytes as the device.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import cpu as oracle
from snarkvm_amd import _lib, fft, matrices, plugin, poly, synthetic
from snarkvm_amd.devmem import HipMem
from snarkvm_amd.matrices import RegisteredMatrix, SparseMatrix
from tests import util
from tests.helpers import reduce_cases as rc
from tests.helpers import spmv_cases as sc
from tests.test_gpu_fr_lincomb import Arena

pytestmark = pytest.mark.gpu

GUARD = sc.GUARD
SHAPES = ["empty_row", "diagonal", "around_S", "one_long_row", "duplicate_columns", "last_column", "tail", "all_r_minus_1", "raw_r_minus_1"]


def product(reg, x, n_out, on_device):
    """y = M x through snarkvm_hip_fr_spmv; device operands in one block with guards around y, x compared unchanged afterwards"""
    if on_device:
        a = Arena([x], n_out)
        reg.mul_device(a.out, n_out, a.ptr(0))
        return a.result()
    y = np.full((n_out + 1, 4), GUARD, dtype=np.uint64)
    before = x.copy()
    _lib.check(_lib.lib().snarkvm_hip_fr_spmv(y.ctypes.data, n_out, reg.handle, sc.ptr(x), 1, 0, 0, 0))
    assert (y[n_out] == GUARD).all() and np.array_equal(x, before)
    return y[:n_out]


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("name", SHAPES)
def test_shapes(name, on_device):
    m, x, n_out, want = sc.shapes()[name]
    reg = RegisteredMatrix(m)
    assert np.array_equal(product(reg, x, n_out, on_device), want)
    if on_device == 0 and n_out == m.rows:
        assert np.array_equal(reg.mul(x), want)
    reg.close()
    reg.close()  # idempotent


def test_skewed_matrix_and_its_transpose():
    """synthetic.r1cs_like_matrix: short rows and a few long ones; its transpose: one row of a quarter of all rows - against Python and, byte for
    byte, against the host replay of the kernels at the device's own segment size and width"""
    m = SparseMatrix(4099, 4096, *synthetic.r1cs_like_matrix(4099, 4096, 20000, 11))
    t = matrices.transpose(m, 8192, 64)
    S = sc.seg_size()
    assert int(t.row_lengths().max()) > S  # a multi-segment row
    for mat, seed in ((m, 1), (t, 2)):
        x = sc.vector(mat.cols, seed)
        want = sc.expected(mat, x)
        twin = sc.selftest(mat, x, mat.rows, S, 4)
        reg = RegisteredMatrix(mat)
        for on_device in (0, 1):
            got = product(reg, x, mat.rows, on_device)
            assert np.array_equal(got, want), on_device
            assert got.tobytes() == twin.tobytes()
        reg.close()


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
_batch = {}


def _batch_case():
    if not _batch:
        m, _, _, _ = sc.shapes()["tail"]
        xs = [sc.vector(m.cols, 10 + k) for k in range(8)]
        _batch.update(m=m, xs=xs, n_out=m.rows + 3, want=[sc.expected(m, x, m.rows + 3) for x in xs])
    return _batch


@pytest.mark.parametrize("count", [1, 3, 8])
def test_batch(count):
    b = _batch_case()
    m, n_out = b["m"], b["n_out"]
    reg = RegisteredMatrix(m)
    for sx in (0, m.cols, m.cols + 5):
        for sy in (n_out, n_out + 5):
            nx = m.cols if sx == 0 else (count - 1) * sx + m.cols
            ny = (count - 1) * sy + n_out
            host = np.full((1 + nx + 1 + ny + 1, 4), GUARD, dtype=np.uint64)
            x0, y0 = 1, 1 + nx + 1
            for k in range(count if sx else 1):
                host[x0 + k * sx : x0 + k * sx + m.cols] = b["xs"][k]
            mem = HipMem.from_numpy(host)
            reg.mul_device(mem.ptr + 32 * y0, n_out, mem.ptr + 32 * x0, count, sx, sy)
            now = mem.download(dtype=np.uint64).reshape(-1, 4)
            assert np.array_equal(now[:y0], host[:y0]), "x or a guard was written"
            written = np.zeros(len(host), dtype=bool)
            for k in range(count):
                at = y0 + k * sy
                assert np.array_equal(now[at : at + n_out], b["want"][k if sx else 0]), (count, sx, sy, k)
                written[at : at + n_out] = True
            assert (now[y0:][~written[y0:]] == GUARD).all(), "a gap between members or the guard behind y was written"
            mem.free()
    reg.close()


@pytest.mark.parametrize("count", [3, 8])
def test_batch_of_host_operands(count):
    """on_device = 0 with count > 1: x is staged as it lies (members and gaps), y comes back member by member at stride_y - the gaps between the
    members of y and the element behind the last keep their guard value, x is unchanged"""
    b = _batch_case()
    m, n_out = b["m"], b["n_out"]
    reg = RegisteredMatrix(m)
    sy = n_out + 5
    for sx in (0, m.cols + 5):
        nx = m.cols if sx == 0 else (count - 1) * sx + m.cols
        hx = np.full((nx, 4), GUARD, dtype=np.uint64)
        for k in range(count if sx else 1):
            hx[k * sx : k * sx + m.cols] = b["xs"][k]
        before = hx.copy()
        hy = np.full(((count - 1) * sy + n_out + 1, 4), GUARD, dtype=np.uint64)
        _lib.check(_lib.lib().snarkvm_hip_fr_spmv(hy.ctypes.data, n_out, reg.handle, hx.ctypes.data, count, sx, sy, 0))
        assert np.array_equal(hx, before)
        written = np.zeros(len(hy), dtype=bool)
        for k in range(count):
            assert np.array_equal(hy[k * sy : k * sy + n_out], b["want"][k if sx else 0]), (count, sx, k)
            written[k * sy : k * sy + n_out] = True
        assert (hy[~written] == GUARD).all(), "a gap between members or the guard behind y was written"
    reg.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(_lib.HipError) as e:
        fn()
    assert e.value.code == sc.INVALID_VALUE and e.value.message, e.value


def test_refusals_leave_y_untouched():
    m, x, _, _ = sc.shapes()["tail"]
    reg = RegisteredMatrix(m)
    L = _lib.lib()
    n_out = m.rows + 2
    cells = 4 * (n_out + 5) + m.cols
    host = np.full((cells, 4), GUARD, dtype=np.uint64)
    host[: m.cols] = x
    mem = HipMem.from_numpy(host)
    d_x, d_y = mem.ptr, mem.ptr + 32 * m.cols

    def spmv(y=d_y, n=n_out, handle=reg.handle, xp=d_x, count=1, sx=0, sy=0, on_device=1):
        return lambda: _lib.check(L.snarkvm_hip_fr_spmv(rc.ptr(y), n, rc.ptr(handle), rc.ptr(xp), count, sx, sy, on_device))

    _refused(spmv(handle=0))
    _refused(spmv(n=m.rows - 1))
    _refused(spmv(n=(1 << 28) + 1))
    _refused(spmv(count=2, sx=m.cols - 1, sy=n_out))
    _refused(spmv(count=2, sx=m.cols, sy=n_out - 1))
    _refused(spmv(count=2, sx=0, sy=n_out - 1))
    _refused(spmv(count=65536, sx=0, sy=n_out))
    _refused(spmv(count=2, sx=0, sy=(1 << 40) + 1))  # strides whose spans could wrap
    _refused(spmv(count=2, sx=(1 << 64) - 32, sy=n_out))
    _refused(spmv(y=0))
    _refused(spmv(xp=0))
    # y overlapping x: y starts inside x, x starts inside y, y == x, and the second member of a batch reaching into x
    _refused(spmv(y=d_x + 32 * (m.cols - 1)))
    _refused(spmv(y=d_x))
    _refused(spmv(y=d_y, xp=d_y + 32 * (n_out - 1)))
    _refused(spmv(y=d_y, xp=d_y + 32 * (n_out + 2), count=2, sx=0, sy=n_out + 2))
    # operands that do not live on one device: a host vector beside a device vector
    hx = x.copy()
    _refused(spmv(xp=hx.ctypes.data))
    hy = np.full((n_out, 4), GUARD, dtype=np.uint64)
    _refused(spmv(y=hy.ctypes.data, n=m.rows - 1, xp=hx.ctypes.data, on_device=0))
    assert (hy == GUARD).all()
    assert np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), host), "a refused call wrote device memory"
    # count == 0 and an empty product: success, nothing touched
    _lib.check(L.snarkvm_hip_fr_spmv(rc.ptr(d_y), n_out, rc.ptr(reg.handle), rc.ptr(d_x), 0, 0, 0, 1))
    empty = RegisteredMatrix(SparseMatrix(0, 4, [0], [], np.zeros((0, 4), dtype=np.uint64)))
    _lib.check(L.snarkvm_hip_fr_spmv(None, 0, rc.ptr(empty.handle), None, 1, 0, 0, 1))
    assert np.array_equal(mem.download(dtype=np.uint64).reshape(-1, 4), host)
    # no rows at all: the whole of y is tail
    empty.mul_device(d_y, 3, d_x)
    now = mem.download(dtype=np.uint64).reshape(-1, 4)
    assert not now[m.cols : m.cols + 3].any() and np.array_equal(now[m.cols + 3 :], host[m.cols + 3 :]) and np.array_equal(now[: m.cols], x)
    empty.close()
    reg.close()
    mem.free()


# ---- inside a scope ----------------------------------------------------------------------------------------------------------------------------
def test_inside_a_scope_between_lagrange_coefficients_and_a_transform():
    """fr_lagrange_coefficients -> fr_spmv -> ntt_device (inverse) enqueued in one scope: the result is the oracle's transform of the Python
    product; the same calls outside a scope give the same bytes; a repeat grows no workspace; a handle freed right after scope_end, and one freed
    before it, both leave a correct result"""
    lg = 12
    n = 1 << lg
    m = SparseMatrix(n - 95, n, *synthetic.r1cs_like_matrix(n - 95, n, 9000, 5))
    tau = rc.rnd(3, 2)[2:3].copy()
    want = oracle.ntt(sc.expected(m, oracle.lagrange_coefficients(lg, tau), n), direction=oracle.INVERSE)
    L = _lib.lib()
    regs = [RegisteredMatrix(m) for _ in range(3)]
    mem = HipMem.from_numpy(np.full((2 * n + 3, 4), GUARD, dtype=np.uint64))
    d_l, d_y = mem.ptr + 32, mem.ptr + 32 * (n + 2)
    stats = np.zeros(5, dtype=np.uint64)
    results = []
    for attempt, reg in enumerate(regs):
        mem.fill(32 * (n + 2), 0x5A, 32 * n)
        in_scope = attempt < 2
        if in_scope:
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(mem.ptr)))
        try:
            _lib.check(L.snarkvm_hip_fr_lagrange_coefficients(ctypes.c_void_p(d_l), ctypes.c_uint32(lg), ctypes.c_void_p(tau.ctypes.data), ctypes.c_int(1)))
            reg.mul_device(d_y, n, d_l)
            _lib.check(L.snarkvm_hip_ntt_device(ctypes.c_void_p(d_y), lg, 0, 1, 0))
            if attempt == 1:
                reg.close()  # before the scope ends: the release waits for the enqueued product
        finally:
            if in_scope:
                _lib.check(L.snarkvm_hip_scope_end())
        reg.close()  # (attempt 0: right after scope_end)
        if attempt == 0:
            L.snarkvm_hip_alloc_stats(None, 1)
        elif attempt == 1:
            L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
        now = mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[n + 2 : 2 * n + 2], want), attempt
        assert np.array_equal(now[1 : n + 1], oracle.lagrange_coefficients(lg, tau)), attempt
        assert (now[0] == GUARD).all() and (now[n + 1] == GUARD).all() and (now[2 * n + 2] == GUARD).all()
        results.append(now[n + 2 : 2 * n + 2].tobytes())
    assert results[0] == results[1] == results[2]
    assert not stats[:4].any(), stats
    mem.free()


def test_a_repeated_host_call_grows_no_workspace():
    m, x, n_out, want = sc.shapes()["around_S"]
    reg = RegisteredMatrix(m)
    L = _lib.lib()
    reg.mul(x)
    L.snarkvm_hip_alloc_stats(None, 1)
    got = reg.mul(x)
    stats = np.zeros(5, dtype=np.uint64)
    L.snarkvm_hip_alloc_stats(ctypes.c_void_p(stats.ctypes.data), 0)
    assert not stats[:4].any(), stats
    assert np.array_equal(got, want)
    reg.close()


# ---- known answers held by the reference (tests/golden/varuna_circuit0.json) ---------------------------------------------------------------
def _fixture(golden):
    tv = golden["varuna"]
    ms = {k: SparseMatrix.from_rows([[(v, j) for j, v in enumerate(row) if v] for row in tv["instance"][k]], 7) for k in "ABC"}
    w = util.ints_to_fr_mont([int(v) for v in tv["witness"][1]])
    return tv, ms, w[:4], w[4:]


def test_z_m_of_the_fixture_and_the_h_0_chain(golden):
    """z_A, z_B, z_C by the device product, zero-padded to the domain, then iNTT * iNTT - iNTT over X^8 - 1 with the existing passes: h_0.txt"""
    tv, ms, public, private = _fixture(golden)
    want = {"A": [2, 2, 2, 2, 2, 8, 32, 0], "B": [4] * 7 + [0], "C": [8, 8, 8, 8, 8, 32, 128, 0]}
    coeffs = {}
    for k, m in ms.items():
        reg = RegisteredMatrix(m)
        z = matrices.z_m(reg, public, private, 8)
        assert util.fr_mont_to_ints(z) == want[k], k
        # the same on device memory, straight into the inverse transform
        mem = HipMem.from_numpy(np.concatenate([public, private, np.full((9, 4), GUARD, dtype=np.uint64)]))
        reg.mul_device(mem.ptr + 32 * 7, 8, mem.ptr)
        _lib.check(_lib.lib().snarkvm_hip_ntt_device(ctypes.c_void_p(mem.ptr + 32 * 7), 3, 0, 1, 0))
        now = mem.download(dtype=np.uint64).reshape(-1, 4)
        assert (now[15] == GUARD).all() and np.array_equal(now[:7], np.concatenate([public, private]))
        coeffs[k] = now[7:15].copy()
        assert np.array_equal(coeffs[k], oracle.ntt(util.ints_to_fr_mont(want[k]), direction=oracle.INVERSE))
        reg.close()
        mem.free()
    mul = fft.PolyMultiplier()
    mul.add_polynomial(poly.trim(coeffs["A"]), "z_a")
    mul.add_polynomial(poly.trim(coeffs["B"]), "z_b")
    rowcheck = mul.multiply()
    cpad = np.zeros_like(rowcheck)
    cpad[:8] = coeffs["C"][: rowcheck.shape[0]]
    q, r = poly.divide_by_vanishing_poly(poly.vec_op("sub", rowcheck, cpad), 8)
    assert r.shape[0] == 0
    assert util.fr_mont_to_ints(q) == [int(v) for v in tv["polynomials"]["h_0"]]


def test_m_at_alpha_of_the_fixture_three_routes(golden):
    """<M^T l_alpha, z> == <l_alpha, M z> == (iNTT(M z))(alpha) for M in {A, B, C}, z at its variable-domain places and alpha the first challenge"""
    tv, ms, public, private = _fixture(golden)
    alpha = util.ints_to_fr_mont([int(tv["challenges"].split()[0])])
    z_placed = util.ints_to_fr_mont([1, 2, 8, 4, 32, 2, 128, 0])
    l_alpha = oracle.lagrange_coefficients(3, alpha)
    for k, m in ms.items():
        t = RegisteredMatrix(matrices.transpose(m, 8, 4))
        mem = HipMem.from_numpy(np.concatenate([z_placed, np.full((19, 4), GUARD, dtype=np.uint64)]))
        d_z, d_l, d_out = mem.ptr, mem.ptr + 32 * 9, mem.ptr + 32 * 18
        matrices.m_at_alpha_evals_device(t, 3, alpha, d_out, d_l)
        first = plugin.fr_reduce_device(plugin.FR_REDUCE_DOT, d_out, d_z, 8)
        now = mem.download(dtype=np.uint64).reshape(-1, 4)
        assert np.array_equal(now[9:17], l_alpha) and (now[8] == GUARD).all() and (now[17] == GUARD).all() and (now[26] == GUARD).all()
        assert np.array_equal(now[18:26], sc.expected(matrices.transpose(m, 8, 4), l_alpha[:7])), k  # 7 constraints in a domain of 8
        reg = RegisteredMatrix(m)
        z_m = matrices.z_m(reg, public, private, 8)
        second = rc.expected(rc.DOT, l_alpha, z_m)
        third = oracle.poly_evaluate(oracle.ntt(z_m, direction=oracle.INVERSE), alpha)
        assert np.array_equal(first, second) and np.array_equal(first, third), k
        assert first.any()
        for h in (t, reg):
            h.close()
        mem.free()


# ---- the credits.aleo/transfer_private shape -------------------------------------------------------------------------------------------------
SAMPLE_SEED = 0x5A3B1E


def _sample_rows(rows):
    """4096 distinct row indices below `rows` from SAMPLE_SEED: x <- (x * 6364136223846793005 + 1442695040888963407) mod 2^64, index = (x >> 33) % rows,
    repeats skipped.  The same indices are LISTED in tests/golden/fr_spmv_sample_rows.json; the test compares the two."""
    x, seen, out = SAMPLE_SEED, set(), []
    while len(out) < 4096:
        x = (x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        i = (x >> 33) % rows
        if i not in seen:
            seen.add(i)
            out.append(i)
    return out


@pytest.mark.parametrize("transposed", [False, True])
def test_transfer_private_shape(transposed):
    rows, cols, nnz = 51002, 1 << 16, 111472
    m = SparseMatrix(rows, cols, *synthetic.r1cs_like_matrix(rows, cols, nnz, 0x7A))
    if transposed:
        m = matrices.transpose(m, 1 << 16, 1 << 8)
    n_out = 1 << 16
    x = sc.vector(m.cols, 4)
    with open(os.path.join(util.ROOT, "tests", "golden", "fr_spmv_sample_rows.json")) as f:
        listed = json.load(f)[str(m.rows)]
    assert listed == _sample_rows(m.rows) and len(set(listed)) == 4096
    sample = set(listed)
    sample |= set(np.flatnonzero(m.row_lengths() > sc.seg_size()).tolist())
    assert len(sample) > 4096 or not transposed  # the transpose has multi-segment rows
    sample = sorted(sample)
    reg = RegisteredMatrix(m)
    got = product(reg, x, n_out, 1)
    reg.close()
    assert np.array_equal(got[sample], sc.expected(m, x, only_rows=sample))
    assert not got[m.rows :].any()
    empty = np.flatnonzero(m.row_lengths() == 0)
    assert not got[empty].any()
