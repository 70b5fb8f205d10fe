"""`snarkvm_hip_fr_spmv` without a GPU (include/snarkvm_hip.h): the segmentation of `snarkvm_hip_fr_matrix_register`, the per-lane accumulation of
fr_spmv_seg_kernel (csrc/poly.hip.h: fr_spmv_lane over Fp::sum_of_products), the butterfly, the partials and the fix-up launch run on the CPU through
`snarkvm_hip_selftest_fr_spmv` for a given segment size and lane-group width.  Every comparison is bit-exact against Python big-int sums of the
oracle's `to_bigint` values (tests/helpers/spmv_cases.py); since field addition is exact, every (segment size, width) pair must give the same bytes.
Registration refusals need no device; the host side of snarkvm_amd/matrices.py is checked on the committed Varuna fixture.
"""
import ctypes

import numpy as np
import pytest

from snarkvm_amd import _lib, matrices, synthetic
from snarkvm_amd.matrices import SparseMatrix
from tests import util
from tests.helpers import spmv_cases as sc

SHAPES = ["empty_row", "diagonal", "around_S", "one_long_row", "duplicate_columns", "last_column", "tail", "all_r_minus_1", "raw_r_minus_1"]


def _refused(err):
    with pytest.raises(_lib.HipError) as e:
        _lib.check(err)
    assert e.value.code == sc.INVALID_VALUE and e.value.message, e.value


def test_the_case_list_is_complete():
    assert sorted(sc.shapes()) == sorted(SHAPES)


@pytest.mark.parametrize("name", SHAPES)
def test_host_twin_matches_python_for_every_segment_size_and_width(name):
    m, x, n_out, want = sc.shapes()[name]
    S = sc.seg_size()
    for seg in (1, 3, S):
        for width in (4, 64):
            assert np.array_equal(sc.selftest(m, x, n_out, seg, width), want), (name, seg, width)


def test_geometry_hook():
    g = sc.geometry(1, 1)
    S = g["S"]
    assert S >= 1 and g["width"] in sc.WIDTHS and g["threads"] % 64 == 0 and g["threads"] % g["width"] == 0 and g["nseg"] == 1
    assert sc.geometry(1, S)["nseg"] == 1 and sc.geometry(1, S + 1)["nseg"] == 2 and sc.geometry(1, 5 * S + 7)["nseg"] == 6
    assert sc.geometry(10, 25)["nseg"] == 10 and sc.geometry(10, 5)["nseg"] == 5 and sc.geometry(10, 0)["nseg"] == 0
    assert sc.geometry(1000, 2000)["width"] == 4      # short rows: the narrowest group
    assert sc.geometry(1, 64 * S)["width"] == (64 if S > 64 else sc.geometry(1, S)["width"])  # full segments of more than 64 entries: a whole wave
    assert _lib.lib().snarkvm_hip_selftest_fr_spmv_geometry(0, 5, np.zeros(4, dtype=np.uint32).ctypes.data) == -1
    assert _lib.lib().snarkvm_hip_selftest_fr_spmv_geometry(1, 1, None) == -1


def test_skewed_matrix_and_its_transpose_on_the_host_twin():
    """the synthetic R1CS-like matrix at a small shape: its transpose has one row of about a quarter of the rows"""
    m = SparseMatrix(4099, 4096, *synthetic.r1cs_like_matrix(4099, 4096, 20000, 11))
    t = matrices.transpose(m, 8192, 64)
    assert t.rows == 8192 and t.cols == 4099 and t.nnz == m.nnz and int(t.row_lengths().max()) > 4099 // 5
    S = sc.seg_size()
    for mat, seed in ((m, 1), (t, 2)):
        x = sc.vector(mat.cols, seed)
        want = sc.expected(mat, x)
        assert np.array_equal(sc.selftest(mat, x, mat.rows, S, 4), want)
        assert np.array_equal(sc.selftest(mat, x, mat.rows, 64, 16), want)


def test_r1cs_like_matrix_has_the_stated_shape():
    rows, cols, nnz = 4099, 4096, 20000
    a = synthetic.r1cs_like_matrix(rows, cols, nnz, 11)
    b = synthetic.r1cs_like_matrix(rows, cols, nnz, 11)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))  # deterministic
    row_ptr, col_idx, vals = a
    lens = np.diff(row_ptr.astype(np.int64))
    assert int(row_ptr[-1]) == nnz == len(col_idx) == len(vals) and int(col_idx.max()) < cols
    long_rows = lens > 4
    assert int(long_rows.sum()) == rows // 100 and int(lens.max()) <= 4096 and abs(int(lens[long_rows].sum()) - nnz // 4) < nnz // 20
    assert ((lens[~long_rows] >= 1) & (lens[~long_rows] <= 4)).all()
    with_zero = np.array([(col_idx[int(row_ptr[r]) : int(row_ptr[r + 1])] == 0).any() for r in range(rows)])
    assert 0.2 < with_zero.mean() < 0.3
    assert 0.2 < (vals == synthetic.FR_ONE_MONT).all(axis=1).mean() < 0.3
    assert synthetic.FR_ONE_MONT.tolist() == util.ints_to_fr_mont([1])[0].tolist()


def test_selftest_refuses_bad_arguments():
    m, x, n_out, _ = sc.shapes()["around_S"]
    L = _lib.lib()
    out = np.full((n_out + 1, 4), sc.GUARD, dtype=np.uint64)

    def call(n=n_out, rows=m.rows, cols=m.cols, rp=m.row_ptr, ci=m.col_idx, seg=3, width=4, y=out):
        return L.snarkvm_hip_selftest_fr_spmv(sc.ptr(y), n, rows, cols, sc.ptr(rp), sc.ptr(ci), sc.ptr(m.vals), sc.ptr(x), seg, width)

    assert call(seg=0) == -1
    for width in (0, 1, 2, 5, 32, 128):
        assert call(width=width) == -1
    assert call(n=m.rows - 1) == -1
    assert call(n=(1 << 28) + 1) == -1
    assert call(cols=int(m.col_idx.max())) == -1  # a column index == cols
    assert call(rp=None) == -1 and call(ci=None) == -1 and call(y=None) == -1
    assert (out == sc.GUARD).all()
    assert call() == 0


# ---- registration: every refusal comes from snarkvm_hip_fr_matrix_register itself, with no device present ---------------------------------
def _register(rows, cols, row_ptr, col_idx, vals, handle="fresh"):
    h = ctypes.c_void_p(0xDEAD)
    rp = None if row_ptr is None else np.ascontiguousarray(row_ptr, dtype=np.uint64)
    ci = None if col_idx is None else np.ascontiguousarray(col_idx, dtype=np.uint32)
    err = _lib.lib().snarkvm_hip_fr_matrix_register(None if handle is None else ctypes.byref(h), rows, cols, sc.ptr(rp) if rp is not None else None,
                                                    sc.ptr(ci) if ci is not None else None, sc.ptr(vals) if vals is not None else None)
    return err, h.value


def test_registration_refusals_need_no_device():
    vals = sc.vector(4, 1)
    good = (2, 3, [0, 1, 4], [0, 1, 2, 1])
    cases = {
        "null handle": (*good, vals, None),
        "null row_ptr": (2, 3, None, [0, 1, 2, 1], vals),
        "null col_idx": (2, 3, [0, 1, 4], None, vals),
        "null vals": (*good, None),
        "row_ptr[0] != 0": (2, 3, [1, 1, 4], [0, 1, 2, 1], vals),
        "decreasing row_ptr": (3, 3, [0, 3, 2, 4], [0, 1, 2, 1], vals),
        "too many entries": (1, 3, [0, 1 << 32], [0], vals),
        "too many rows": ((1 << 28) + 1, 3, [0, 0], [0], vals),  # refused before row_ptr is walked
        "too many cols": (2, (1 << 28) + 1, [0, 1, 4], [0, 1, 2, 1], vals),
        "col_idx == cols": (2, 3, [0, 1, 4], [0, 1, 3, 1], vals),
        "col_idx == cols in the last entry": (2, 3, [0, 1, 4], [0, 1, 2, 3], vals),
    }
    for name, args in cases.items():
        err, h = _register(*args)
        _refused(err)
        if args[-1] is not None or len(args) == 5:
            assert h is None, name  # the handle is NULL after a refusal


def test_product_refusals_that_need_no_device():
    L = _lib.lib()
    y = np.full((4, 4), sc.GUARD, dtype=np.uint64)
    x = sc.vector(3, 1)
    for on_device in (0, 1):
        _refused(L.snarkvm_hip_fr_spmv(y.ctypes.data, 4, None, x.ctypes.data, 1, 0, 0, on_device))  # a NULL handle
        _refused(L.snarkvm_hip_fr_spmv(y.ctypes.data, 0, None, x.ctypes.data, 0, 0, 0, on_device))
    assert (y == sc.GUARD).all()
    L.snarkvm_hip_fr_matrix_free(None)  # a no-op


# ---- snarkvm_amd/matrices.py on the committed fixture ----------------------------------------------------------------------------------------
def _fixture_matrices(golden):
    inst = golden["varuna"]["instance"]
    return {k: SparseMatrix.from_rows([[(v, j) for j, v in enumerate(row) if v] for row in inst[k]], 7) for k in "ABC"}


def test_reindex_by_subdomain_on_the_fixture(golden):
    variables = [int(v) for v in golden["varuna"]["witness"][1]]
    assert variables == [1, 8, 32, 128, 2, 4, 2]
    placed = [0] * 8
    for i, v in enumerate(variables):
        placed[matrices.reindex_by_subdomain(8, 4, i)] = v
    assert placed == [1, 2, 8, 4, 32, 2, 128, 0]  # the vector of KAT-iNTT_8
    assert sorted(matrices.reindex_by_subdomain(8, 4, i) for i in range(8)) == list(range(8))
    assert [matrices.reindex_by_subdomain(16, 4, i) for i in range(16)] == [0, 4, 8, 12, 1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15]
    for big, small in ((8, 8), (4, 8)):
        with pytest.raises(ValueError):
            matrices.reindex_by_subdomain(big, small, 0)
    with pytest.raises(ValueError):
        matrices.transpose(_fixture_matrices(golden)["A"], 4, 4)


def test_transpose_on_the_fixture(golden):
    ms = _fixture_matrices(golden)
    want = {"A": [0, 5, 1, 0, 1, 0, 0, 0], "B": [0, 0, 0, 7, 0, 0, 0, 0], "C": [0, 0, 5, 0, 1, 0, 1, 0]}
    one = util.ints_to_fr_mont([1])[0]
    for k, m in ms.items():
        assert m.rows == 7 and m.cols == 7 and (m.vals == one).all()
        t = matrices.transpose(m, 8, 4)
        assert (t.rows, t.cols, t.nnz) == (8, 7, m.nnz)
        assert t.row_lengths().tolist() == want[k], k
        for r in range(8):  # increasing original-row order inside a transposed row
            cols = t.col_idx[int(t.row_ptr[r]) : int(t.row_ptr[r + 1])].tolist()
            assert cols == sorted(cols)
        # the same entries: (row, reindexed column) pairs
        src = sorted((r, matrices.reindex_by_subdomain(8, 4, int(c))) for r in range(7) for c in m.col_idx[int(m.row_ptr[r]) : int(m.row_ptr[r + 1])])
        dst = sorted((int(c), r) for r in range(8) for c in t.col_idx[int(t.row_ptr[r]) : int(t.row_ptr[r + 1])])
        assert src == dst


def test_from_rows_takes_ints_and_limbs():
    limbs = util.ints_to_fr_mont([5])[0]
    m = SparseMatrix.from_rows([[(5, 2), (limbs, 0)], [], [(-1, 1)]], 3)
    assert m.row_ptr.tolist() == [0, 2, 2, 3] and m.col_idx.tolist() == [2, 0, 1]
    assert np.array_equal(m.vals, util.ints_to_fr_mont([5, 5, sc.R - 1]))
    with pytest.raises(ValueError):
        SparseMatrix.from_rows([[(1, 3)]], 3)
