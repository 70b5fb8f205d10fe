"""Cases and expected values shared by tests/test_fr_spmv_host.py (CPU) and tests/test_gpu_fr_spmv.py: the matrices and vectors of
`snarkvm_hip_fr_spmv` and what every result is compared with, bit for bit.

Expected values do not come from the library: `oracle.fr_op("to_bigint")` turns values and vector into Python ints, every row's sum of products
is taken mod r in Python, and `oracle.fr_op("from_bigint")` gives the memory form back (the route of tests/helpers/reduce_cases.py).  Boundary
shapes are derived from the segment size S that `snarkvm_hip_selftest_fr_spmv_geometry` reports, not hard-coded.
"""
import ctypes
import functools

import numpy as np

from oracle import cpu as oracle
from snarkvm_amd import _lib
from snarkvm_amd.matrices import SparseMatrix
from tests import util
from tests.helpers import reduce_cases as rc

R = rc.R
GUARD = rc.GUARD
INVALID_VALUE = 1  # hipErrorInvalidValue
WIDTHS = (4, 8, 16, 64)


def geometry(rows, nnz):
    """{S, width, threads, nseg} of what registration lays out for a uniform matrix (snarkvm_hip_selftest_fr_spmv_geometry)"""
    out = np.zeros(4, dtype=np.uint32)
    assert _lib.lib().snarkvm_hip_selftest_fr_spmv_geometry(rows, nnz, out.ctypes.data) == 0
    return dict(zip(("S", "width", "threads", "nseg"), (int(x) for x in out)))


def seg_size():
    return geometry(1, 1)["S"]


def expected(m, x, n_out=None, only_rows=None):
    """M x by Python big ints -> (n_out, 4) memory form, zero behind the rows; only_rows: just those rows -> (len(only_rows), 4)"""
    vals, xs = rc.to_ints(m.vals), rc.to_ints(x)
    assert len(xs) == m.cols
    rp, ci = m.row_ptr.tolist(), m.col_idx.tolist()
    rows = range(m.rows) if only_rows is None else only_rows
    sums = [sum(vals[k] * xs[ci[k]] for k in range(rp[r], rp[r + 1])) % R for r in rows]
    if only_rows is not None:
        return oracle.fr_op("from_bigint", util.ints_to_fr(sums)) if sums else np.zeros((0, 4), dtype=np.uint64)
    n_out = m.rows if n_out is None else n_out
    y = np.zeros((n_out, 4), dtype=np.uint64)
    if sums:
        y[: m.rows] = oracle.fr_op("from_bigint", util.ints_to_fr(sums))
    return y


def from_lengths(lens, cols, seed, col_of=None, kind="mixed"):
    """a matrix with the given row lengths; columns (k * 7 + seed) % cols unless col_of(k) says otherwise; values `mixed` (random with the
    special values 0, 1, 2, r-1, r-2, (r+-1)/2 at every fifth place), `max` (all r - 1) or `rawmax` (memory images the integer r - 1)"""
    nnz = int(sum(lens))
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    col = np.array([(k * 7 + seed) % cols if col_of is None else col_of(k) for k in range(nnz)], dtype=np.uint32)
    if kind == "mixed":
        vals = rc.mixed(nnz, seed)
    else:
        vals = rc.max_terms(nnz, kind)[0]
    return SparseMatrix(len(lens), cols, row_ptr, col, vals)


def vector(cols, seed, kind="mixed"):
    return rc.mixed(cols, seed) if kind == "mixed" else rc.max_terms(cols, kind)[0]


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (matrix, x, n_out, expected y); computed once and shared - nothing may write into them"""
    S = seg_size()
    cases = {}

    def add(name, m, kind="mixed", n_out=None, seed=3):
        x = vector(m.cols, seed, kind)
        n_out = m.rows if n_out is None else n_out
        want = expected(m, x, n_out)
        for a in (m.row_ptr, m.col_idx, m.vals, x, want):
            a.setflags(write=False)
        cases[name] = (m, x, n_out, want)

    add("empty_row", from_lengths([0], 3, 1))
    add("diagonal", from_lengths([1] * 37, 37, 0, col_of=lambda k: k))
    add("around_S", from_lengths([S - 1, S, S + 1, 3 * S + 1], 50, 2))
    add("one_long_row", from_lengths([0] * 150 + [5 * S + 7] + [0] * 150, 97, 4))
    add("duplicate_columns", from_lengths([9, 2], 5, 5, col_of=lambda k: (3, 3, 1, 3, 0, 1, 3, 3, 4, 2, 2)[k]))
    add("last_column", from_lengths([1, 0, S + 2, 3], 11, 6, col_of=lambda k: 10))
    add("tail", from_lengths([2, 0, S + 1, 1, 0], 13, 7), n_out=5 + 5)
    add("all_r_minus_1", from_lengths([1, S, 2 * S + 3, 0, 5], 19, 8, kind="max"), kind="max")
    add("raw_r_minus_1", from_lengths([1, S, 2 * S + 3, 0, 5], 19, 8, kind="rawmax"), kind="rawmax")
    return cases


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def register(m):
    """snarkvm_hip_fr_matrix_register -> (error, handle address or 0)"""
    h = ctypes.c_void_p(0xDEAD)
    err = _lib.lib().snarkvm_hip_fr_matrix_register(ctypes.byref(h), m.rows, m.cols, m.row_ptr.ctypes.data, ptr(m.col_idx), ptr(m.vals))
    return err, h.value or 0


def selftest(m, x, n_out, seg, width):
    """snarkvm_hip_selftest_fr_spmv -> (n_out, 4); the element behind the result is a guard"""
    out = np.full((n_out + 1, 4), GUARD, dtype=np.uint64)
    assert _lib.lib().snarkvm_hip_selftest_fr_spmv(out.ctypes.data, n_out, m.rows, m.cols, m.row_ptr.ctypes.data, ptr(m.col_idx), ptr(m.vals), ptr(x), seg, width) == 0
    assert (out[n_out] == GUARD).all()
    return out[:n_out]
