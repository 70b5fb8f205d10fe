"""The sparse side of the Varuna prover on the gfx950 backend: an R1CS matrix (`Matrix<F>` = a list of rows of `(value, column)`,
algorithms/src/snark/varuna/ahp/matrices.rs) registered once in device memory and multiplied with vectors that live there.

    z_M = M z for M in {A, B, C}            snark/varuna/ahp/prover/round_functions/mod.rs:131-188 (`inner_product` over every row)
    M(alpha, .) = M^T l_alpha               snark/varuna/ahp/prover/round_functions/third.rs:303-306, with the transpose of ahp/matrices.rs:250-264

The transpose is circuit data like the matrix itself: built once on the host (`transpose`) and registered; the product is
`snarkvm_hip_fr_spmv` (include/snarkvm_hip.h).  Nothing here builds a circuit index or drives a prover round.
"""
import ctypes

import numpy as np

from . import _lib, plugin

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041
_MONT_R = (1 << 256) % R_MOD
_MASK = (1 << 64) - 1


def _fr_mont(value):
    v = int(value) % R_MOD * _MONT_R % R_MOD
    return (v & _MASK, (v >> 64) & _MASK, (v >> 128) & _MASK, v >> 192)


class SparseMatrix:
    """CSR arrays of a `rows` x `cols` matrix over Fr: row r owns entries row_ptr[r] .. row_ptr[r + 1] - 1, entry k is vals[k] ((nnz, 4) uint64,
    Montgomery memory form) at column col_idx[k]."""

    def __init__(self, rows, cols, row_ptr, col_idx, vals):
        self.rows, self.cols = int(rows), int(cols)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64).reshape(-1)
        self.col_idx = np.ascontiguousarray(col_idx, dtype=np.uint32).reshape(-1)
        self.vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
        if self.row_ptr.shape[0] != self.rows + 1 or self.col_idx.shape[0] != self.vals.shape[0] or int(self.row_ptr[-1]) != self.vals.shape[0]:
            raise ValueError("SparseMatrix: row_ptr, col_idx and vals do not describe one matrix")

    @property
    def nnz(self):
        return self.vals.shape[0]

    @classmethod
    def from_rows(cls, rows, num_cols):
        """The reference's `Matrix<F>`: a list of rows, each a list of `(value, column)`.  A value is a Python int (any residue) or a 4-limb
        element already in Montgomery memory form."""
        row_ptr, cols, vals = [0], [], []
        for row in rows:
            for value, column in row:
                vals.append(_fr_mont(value) if isinstance(value, (int, np.integer)) else tuple(int(l) for l in value))
                cols.append(int(column))
            row_ptr.append(len(cols))
        if cols and (min(cols) < 0 or max(cols) >= num_cols):
            raise ValueError("SparseMatrix.from_rows: a column index is outside the matrix")
        return cls(len(rows), num_cols, row_ptr, cols, np.array(vals, dtype=np.uint64).reshape(-1, 4))

    def row_lengths(self):
        return np.diff(self.row_ptr.astype(np.int64))


def _check_subdomain(domain_size, sub_size):
    if domain_size <= sub_size:
        raise ValueError("other.size() must be smaller than self.size()")  # fft/domain.rs:323


def reindex_by_subdomain(domain_size, sub_size, index):
    """`EvaluationDomain::reindex_by_subdomain` (fft/domain.rs:322-344): the index in the domain of `domain_size` elements of element `index`
    counted through the subdomain of `sub_size` elements first and the rest of the domain afterwards."""
    _check_subdomain(domain_size, sub_size)
    period = domain_size // sub_size
    if index < sub_size:
        return index * period
    i = index - sub_size
    return i + i // (period - 1) + 1


def _reindex_all(domain_size, sub_size, index):
    _check_subdomain(domain_size, sub_size)
    index = np.asarray(index, dtype=np.int64)
    period = domain_size // sub_size
    i = index - sub_size
    return np.where(index < sub_size, index * period, i + i // (period - 1) + 1)


def transpose(matrix, variable_domain_size, input_domain_size):
    """`transpose` of ahp/matrices.rs:250-264: entry (value, column) of row r becomes entry (value, r) of row
    reindex_by_subdomain(column) of a matrix of variable_domain_size rows; the entries of a transposed row are in increasing original-row
    order, as the reference pushes them."""
    at = _reindex_all(variable_domain_size, input_domain_size, matrix.col_idx)
    if at.size and int(at.max()) >= variable_domain_size:
        raise ValueError("transpose: a variable does not fit the variable domain")
    order = np.argsort(at, kind="stable")  # CSR order is row-major, so a stable sort keeps the rows increasing inside a column
    src_row = np.repeat(np.arange(matrix.rows, dtype=np.int64), matrix.row_lengths())
    row_ptr = np.zeros(variable_domain_size + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum(np.bincount(at, minlength=variable_domain_size)).astype(np.uint64)
    return SparseMatrix(variable_domain_size, matrix.rows, row_ptr, src_row[order].astype(np.uint32), matrix.vals[order])


class RegisteredMatrix:
    """A SparseMatrix resident in device memory (`snarkvm_hip_fr_matrix_register`: entries and work layout on every device in use), for as many
    products as the proving key lives.  close() - also run when the object dies - releases it; that is safe while a scope of the calling thread
    still has a product enqueued (the release waits for the device)."""

    def __init__(self, matrix):
        self.rows, self.cols, self.nnz = matrix.rows, matrix.cols, matrix.nnz
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().snarkvm_hip_fr_matrix_register(ctypes.byref(h), matrix.rows, matrix.cols, matrix.row_ptr.ctypes.data,
                                                             matrix.col_idx.ctypes.data if matrix.nnz else None, matrix.vals.ctypes.data if matrix.nnz else None))
        self.handle = h.value or 0

    def mul(self, x, n_out=None):
        """y = M x on host arrays: x (cols, 4) -> y (n_out, 4), n_out >= rows (default rows), the tail zero."""
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
        if x.shape[0] != self.cols:
            raise ValueError(f"RegisteredMatrix.mul: x has {x.shape[0]} elements, the matrix {self.cols} columns")
        n_out = self.rows if n_out is None else int(n_out)
        y = np.zeros((n_out, 4), dtype=np.uint64)
        _lib.check(_lib.lib().snarkvm_hip_fr_spmv(y.ctypes.data if n_out else None, n_out, self.handle, x.ctypes.data if self.cols else None, 1, 0, 0, 0))
        return y

    def mul_device(self, d_y, n_out, d_x, count=1, stride_x=0, stride_y=0):
        """y = M x on device vectors (plugin.fr_spmv_device); inside a scope only enqueued."""
        plugin.fr_spmv_device(self.handle, _dev_ptr(d_y), n_out, _dev_ptr(d_x), count, stride_x, stride_y)

    def close(self):
        if self.handle:
            h, self.handle = self.handle, 0
            _lib.lib().snarkvm_hip_fr_matrix_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown / a dead device: nothing left to do
            pass


def _dev_ptr(x):
    return int(getattr(x, "ptr", x))


def z_m(reg, padded_public, private, n_out=None):
    """z_M: the `inner_product` of round_functions/mod.rs:169-188 over every row of the registered matrix - variable i is
    padded_public[i] below the number of public variables and private[i - that] above, i.e. x is simply public ++ private."""
    z = np.concatenate([np.asarray(padded_public, dtype=np.uint64).reshape(-1, 4), np.asarray(private, dtype=np.uint64).reshape(-1, 4)])
    return reg.mul(z, n_out)


def m_at_alpha_evals_device(reg_transposed, lg_constraint_domain, alpha, d_out, d_lagrange):
    """third.rs:303-306 without a download: `constraint_domain.evaluate_all_lagrange_coefficients(alpha)` into the device vector d_lagrange
    (2^lg_constraint_domain elements, the caller's; `snarkvm_hip_fr_lagrange_coefficients`), then for every row of the registered TRANSPOSE the
    sum of val * l_at_alpha[row_index] into d_out (reg_transposed.rows = variable-domain-size elements), ready for the inverse transform.
    Inside a scope both calls are only enqueued."""
    if reg_transposed.cols > (1 << lg_constraint_domain):
        raise ValueError("m_at_alpha_evals_device: the matrix has more constraints than the constraint domain has elements")
    tau = np.ascontiguousarray(alpha, dtype=np.uint64).reshape(1, 4)
    _lib.check(_lib.lib().snarkvm_hip_fr_lagrange_coefficients(_dev_ptr(d_lagrange), lg_constraint_domain, tau.ctypes.data, 1))
    reg_transposed.mul_device(d_out, reg_transposed.rows, d_lagrange)
