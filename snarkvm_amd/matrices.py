"""The sparse side of the Varuna prover on the gfx950 backend: an R1CS matrix (`Matrix<F>` = a list of rows of `(value, column)`,
algorithms/src/snark/varuna/ahp/matrices.rs) registered once in device memory and multiplied with vectors that live there.

    z_M = M z for M in {A, B, C}            snark/varuna/ahp/prover/round_functions/mod.rs:131-188 (`inner_product` over every row)
    M(alpha, .) = M^T l_alpha               snark/varuna/ahp/prover/round_functions/third.rs:303-306, with the transpose of ahp/matrices.rs:250-264
    a, b, f on K, sum, g_M, lhs_M           round_functions/fourth.rs:155-245 over the arithmetization of ahp/matrices.rs:138-195; h_2: fifth.rs:50-64

The transpose is circuit data like the matrix itself: built once on the host (`transpose`) and registered; the product is
`snarkvm_hip_fr_spmv` (include/snarkvm_hip.h).  The arithmetization (row, col, row_col_val on K) is circuit data too: built once on the host
(`matrix_evals`), registered (`RegisteredArithmetization`), and turned into the round-4 witness of every proof by one fused kernel
(`snarkvm_hip_fr_matrix_sumcheck_evals`) followed by entry points that already exist (`matrix_sumcheck_witness`).

    z = w (X^|X| - 1) + x                   round_functions/third.rs:220-249 (`assignment_device`)
    h_1, x g_1, g_1 and the MatrixSums      third.rs:126-218, 280-327 with ahp/selectors.rs:100-121 (`lineval_sumcheck_witness`)

Round 3 is driven here from the registered transposes to its two oracles: the sparse products, the transforms and the per-member products
are entry points that already exist, and the selector of every (instance, matrix) member, the running h_1 / x g_1 sums, the mask polynomial
and the sums over the variable domain are ONE pass (`snarkvm_hip_fr_selector_fold`).

    w = (gather of the private variables - x) / (X^|X| - 1)     round_functions/first.rs:127-161 (`witness_poly_device`)
    h_0 = sum mu (z_a z_b - z_c) / v_R                          round_functions/second.rs:76-142 with ahp/selectors.rs:88-99 (`rowcheck_witness`)

Rounds 1 and 2 open a proof: w by the gather `snarkvm_hip_fr_witness_evals` between two transforms at |V|, h_0 for all instances of all circuits
on one coset per domain size with `snarkvm_hip_fr_rowcheck_fold` as both the divisibility test and the sum.

    z = iNTT_|V|(interleave(public, private)), w = z div (X^|X| - 1), x_poly = z mod (X^|X| - 1)     (`first_round_device`)

Round 1 in lock step: every instance of every circuit from ONE gather (`snarkvm_hip_fr_assignment_evals`), one inverse transform and one division
per instance, with z_a, z_b, z_c as three strided products per circuit - enqueued in the caller's scope like rounds 2 to 4.

    row, col, row_col, row_col_val on K, the twelve index polynomials, their commitments and the certificate
                                                                ahp/indexer/indexer.rs:126-260, circuit.rs:142-155, varuna.rs:103-117 (`CircuitIndex`)

The circuit index is built here as well, from the three CSR matrices alone: `snarkvm_hip_fr_arithmetize` computes the arithmetization where it
will live (`RegisteredArithmetization.from_csr`: every device its own replica), one inverse transform batch per matrix interpolates it, and the
registered objects, resident polynomials and commitments that `CircuitIndex.build` leaves are the ones the drivers above and the gamma-point opening take.
"""
import collections
import ctypes

import numpy as np

from . import _lib, plugin
from .devmem import HipMem

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
    padded_public[i] below the number of public variables and private[i - that] above, i.e. x is simply public ++ private.
    All instances of a circuit at once, on device rows: `first_round_device`."""
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


# ---- round 4: the matrix sumcheck ------------------------------------------------------------------------------------------------------------
_TWO_ADICITY = 47
_TWO_ADIC_ROOT = 8065159656716812877374967518403273466521432693661810619979959746626482506078  # curves/src/bls12_377/fr.rs:109-120


def _lg(size, what):
    size = int(size)
    if size < 1 or size & (size - 1):
        raise ValueError(f"{what} is not a power of two")
    return size.bit_length() - 1


def _domain_elements(size):
    """the elements 1, w, w^2, ... of the multiplicative subgroup of `size` elements (EvaluationDomain::elements), Python ints"""
    w = pow(_TWO_ADIC_ROOT, 1 << (_TWO_ADICITY - _lg(size, "a domain size")), R_MOD)
    out, x = [], 1
    for _ in range(size):
        out.append(x)
        x = x * w % R_MOD
    return out


def _mont_limbs(values):
    return np.array([_fr_mont(v) for v in values], dtype=np.uint64).reshape(-1, 4)


def _from_mont(limbs):
    inv = pow(_MONT_R, -1, R_MOD)
    return [(int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192) * inv % R_MOD for a, b, c, d in np.asarray(limbs, dtype=np.uint64).reshape(-1, 4).tolist()]


def matrix_evals(matrix, non_zero_domain_size, variable_domain_size, input_domain_size, constraint_domain_size=None):
    """`matrix_evals` of ahp/matrices.rs:138-195: the arithmetization of a SparseMatrix on the non-zero domain K -> (row, col, row_col_val), each a
    (|K|, 4) array in Montgomery memory form.  Entry (val, j) of row i gives row = the i-th element of the constraint domain (the smallest power of
    two >= the number of rows unless constraint_domain_size says otherwise), col = element reindex_by_subdomain(j) of the variable domain and
    row_col_val = val * row * col; the places behind the entries are padded with (1, 1, 0).  Host-side big-int work, done once per circuit."""
    k = int(non_zero_domain_size)
    _lg(k, "non_zero_domain_size")
    if matrix.nnz > k:
        raise ValueError("matrix_evals: the matrix has more entries than the non-zero domain has elements")
    if constraint_domain_size is None:
        constraint_domain_size = 1 << max(0, (matrix.rows - 1).bit_length())
    if matrix.rows > constraint_domain_size:
        raise ValueError("matrix_evals: the matrix has more rows than the constraint domain has elements")
    r_elems, c_elems = _domain_elements(constraint_domain_size), _domain_elements(variable_domain_size)
    at = _reindex_all(variable_domain_size, input_domain_size, matrix.col_idx).tolist() if matrix.nnz else []
    if at and max(at) >= variable_domain_size:
        raise ValueError("matrix_evals: a variable does not fit the variable domain")
    src_row = np.repeat(np.arange(matrix.rows, dtype=np.int64), matrix.row_lengths()).tolist()
    vals = _from_mont(matrix.vals)
    row = [r_elems[i] for i in src_row] + [1] * (k - matrix.nnz)
    col = [c_elems[j] for j in at] + [1] * (k - matrix.nnz)
    rcv = [v * r % R_MOD * c % R_MOD for v, r, c in zip(vals, row, col)] + [0] * (k - matrix.nnz)
    return _mont_limbs(row), _mont_limbs(col), _mont_limbs(rcv)


class RegisteredArithmetization:
    """row, col and row_col_val of one matrix on K resident in device memory (`snarkvm_hip_fr_arith_register`: on every device in use), for as many
    proofs as the proving key lives - the twin of RegisteredMatrix.  close() - also run when the object dies - releases it; that is safe while a
    scope of the calling thread still has an evaluation enqueued (the release waits for the device)."""

    def __init__(self, row, col, row_col_val):
        row, col, rcv = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (row, col, row_col_val))
        if not row.shape[0] == col.shape[0] == rcv.shape[0]:
            raise ValueError("RegisteredArithmetization: row, col and row_col_val differ in length")
        self.k = row.shape[0]
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().snarkvm_hip_fr_arith_register(ctypes.byref(h), self.k, *(x.ctypes.data if self.k else None for x in (row, col, rcv))))
        self.handle = h.value or 0

    @classmethod
    def from_matrix(cls, matrix, non_zero_domain_size, variable_domain_size, input_domain_size, constraint_domain_size=None):
        return cls(*matrix_evals(matrix, non_zero_domain_size, variable_domain_size, input_domain_size, constraint_domain_size))

    @classmethod
    def from_csr(cls, matrix, non_zero_domain_size, lg_constraint, lg_variable, lg_input):
        """The same object without the host-side arithmetization: the CSR arrays go to the device and every device in use computes its own
        replica (`snarkvm_hip_fr_arith_register_csr`)."""
        self = cls.__new__(cls)
        self.k, self.handle = int(non_zero_domain_size), 0
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().snarkvm_hip_fr_arith_register_csr(ctypes.byref(h), self.k, matrix.rows, matrix.row_ptr.ctypes.data, matrix.col_idx.ctypes.data if matrix.nnz else None,
                                                                matrix.vals.ctypes.data if matrix.nnz else None, int(lg_constraint), int(lg_variable), int(lg_input)))
        self.handle = h.value or 0
        return self

    def close(self):
        if self.handle:
            h, self.handle = self.handle, 0
            _lib.lib().snarkvm_hip_fr_arith_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown / a dead device: nothing left to do
            pass


def sumcheck_scales(lg_r, lg_c, alpha, beta):
    """a_scale = v_R(alpha) v_C(beta), b_scale = |R| |C|, f_scale = a_scale / (|R| |C|) (fourth.rs:95-97, 171-172, 208) as a (3, 4) array; alpha, beta:
    Montgomery limbs"""
    al, be = _from_mont(alpha)[0], _from_mont(beta)[0]
    a_scale = (pow(al, 1 << lg_r, R_MOD) - 1) * (pow(be, 1 << lg_c, R_MOD) - 1) % R_MOD
    b_scale = (1 << (lg_r + lg_c)) % R_MOD
    return _mont_limbs([a_scale, b_scale, a_scale * pow(b_scale, -1, R_MOD) % R_MOD])


class DevicePoly:
    """`n` coefficients at device address `ptr`; `owner` keeps the block they live in alive"""

    def __init__(self, ptr, n, owner):
        self.ptr, self.n, self.owner = int(ptr), int(n), owner

    def download(self):
        out = np.empty((self.n, 4), dtype=np.uint64)
        if self.n:
            _lib.check(_lib.lib().snarkvm_hip_memcpy_d2h(out.ctypes.data, self.ptr, 32 * self.n))
        return out


def matrix_sumcheck_witness(regs, lg_r, lg_c, alpha, beta, max_non_zero_domain_size, scales=None, device=-1):
    """`calculate_matrix_sumcheck_witness` (fourth.rs:155-245) for the registered arithmetizations `regs` of ONE circuit (constraint domain 2^lg_r,
    variable domain 2^lg_c; every |K_M| a power of two), on device memory: the fused evaluations of a, b, f for all members, one inverse
    transform batch per domain size, then per member `polymul_device(b, f)`, a - b f in one `fr_lincomb`, the division by v_K
    (`fr_divide_by_vanishing`), the zero test of the remainder (`fr_support`; a non-zero remainder raises ValueError like the `ensure!` of
    selectors.rs:92-93) and the |K_M| / |K_max| multiplier (selectors.rs:95-96).
    -> one (sum, lhs, g, a_poly, b_poly) per member: sum = f[0] as a (1, 4) host array, the others DevicePoly - lhs |K_M| coefficients, g = f from
    coefficient 1 on (|K_M| - 1 coefficients, a pointer offset into f: ready for a resident commitment), a_poly and b_poly |K_M| coefficients.
    Lengths are untrimmed.  scales: (3, 4) a_scale, b_scale, f_scale when the caller has them already (default: sumcheck_scales).  Call it outside a
    scope: it reads the sums and the remainder tests back."""
    L = _lib.lib()
    lgs = [_lg(r.k, "the size of a registered arithmetization") for r in regs]
    k_max = int(max_non_zero_domain_size)
    _lg(k_max, "max_non_zero_domain_size")
    scales = sumcheck_scales(lg_r, lg_c, alpha, beta) if scales is None else scales
    # per member: a | b | f | b f and then a - b f (2 |K|) | quotient | remainder
    mems = [HipMem(32 * 7 * r.k, device) for r in regs]
    at = lambda m, off: mems[m].ptr + 32 * off * regs[m].k
    n = len(regs)
    plugin.fr_sumcheck_evals_device([r.handle for r in regs], [at(m, 0) for m in range(n)], [at(m, 1) for m in range(n)], [at(m, 2) for m in range(n)],
                                    alpha, beta, scales)
    for lg in sorted(set(lgs)):
        ptrs = [at(m, j) for m in range(n) if lgs[m] == lg for j in range(3)]
        plugin.NTT_device_batch(lg, ptrs, directions=[1] * len(ptrs), types=[0] * len(ptrs))
    minus_one = _mont_limbs([1, R_MOD - 1])
    out = []
    for m, reg in enumerate(regs):
        k = reg.k
        d_a, d_b, d_f, d_h, d_q, d_r = (at(m, j) for j in (0, 1, 2, 3, 5, 6))
        total = mems[m].download(32, 32 * 2 * k, dtype=np.uint64).reshape(1, 4)
        plugin.polymul_device(lgs[m] + 1, d_h, polys=[(d_b, k), (d_f, k)])
        plugin.fr_lincomb_device(d_h, 2 * k, [d_a, d_h], [k, 2 * k], minus_one)
        _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(d_q, d_r, d_h, 2 * k, k, 1))
        if int(plugin.fr_support_device(d_r, k)[0]) != 0:
            raise ValueError("Failed to divide by vanishing polynomial - non-zero remainder")
        if k != k_max:
            mult = _mont_limbs([k * pow(k_max, -1, R_MOD) % R_MOD])
            _lib.check(L.snarkvm_hip_fr_vec_op(4, d_q, d_q, None, None, mult.ctypes.data, k, 1))
        out.append((total, DevicePoly(d_q, k, mems[m]), DevicePoly(d_f + 32, k - 1, mems[m]), DevicePoly(d_a, k, mems[m]), DevicePoly(d_b, k, mems[m])))
    return out


def h_2(lhs_list, deltas, device=-1):
    """fifth.rs:50-64: sum_M delta_M lhs_M over the DevicePoly `lhs_list` as ONE `fr_lincomb` -> DevicePoly of max |K_M| coefficients.  deltas:
    (len(lhs_list), 4) Montgomery limbs on the host."""
    n = max((p.n for p in lhs_list), default=0)
    mem = HipMem(32 * max(n, 1), device)
    plugin.fr_lincomb_device(mem.ptr, n, [p.ptr for p in lhs_list], [p.n for p in lhs_list], deltas)
    return DevicePoly(mem.ptr, n, mem)


# ---- round 3: the lineval sumcheck -------------------------------------------------------------------------------------------------------------
def assignment_device(d_w, w_len, d_x, input_size, d_out):
    """`calculate_assignments` (third.rs:236-239) for one instance on device memory: d_out (w_len + input_size coefficients, the caller's) =
    w (X^input_size - 1) + x, with w of w_len coefficients at d_w and x of input_size coefficients at d_x - `fr_mul_by_vanishing`, then x added
    in place by one `fr_lincomb`.  d_out must overlap neither operand.  -> the number of coefficients written.  Inside a scope both calls are
    only enqueued.  The lock-step route yields z before w, without either call: `first_round_device`."""
    n = int(w_len) + int(input_size)
    out = _dev_ptr(d_out)
    _lib.check(_lib.lib().snarkvm_hip_fr_mul_by_vanishing(out, _dev_ptr(d_w) or None, int(w_len), int(input_size), 1))
    plugin.fr_lincomb_device(out, n, [out, _dev_ptr(d_x)], [n, int(input_size)], _mont_limbs([1, 1]))
    return n


LinevalCircuit = collections.namedtuple("LinevalCircuit", "transposes lg_r lg_c circuit_combiner instance_combiners assignments")
LinevalCircuit.__doc__ = """One circuit of round 3: `transposes` = the RegisteredMatrix of the transposes of A, B, C (`transpose`, 2^lg_c rows each), the
constraint domain 2^lg_r and the variable domain 2^lg_c, `circuit_combiner` ((4,) Montgomery limbs), `instance_combiners` ((instances, 4)) and
`assignments`: one DevicePoly z per instance (`assignment_device`)."""


def lineval_sumcheck_witness(circuits, alpha, eta_b, eta_c, lg_max_variable_domain, mask=None, device=-1):
    """`calculate_lineval_sumcheck_witness` (third.rs:126-218) over the LinevalCircuit list `circuits`, on device memory.  Per circuit, once (the
    reference repeats it per instance, but it does not depend on the instance): l_alpha and M(alpha, .) = M^T l_alpha for the three registered
    transposes, one inverse transform batch at |C|.  Then the M(alpha, X) and every assignment go zero-padded to the product domain (the
    smallest power of two >= |C| + len(z) - 1) through ONE forward transform batch - an assignment is transformed once, not once per matrix -
    and every (instance, matrix) product is one `polymul_device` over two evaluation vectors.  All 3 I members, and the mask polynomial
    (third.rs:207-213: a further member with n = N and multiplier one), end in ONE `snarkvm_hip_fr_selector_fold`.
    alpha, eta_b, eta_c: (4,) Montgomery limbs; mask: a DevicePoly or None (non-hiding mode).
    -> (h_1, xg_1, g_1, sums): DevicePoly h_1 (untrimmed: the longest quotient, at least one coefficient), xg_1 (N = 2^lg_max_variable_domain
    coefficients) and g_1 = xg_1 from coefficient 1 on (a pointer offset: ready for a resident commitment); sums: per circuit an
    (instances, 3, 4) host array in the MatrixSums order sum_a, sum_b, sum_c.  Call it outside a scope: it reads the sums back."""
    L = _lib.lib()
    N = 1 << int(lg_max_variable_domain)
    n_inv = pow(N, -1, R_MOD)
    matrix_combiners = [1, _from_mont(eta_b)[0], _from_mont(eta_c)[0]]
    tau = np.ascontiguousarray(alpha, dtype=np.uint64).reshape(1, 4)
    keep, ptrs, lens, srcs, mus = [], [], [], [], []
    for c in circuits:
        size_c = 1 << c.lg_c
        if size_c > N or any(t.rows != size_c for t in c.transposes) or len(c.transposes) != 3:
            raise ValueError("lineval_sumcheck_witness: three transposes of |C| rows each, |C| <= the maximal variable domain")
        inst = _from_mont(c.instance_combiners)
        if len(inst) != len(c.assignments):
            raise ValueError("lineval_sumcheck_witness: one instance combiner per assignment")
        z_max = max((z.n for z in c.assignments), default=0)
        if not c.assignments or z_max == 0:
            continue
        lg_p = max(size_c + z_max - 2, 0).bit_length()
        P = 1 << lg_p
        # m_A | m_B | m_C | one padded copy per assignment | one product per (instance, matrix); l_alpha apart
        mem = HipMem(32 * P * (3 + 4 * len(c.assignments)), device)
        lag = HipMem(32 << c.lg_r, device)
        at = lambda j: mem.ptr + 32 * P * j
        mem.fill(0, 0, 32 * P * (3 + len(c.assignments)))
        _lib.check(L.snarkvm_hip_fr_lagrange_coefficients(lag.ptr, c.lg_r, tau.ctypes.data, 1))
        for m, t in enumerate(c.transposes):
            if t.cols > (1 << c.lg_r):
                raise ValueError("lineval_sumcheck_witness: a matrix has more constraints than the constraint domain has elements")
            t.mul_device(at(m), size_c, lag.ptr)
        plugin.NTT_device_batch(c.lg_c, [at(m) for m in range(3)], directions=[1] * 3, types=[0] * 3)
        for i, z in enumerate(c.assignments):
            mem.copy_from(32 * P * (3 + i), z.ptr, 32 * z.n)
        nv = 3 + len(c.assignments)
        plugin.NTT_device_batch(lg_p, [at(j) for j in range(nv)], directions=[0] * nv, types=[0] * nv)
        cc = _from_mont(c.circuit_combiner)[0]
        for i, z in enumerate(c.assignments):
            for m in range(3):
                d_prod = at(nv + 3 * i + m)
                plugin.polymul_device(lg_p, d_prod, evals=[at(m), at(3 + i)])
                ptrs.append(d_prod), lens.append(size_c + z.n - 1), srcs.append(size_c)
                mus.append(cc * inst[i] % R_MOD * matrix_combiners[m] % R_MOD * size_c % R_MOD * n_inv % R_MOD)
        keep += [mem, lag]
    members = len(ptrs)
    if mask is not None and mask.n:
        ptrs.append(mask.ptr), lens.append(mask.n), srcs.append(N), mus.append(1)
    h_len = max([max(l - s, 0) for l, s in zip(lens, srcs)] + [1])
    out = HipMem(32 * (h_len + N + max(len(ptrs), 1)), device)
    d_h, d_xg, d_sums = out.ptr, out.ptr + 32 * h_len, out.ptr + 32 * (h_len + N)
    plugin.fr_selector_fold_device(d_h, h_len, d_xg, N, d_sums if ptrs else None, ptrs, lens, srcs, _mont_limbs(mus))
    flat = out.download(32 * members, 32 * (h_len + N), dtype=np.uint64).reshape(-1, 3, 4)
    sums, first = [], 0
    for c in circuits:
        count = len(c.assignments) if any(z.n for z in c.assignments) else 0
        sums.append(flat[first : first + count].copy() if count else np.zeros((len(c.assignments), 3, 4), dtype=np.uint64))
        first += count
    del keep
    return DevicePoly(d_h, h_len, out), DevicePoly(d_xg, N, out), DevicePoly(d_xg + 32, N - 1, out), sums


# ---- rounds 1 and 2: w and the rowcheck witness h_0 ----------------------------------------------------------------------------------------------
_COSET_GENERATOR = 22  # Fr::GENERATOR (curves/src/bls12_377/fr.rs): the shift of the coset transforms (NTTType::Coset)


class _Scope:
    """A deferred-synchronisation scope of the calling thread around a driver function, unless the thread has one open already (scopes do not
    nest): every device-resident call inside is only enqueued and the host waits once.  `own`: this object opened it."""

    def __init__(self, d_any):
        self.d_any, self.own = int(d_any), False

    def __enter__(self):
        L = _lib.lib()
        if not L.snarkvm_hip_scope_stream():
            _lib.check(L.snarkvm_hip_scope_begin(ctypes.c_void_p(self.d_any)))
            self.own = True
        return self

    def __exit__(self, exc_type, exc, tb):
        if self.own:
            err = _lib.lib().snarkvm_hip_scope_end()  # a failed call must not leave this thread's scope open
            if exc_type is None:
                _lib.check(err)
        return False


def witness_poly_device(d_w, w_len, d_x_poly, input_size, lg_variable_domain, d_out, device=-1):
    """`calculate_w` (first.rs:127-161) for one instance on device memory: the private variables (w_len <= |V| - |X| elements at d_w) and x_poly
    (input_size = |X| coefficients at d_x_poly: the interpolation of the padded public input) -> the |V| - |X| coefficients of w in d_out (the
    caller's; it must overlap neither operand).  x_poly goes zero-padded to |V| = 2^lg_variable_domain through the forward transform, the gather
    `snarkvm_hip_fr_witness_evals` runs in place on its evaluations, the inverse transform yields w (X^|X| - 1) and `fr_divide_by_vanishing` by
    X^|X| - 1 the quotient; the remainder is tested with `fr_support` and a non-zero one raises ValueError (it cannot happen for valid sizes: the
    gathered vector vanishes on the input subgroup).  Workspace: |V| + |X| elements on `device` (the device of d_out), released on return.  The five
    calls run in one scope and wait once.  Call it outside a scope: it reads the remainder test back.  -> the number of coefficients written.
    Every instance of every circuit in one scope, from one inverse transform each and with nothing read back: `first_round_device`."""
    L = _lib.lib()
    V, X, w_len = 1 << int(lg_variable_domain), int(input_size), int(w_len)
    if X < 1 or X & (X - 1) or X > V:
        raise ValueError("witness_poly_device: input_size is a power of two, at most the variable domain")
    if w_len < 0 or w_len > V - X:
        raise ValueError("witness_poly_device: more private variables than the variable domain has room for")
    if L.snarkvm_hip_scope_stream():
        raise ValueError("witness_poly_device: call it outside a scope (it reads the remainder test back)")
    work = HipMem(32 * (V + X), device)
    d_rem = work.ptr + 32 * V
    with _Scope(work.ptr):
        work.fill(32 * X, 0, 32 * (V - X))
        work.copy_from(0, _dev_ptr(d_x_poly), 32 * X)
        plugin.NTT_device_batch(int(lg_variable_domain), [work.ptr], directions=[0], types=[0])
        plugin.fr_witness_evals_device(work.ptr, V, _dev_ptr(d_w) if w_len else None, w_len, work.ptr, X)
        plugin.NTT_device_batch(int(lg_variable_domain), [work.ptr], directions=[1], types=[0])
        _lib.check(L.snarkvm_hip_fr_divide_by_vanishing(_dev_ptr(d_out) if V > X else None, d_rem, work.ptr, V, X, 1))
        support = plugin.fr_support_device(d_rem, X)
    if int(support[0]) != 0:
        raise ValueError("Failed to divide by vanishing polynomial - non-zero remainder")
    return V - X


def witness_label(circuit_id, poly, i):
    """`witness_label` of ahp/ahp.rs:46-50"""
    return f"circuit_{circuit_id}_{poly}_{i:0>8}"


FirstRoundCircuit = collections.namedtuple("FirstRoundCircuit", "matrices lg_r lg_c lg_x vars num_vars stride instances")
FirstRoundCircuit.__doc__ = """One circuit of round 1: `matrices` = the RegisteredMatrix of A, B, C (num_vars columns each), the constraint, variable and input
domains 2^lg_r, 2^lg_c, 2^lg_x, and `vars`: a device arena (pointer or HipMem) of `instances` rows, row m starting m * stride elements in and
holding padded_public (2^lg_x values) ++ private (num_vars - 2^lg_x values) - the x operand of the matrices' products."""

FirstRoundWitness = collections.namedtuple("FirstRoundWitness", "z w x_poly z_m w_labeled")
FirstRoundWitness.__doc__ = """What round 1 leaves for one circuit, one entry per instance each: DevicePoly `z` (|V| coefficients, untrimmed: `LinevalCircuit.assignments`),
`w` (|V| - |X|) and `x_poly` (|X|); `z_m`: the (z_a, z_b, z_c) triples of |R| evaluations (`RowcheckCircuit.z`); `w_labeled`: the w as
sonic_pc.ResidentPolynomial under `witness_label(circuit_id, "w", i)`, ready for `SonicKZG10.commit`."""


def _ntt_batch_cap(lg):
    """the vectors one launch sequence of `snarkvm_hip_ntt_device_batch` takes (include/snarkvm_hip.h)"""
    return 48 if lg <= 26 else 48 >> (lg - 26)


def first_round_device(circuits, device=-1, circuit_ids=None, hiding_bound=None):
    """Round 1 in lock step over the FirstRoundCircuit list `circuits`, on device memory: for every instance of every circuit the assignment z,
    the witness polynomial w (`calculate_w`, first.rs:127-161), x_poly (prover/state.rs:150) and z_a, z_b, z_c (round_functions/mod.rs:131-188).
    The reference's evaluations of w plus those of x_poly are the evaluations of z itself - the public input on the input subgroup, the private
    variables elsewhere, the interleaving of `reindex_by_subdomain` - and z = w (X^|X| - 1) + x_poly with deg x_poly < |X|, so
        z = iNTT_|V|(interleave(public, private)),   w = z div (X^|X| - 1),   x_poly = z mod (X^|X| - 1).
    Per circuit: ONE `snarkvm_hip_fr_assignment_evals` over all instances, the inverse transforms at |V| (`NTT_device_batch`, in chunks of what one
    launch sequence takes), ONE `snarkvm_hip_fr_divide_by_vanishing_strided` and three strided `fr_spmv` over the rows with n_out = |R| - no
    forward transform, no transform at |X|, no remainder to test.  One block of device memory per circuit holds z | w ++ x_poly | z_a | z_b | z_c
    of every instance.  Field arithmetic is exact: every byte equals the per-instance route's (`witness_poly_device`, `assignment_device`, `z_m`).
    Every call is only enqueued - in the caller's open scope, or in a scope of its own when the calling thread has none (then the host waits
    once); nothing is read back.  circuit_ids: the ids the labels of w carry (default: the position in `circuits`); hiding_bound: that of every w
    (`zk_bound`, first.rs:160).  -> one FirstRoundWitness per circuit."""
    from . import sonic_pc

    if circuit_ids is None:
        circuit_ids = list(range(len(circuits)))
    if len(circuit_ids) != len(circuits):
        raise ValueError("first_round_device: one circuit id per circuit")
    plans = []
    for c in circuits:
        V, X, R, count = 1 << int(c.lg_c), 1 << int(c.lg_x), 1 << int(c.lg_r), int(c.instances)
        if X > V:
            raise ValueError("first_round_device: the input domain is larger than the variable domain")
        if not X <= int(c.num_vars) <= V:
            raise ValueError("first_round_device: a row holds between |X| and |V| variables")
        if len(c.matrices) != 3 or any(m.cols != int(c.num_vars) or m.rows > R for m in c.matrices):
            raise ValueError("first_round_device: three matrices of num_vars columns and at most |R| rows each")
        if count < 0 or (count > 1 and int(c.stride) < int(c.num_vars)):
            raise ValueError("first_round_device: the rows of the arena overlap")
        plans.append((V, X, R, count))
    # per circuit: z of every instance | w ++ x_poly of every instance | z_a | z_b | z_c of every instance
    mems = [HipMem(32 * max(count * (2 * V + 3 * R), 1), device) for V, X, R, count in plans]
    out = []
    if not mems:
        return out
    with _Scope(mems[0].ptr):
        for c, cid, mem, (V, X, R, count) in zip(circuits, circuit_ids, mems, plans):
            d_z, d_w, d_zm = mem.ptr, mem.ptr + 32 * count * V, mem.ptr + 32 * count * 2 * V
            if count:
                plugin.fr_assignment_evals_device(d_z, V, _dev_ptr(c.vars), c.num_vars, X, count, V, c.stride)
                cap = _ntt_batch_cap(int(c.lg_c))
                for first in range(0, count, cap):
                    ptrs = [d_z + 32 * V * i for i in range(first, min(first + cap, count))]
                    plugin.NTT_device_batch(int(c.lg_c), ptrs, directions=[1] * len(ptrs), types=[0] * len(ptrs))
                # member i: quotient at d_w + i |V| (|V| - |X| coefficients), remainder right behind it (|X| coefficients)
                _lib.check(_lib.lib().snarkvm_hip_fr_divide_by_vanishing_strided(d_w if V > X else None, d_w + 32 * (V - X), d_z, V, X, count, V))
                for j, m in enumerate(c.matrices):
                    m.mul_device(d_zm + 32 * count * R * j, R, c.vars, count, int(c.stride), R)
            z = [DevicePoly(d_z + 32 * V * i, V, mem) for i in range(count)]
            w = [DevicePoly(d_w + 32 * V * i, V - X, mem) for i in range(count)]
            x_poly = [DevicePoly(d_w + 32 * (V * i + V - X), X, mem) for i in range(count)]
            triples = [tuple(DevicePoly(d_zm + 32 * R * (count * j + i), R, mem) for j in range(3)) for i in range(count)]
            labeled = [sonic_pc.ResidentPolynomial(witness_label(cid, "w", i), p.ptr, p.n, None, hiding_bound) for i, p in enumerate(w)]
            for p in labeled:
                p._owner = mem  # the block stays alive as long as a polynomial in it
            out.append(FirstRoundWitness(z, w, x_poly, triples, labeled))
    return out


RowcheckCircuit = collections.namedtuple("RowcheckCircuit", "lg_r circuit_combiner instance_combiners z")
RowcheckCircuit.__doc__ = """One circuit of round 2: the constraint domain 2^lg_r, `circuit_combiner` ((4,) Montgomery limbs), `instance_combiners`
((instances, 4)) and `z`: per instance the three device vectors (z_a, z_b, z_c) of 2^lg_r evaluations each - pointers or DevicePoly, the
n_out-padded outputs of `RegisteredMatrix.mul_device`."""


class RowcheckWitness(DevicePoly):
    """h_0 as a DevicePoly, with the divisibility test of the round: `violations` = per (circuit, instance) member, in the order of `members`, the
    number of rows with z_a z_b != z_c - filled when the scope the calls were enqueued in has ended."""

    def __init__(self, ptr, n, owner, members, counts):
        super().__init__(ptr, n, owner)
        self.members, self._counts = members, counts

    @property
    def violations(self):
        return [int(c) for arr in self._counts for c in arr]

    def ensure_divisible(self):
        """the `ensure!` of selectors.rs:92-93: raises ValueError naming the first member with a violated row"""
        for (circuit, instance), count in zip(self.members, self.violations):
            if count:
                raise ValueError(f"Failed to divide by vanishing polynomial - non-zero remainder (circuit {circuit}, instance {instance}: "
                                 f"{count} rows with z_a z_b != z_c)")
        return self


def rowcheck_witness(circuits, lg_max_constraint_domain, device=-1):
    """`calculate_rowcheck_witness` (second.rs:76-142) over the RowcheckCircuit list `circuits`, on device memory: h_0 = the sum over every instance
    of every circuit of instance_combiner * circuit_combiner * |R| / |R_max| * (z_a z_b - z_c) / v_R (apply_randomized_selector without a remainder
    witness, selectors.rs:88-99).  z_a z_b - z_c has degree <= 2 |R| - 2 and its quotient by v_R degree <= |R| - 2, so the quotient is fixed by
    its values on ONE coset g R (g = 22, the shift of NTTType::Coset), where v_R is the constant g^|R| - 1 - no transform at 2 |R|.  Per distinct
    domain size: one check-only `snarkvm_hip_fr_rowcheck_fold` over the evaluations as given (the remainder by v_R is zero iff z_a z_b = z_c on
    all of R), one inverse transform batch, one forward coset batch, ONE fold with mu = instance_combiner * circuit_combiner * |R| / |R_max| /
    (g^|R| - 1) and - the inverse transform being linear - ONE inverse coset transform where the reference runs one per instance; then one
    `fr_lincomb` across the sizes when there are several (or a size below |R_max|).  Field arithmetic is exact: the coefficients are the
    reference's bytes whenever the reference succeeds.
    The input vectors are CONSUMED, as `z_a.take()` does (second.rs:104-106): on return they hold coset evaluations.
    Every call is only enqueued: in a scope of its own when the calling thread has none open - then the host waits once, a violated row raises
    ValueError with the reference's message "Failed to divide by vanishing polynomial - non-zero remainder", naming the first offending member,
    and no h_0 is returned - or in the caller's open scope: nothing is waited for, and the caller runs `ensure_divisible()` on the result after
    its scope has ended (the counts arrive with `snarkvm_hip_scope_end`, like the result of `fr_support`).
    -> RowcheckWitness (a DevicePoly) of |R_max| = 2^lg_max_constraint_domain coefficients, untrimmed."""
    lg_max = int(lg_max_constraint_domain)
    n_max = 1 << lg_max
    by_size = collections.OrderedDict()
    for ci, c in enumerate(circuits):
        lg = int(c.lg_r)
        if lg < 0 or lg > lg_max:
            raise ValueError("rowcheck_witness: a constraint domain is larger than the maximal one")
        inst = _from_mont(c.instance_combiners)
        if len(inst) != len(c.z):
            raise ValueError("rowcheck_witness: one instance combiner per instance")
        cc = _from_mont(c.circuit_combiner)[0]
        for i, (za, zb, zc) in enumerate(c.z):
            by_size.setdefault(lg, []).append(((ci, i), (_dev_ptr(za), _dev_ptr(zb), _dev_ptr(zc)), cc * inst[i] % R_MOD))
    sizes = sorted(by_size)
    direct = len(sizes) == 1 and sizes[0] == lg_max  # the one fold's output is h_0 itself
    total = sum(1 << lg for lg in sizes) + (0 if direct else n_max)
    mem = HipMem(32 * max(total, 1), device)
    members, counts, parts, at = [], [], [], 0 if direct else n_max
    with _Scope(mem.ptr) as scope:
        for lg in sizes:
            n, group = 1 << lg, by_size[lg]
            a, b, c3 = ([m[1][j] for m in group] for j in range(3))
            members += [m[0] for m in group]
            counts.append(plugin.fr_rowcheck_fold_device(None, n, a, b, c3, None))
            ptrs = a + b + c3
            plugin.NTT_device_batch(lg, ptrs, directions=[1] * len(ptrs), types=[0] * len(ptrs))
            plugin.NTT_device_batch(lg, ptrs, directions=[0] * len(ptrs), types=[1] * len(ptrs))
            scale = (1 << lg) * pow(n_max, -1, R_MOD) % R_MOD * pow(pow(_COSET_GENERATOR, n, R_MOD) - 1, -1, R_MOD) % R_MOD
            d_part = mem.ptr + 32 * at
            plugin.fr_rowcheck_fold_device(d_part, n, a, b, c3, _mont_limbs([m[2] * scale % R_MOD for m in group]), violations=False)
            plugin.NTT_device_batch(lg, [d_part], directions=[1], types=[1])
            parts.append((d_part, n))
            at += n
        if not direct:
            plugin.fr_lincomb_device(mem.ptr, n_max, [p for p, _ in parts], [n for _, n in parts], _mont_limbs([1] * len(parts)))
    out = RowcheckWitness(mem.ptr, n_max, mem, members, counts)
    return out.ensure_divisible() if scope.own else out


# ---- the circuit index: arithmetize, interpolate, commit ---------------------------------------------------------------------------------------
INDEX_KINDS = ("row", "col", "row_col", "row_col_val")  # the order of index_polynomial_labels_single (indexer.rs:104-115) and of a device block


def _domain_lg(n):
    """lg of EvaluationDomain::new(n): the smallest power of two >= n (one element for n = 0)"""
    return max(0, (int(n) - 1).bit_length())


def index_label(circuit_id, kind, matrix):
    return f"circuit_{circuit_id}_{kind}_{matrix}"


class CircuitIndex:
    """What `AHPForR1CS::index` leaves for a circuit (indexer.rs:46-92, 126-228) - without constraint synthesis, `into_matrix_helper` and the id hash,
    which stay with the caller: from the three CSR matrices alone, everything the round drivers of this module and the gamma-point opening consume.

        matrices, transposes    RegisteredMatrix of A, B, C and of their transposes (z_M; `LinevalCircuit.transposes`)
        ariths                  RegisteredArithmetization per matrix, computed on every device from the CSR arrays (`matrix_sumcheck_witness`)
        polynomials             {label: sonic_pc.ResidentPolynomial}: the twelve index polynomials circuit_{id}_{row,col,row_col,row_col_val}_{a,b,c}
                                (`Circuit::interpolate_matrix_evals`, circuit.rs:142-150), |K_M| coefficients each, no degree or hiding bound
        commitments             with a committer key: their LabeledCommitments in label order (`batch_circuit_setup`, varuna.rs:103-117)

    lg_r, lg_c, lg_x, lg_k[m]: the constraint, variable, input and non-zero domains as `index_helper` sizes them (indexer.rs:178-184)."""

    @classmethod
    def build(cls, a, b, c, num_public, circuit_id, ck=None, device=-1):
        """a, b, c: SparseMatrix of the same shape (rows = constraints, cols = public + private variables); num_public: the padded public
        variables; ck: a sonic_pc.CommitterUnionKey, or None for no verifying key.  Per matrix the four evaluation vectors are ONE
        `snarkvm_hip_fr_arithmetize` into one device block with stride |K_M| and their copy goes through ONE inverse transform batch - every matrix
        enqueued in one scope, the host waits once.  Call it outside a scope."""
        from . import sonic_pc

        mats = [a, b, c]
        if any(m.rows != a.rows or m.cols != a.cols for m in mats):
            raise ValueError("CircuitIndex.build: A, B and C differ in shape")
        if _lib.lib().snarkvm_hip_scope_stream():
            raise ValueError("CircuitIndex.build: call it outside a scope (registration and the commitments wait for the device)")
        self = cls.__new__(cls)
        self.circuit_id, self.device = circuit_id, device
        self.lg_r, self.lg_c, self.lg_x = _domain_lg(a.rows), _domain_lg(a.cols), _domain_lg(num_public)
        _check_subdomain(1 << self.lg_c, 1 << self.lg_x)
        self.lg_k = [_domain_lg(m.nnz) for m in mats]
        self.matrices, self.transposes, self.ariths, self._evals, self._polys = [], [], [], [], []
        self.polynomials, self.commitments, self._pruned = {}, None, False
        try:
            for m, lg in zip(mats, self.lg_k):
                self.matrices.append(RegisteredMatrix(m))
                self.transposes.append(RegisteredMatrix(transpose(m, 1 << self.lg_c, 1 << self.lg_x)))
                self.ariths.append(RegisteredArithmetization.from_csr(m, 1 << lg, self.lg_r, self.lg_c, self.lg_x))
            csr = []
            for m, lg in zip(mats, self.lg_k):
                at_col = (8 * (m.rows + 1) + 31) & ~31
                at_val = (at_col + 4 * m.nnz + 31) & ~31
                mem = HipMem(at_val + 32 * max(m.nnz, 1), device)
                mem.upload(m.row_ptr)
                if m.nnz:
                    mem.upload(m.col_idx, at_col)
                    mem.upload(m.vals, at_val)
                csr.append((mem, at_col, at_val))
                self._evals.append(HipMem(32 * 4 << lg, device))
                self._polys.append(HipMem(32 * 4 << lg, device))
            with _Scope(self._evals[0].ptr):
                for m, lg, (mem, at_col, at_val), ev, po in zip(mats, self.lg_k, csr, self._evals, self._polys):
                    k = 1 << lg
                    plugin.fr_arithmetize_device(*(ev.ptr + 32 * k * j for j in range(4)), k, m.rows, mem.ptr, mem.ptr + at_col, mem.ptr + at_val, self.lg_r, self.lg_c, self.lg_x)
                    po.copy_from(0, ev.ptr, 32 * 4 * k)
                    plugin.NTT_device_batch(lg, [po.ptr + 32 * k * j for j in range(4)], directions=[1] * 4, types=[0] * 4)
            for mem, _, _ in csr:
                mem.free()
            for name, lg, po in zip("abc", self.lg_k, self._polys):
                for j, kind in enumerate(INDEX_KINDS):
                    label = index_label(circuit_id, kind, name)
                    self.polynomials[label] = sonic_pc.ResidentPolynomial(label, po.ptr + (32 * j << lg), 1 << lg)
            if ck is not None:
                ordered = [self.polynomials[label] for label in sorted(self.polynomials)]  # varuna.rs:116 sorts the commitments by label
                self.commitments, _ = sonic_pc.SonicKZG10.commit((1 << max(self.lg_k)) - 1, ck, ordered)
        except Exception:
            self.close()
            raise
        return self

    def evaluate_index_polynomials(self, point, combiners):
        """`evaluate_index_polynomials` (indexer.rs:232-260), the core of prove_vk / verify_vk: per matrix the Lagrange coefficients of K_M at `point`
        in device memory (`snarkvm_hip_fr_lagrange_coefficients`) and the four inner products with the kept evaluation vectors (ONE strided
        `snarkvm_hip_fr_reduce`), all in one scope; the twelve values meet the combiners in label order on the host.  point: (4,) Montgomery limbs,
        combiners: (12, 4).  -> (sonic_pc.LinearCombination "circuit_check", the sum as (4,) Montgomery limbs).  Call it outside a scope."""
        from . import sonic_pc

        if self._pruned:
            raise ValueError("row_col evaluations are not available")  # matrices.rs: MatrixEvals::evaluate
        if _lib.lib().snarkvm_hip_scope_stream():
            raise ValueError("evaluate_index_polynomials: call it outside a scope (the values are needed at once)")
        tau = np.ascontiguousarray(point, dtype=np.uint64).reshape(1, 4)
        combiners = np.ascontiguousarray(combiners, dtype=np.uint64).reshape(-1, 4)
        lags = [HipMem(32 << lg, self.device) for lg in self.lg_k]
        with _Scope(lags[0].ptr):
            values = []
            for lg, ev, lag in zip(self.lg_k, self._evals, lags):
                _lib.check(_lib.lib().snarkvm_hip_fr_lagrange_coefficients(lag.ptr, lg, tau.ctypes.data, 1))
                values.append(plugin.fr_reduce_strided_device(plugin.FR_REDUCE_DOT, ev.ptr, lag.ptr, 1 << lg, 4, 1 << lg, b_shared=True))
        for lag in lags:
            lag.free()
        evals = {index_label(self.circuit_id, kind, name): v[j] for name, v in zip("abc", values) for j, kind in enumerate(INDEX_KINDS)}
        labels = sorted(evals)
        if combiners.shape[0] < len(labels):
            raise ValueError("No combiner left")
        if combiners.shape[0] > len(labels):
            raise ValueError("Found more combiners than sorted_evals")
        lc, total = sonic_pc.LinearCombination.empty("circuit_check"), None
        for label, combiner in zip(labels, combiners):
            lc.add(combiner, label)
            total = sonic_pc._fr_add(total, sonic_pc._fr_mul(evals[label], combiner))
        return lc, total

    def prune_row_col_evals(self):
        """circuit.rs:151-155: the row_col evaluations are not part of a proving key; `evaluate_index_polynomials` is refused afterwards"""
        self._pruned = True

    def close(self):
        """releases the registered objects, the evaluations and the polynomials (every ResidentPolynomial of `polynomials` dangles afterwards);
        safe to call twice"""
        for reg in self.matrices + self.transposes + self.ariths:
            reg.close()
        for mem in self._evals + self._polys:
            mem.free()
        self.matrices, self.transposes, self.ariths, self._evals, self._polys, self.polynomials = [], [], [], [], [], {}

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown / a dead device: nothing left to do
            pass
