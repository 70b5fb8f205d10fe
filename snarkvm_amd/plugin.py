"""Mirror of the reference's accelerator plugin crate `snarkvm_algorithms_cuda` (algorithms/cuda/src/lib.rs:77-168):
the three functions `NTT`, `polymul`, `msm` with the same names, argument meaning and error behaviour
(`Err(cuda::Error)` becomes `HipError`; a length mismatch panics / raises before the FFI call), bound to the
C ABI of libsnarkvm_hip.so.  Data crosses the boundary as numpy views of the Rust memory layouts
(snarkvm_amd.layout)."""
import ctypes

import numpy as np

from . import _lib
from .layout import G1_AFFINE, G1_PROJECTIVE, NTTDirection, NTTInputOutputOrder, NTTType

__all__ = ["NTT", "polymul", "polymul_device", "fr_lincomb_device", "FR_LINCOMB_CHUNK", "fr_open_fold_device", "fr_selector_fold_device", "FR_SELECTOR_CHUNK", "fr_witness_evals_device", "fr_assignment_evals_device", "fr_rowcheck_fold_device", "FR_ROWCHECK_CHUNK", "fr_reduce_device", "fr_reduce_strided_device", "fr_support_device", "fr_support_strided_device", "FR_REDUCE_SUM", "FR_REDUCE_DOT", "fr_evaluate_device", "fr_evaluate", "FR_EVALUATE_MEMBERS", "FR_EVALUATE_POINTS","fr_spmv_device", "fr_sumcheck_evals_device", "fr_sumcheck_evals", "fr_arithmetize_device", "fr_arithmetize", "msm", "set_base_cache", "base_cache_stats", "NTTInputOutputOrder", "NTTDirection", "NTTType"]


def _ptr(a):
    return a.ctypes.data


def NTT(domain_size, inout, ntt_order, ntt_direction, ntt_type):
    """lib.rs:77-97.  In-place NTT of `inout` ((domain_size, 4) u64 Montgomery limbs, C-contiguous)."""
    if domain_size & (domain_size - 1):
        raise ValueError("domain_size is not power of 2")  # lib.rs:84-86 panics
    if not (isinstance(inout, np.ndarray) and inout.dtype == np.uint64 and inout.flags.c_contiguous and inout.size == 4 * domain_size):
        raise ValueError("inout must be a C-contiguous uint64 array of domain_size x 4 limbs")
    lg = domain_size.bit_length() - 1
    err = _lib.lib().snarkvm_ntt(_ptr(inout), lg, ntt_order, ntt_direction, ntt_type)
    _lib.check(err)


def NTT_device_batch(lg, device_ptrs, directions=None, types=None, ntt_order=0):
    """Extension (no reference counterpart): `len(device_ptrs)` independent in-place transforms of 2^lg elements over device
    vectors, one enqueue and one synchronisation (`snarkvm_hip_ntt_device_batch`).  directions / types: per vector or None."""
    k = len(device_ptrs)
    if k == 0:
        return
    ptrs = (ctypes.c_void_p * k)(*[int(p) for p in device_ptrs])
    dirs = (ctypes.c_int * k)(*[int(d) for d in directions]) if directions is not None else None
    tys = (ctypes.c_int * k)(*[int(t) for t in types]) if types is not None else None
    _lib.check(_lib.lib().snarkvm_hip_ntt_device_batch(ptrs, k, lg, ntt_order, dirs, tys))


def polymul(domain, polynomials, evaluations, zero=None):
    """lib.rs:100-145.  Returns the product as a (domain, 4) array (full domain length; the reference trims
    trailing zeros afterwards in DensePolynomial::from_coefficients_vec, multiplier.rs:93)."""
    if domain & (domain - 1):
        raise ValueError("domain_size is not power of 2")
    lg = domain.bit_length() - 1
    polys = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polynomials]
    evals = [np.ascontiguousarray(e, dtype=np.uint64).reshape(-1, 4) for e in evaluations]
    out = np.zeros((domain, 4), dtype=np.uint64)  # lib.rs:126-127: pre-filled with `zero`
    pp = (ctypes.c_void_p * max(1, len(polys)))(*[p.ctypes.data for p in polys])
    pl = (ctypes.c_size_t * max(1, len(polys)))(*[p.shape[0] for p in polys])
    ep = (ctypes.c_void_p * max(1, len(evals)))(*[e.ctypes.data for e in evals])
    el = (ctypes.c_size_t * max(1, len(evals)))(*[e.shape[0] for e in evals])
    err = _lib.lib().snarkvm_polymul(_ptr(out), len(polys), pp, pl, len(evals), ep, el, lg)
    _lib.check(err)
    return out


def polymul_device(lg, out_ptr, polys=(), evals=()):
    """Extension (no reference counterpart): `polymul` over operands that live in device memory and stay there
    (`snarkvm_hip_polymul_device`).  out_ptr: device vector of 2^lg elements, all of it written; polys: (device pointer, length) pairs
    of coefficient-form operands, length <= 2^lg; evals: device pointers of evaluation vectors of 2^lg elements.  No operand is written;
    out_ptr may be the start of one of them.  Inside a scope the call is only enqueued."""
    polys = [(int(p), int(n)) for p, n in polys]
    evals = [int(e) for e in evals]
    pp = (ctypes.c_void_p * max(1, len(polys)))(*[p for p, _ in polys])
    pl = (ctypes.c_size_t * max(1, len(polys)))(*[n for _, n in polys])
    ep = (ctypes.c_void_p * max(1, len(evals)))(*evals)
    el = (ctypes.c_size_t * max(1, len(evals)))(*([1 << lg] * len(evals)))
    _lib.check(_lib.lib().snarkvm_hip_polymul_device(int(out_ptr), len(polys), pp, pl, len(evals), ep, el, lg))


FR_LINCOMB_CHUNK = 24  # operands per kernel launch of snarkvm_hip_fr_lincomb (include/snarkvm_hip.h; csrc/poly.hip.h FR_LINCOMB_CHUNK)


def fr_lincomb_device(d_out, n_out, d_polys, lens, coeffs):
    """Extension (no reference counterpart): d_out[i] = sum_k coeffs[k] * d_polys[k][i] for i < n_out over vectors that live in device memory
    (`snarkvm_hip_fr_lincomb`, on_device = 1); d_polys[k] counts as zero from lens[k] <= n_out on.  coeffs: (k, 4) Montgomery limbs on the
    host.  No operand is written; d_out may be the start of one of them.  Inside a scope the call is only enqueued."""
    k = len(d_polys)
    if len(lens) != k:
        raise ValueError("length mismatch")
    cs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4) if k else np.zeros((0, 4), dtype=np.uint64)
    if cs.shape[0] != k:
        raise ValueError("length mismatch")
    pp = (ctypes.c_void_p * max(1, k))(*[int(p) if p else None for p in d_polys])
    pl = (ctypes.c_size_t * max(1, k))(*[int(n) for n in lens])
    _lib.check(_lib.lib().snarkvm_hip_fr_lincomb(int(d_out) if d_out else None, int(n_out), k, pp, pl, _ptr(cs), 1))


def fr_open_fold_device(d_quot, n, d_polys, lens, coeffs, point, remainder=True):
    """Extension (no reference counterpart): the opening fold over vectors that live in device memory (`snarkvm_hip_fr_open_fold`, on_device = 1).
    With comb[i] = sum_k coeffs[k] * d_polys[k][i] for i < n (d_polys[k] counts as zero from lens[k] <= n on), formed once:
        d_quot[i] = sum_{j > i} comb[j] * point^(j - i - 1)   for i < n: comb / (X - point) in the first n - 1 elements, then a zero
                    (skipped when d_quot is None: the value alone)
        value     = comb(point)                                (skipped with remainder=False)
    coeffs: (k, 4) Montgomery limbs on the host, point: (4,).  -> the value as a (1, 4) array, or None.  No operand is written and none may
    overlap d_quot.  Inside a scope the call is only enqueued and the returned array is filled when the scope ends: keep it alive until then."""
    k = len(d_polys)
    if len(lens) != k:
        raise ValueError("length mismatch")
    cs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4) if k else np.zeros((0, 4), dtype=np.uint64)
    if cs.shape[0] != k:
        raise ValueError("length mismatch")
    z = _fr_scalar(point)
    pp = (ctypes.c_void_p * max(1, k))(*[int(p) if p else None for p in d_polys])
    pl = (ctypes.c_size_t * max(1, k))(*[int(x) for x in lens])
    out = np.zeros((1, 4), dtype=np.uint64) if remainder else None
    _lib.check(_lib.lib().snarkvm_hip_fr_open_fold(int(d_quot) if d_quot else None, _ptr(out) if remainder else None, int(n), k, pp, pl, _ptr(cs) if k else None,
                                                   _ptr(z), 1))
    return out


FR_SELECTOR_CHUNK = 24  # members per kernel launch of snarkvm_hip_fr_selector_fold (include/snarkvm_hip.h; csrc/poly.hip.h FR_SELECTOR_CHUNK)


def fr_selector_fold_device(d_h, h_len, d_xg, target_size, d_sums, d_polys, lens, src_sizes, multipliers):
    """Extension (no reference counterpart): the sums of Varuna's round 3 over members that live in device memory (`snarkvm_hip_fr_selector_fold`,
    on_device = 1; third.rs:280-327 with apply_randomized_selector, selectors.rs:100-121).  Member k = d_polys[k] (lens[k] coefficients) with source
    domain src_sizes[k] and multiplier multipliers[k] ((k, 4) Montgomery limbs on the host):
        d_h[i]  = sum_k mu_k sum_{j >= 1} p_k[i + j n_k]            i < h_len
        d_xg[i] = sum_k mu_k sum_{j >= 0} p_k[(i mod n_k) + j n_k]  i < target_size
        d_sums[k] = n_k sum_j p_k[j n_k]                             (len(d_polys) elements of device memory, not scaled by mu_k)
    Each of d_h, d_xg and d_sums may be None (skipped).  No member is written.  Inside a scope the call is only enqueued."""
    k = len(d_polys)
    if len(lens) != k or len(src_sizes) != k:
        raise ValueError("length mismatch")
    mu = np.ascontiguousarray(multipliers, dtype=np.uint64).reshape(-1, 4) if k else np.zeros((0, 4), dtype=np.uint64)
    if mu.shape[0] != k:
        raise ValueError("length mismatch")
    pp = (ctypes.c_void_p * max(1, k))(*[int(p) if p else None for p in d_polys])
    pl = (ctypes.c_size_t * max(1, k))(*[int(n) for n in lens])
    ps = (ctypes.c_size_t * max(1, k))(*[int(n) for n in src_sizes])
    _lib.check(_lib.lib().snarkvm_hip_fr_selector_fold(int(d_h) if d_h else None, int(h_len), int(d_xg) if d_xg else None, int(target_size),
                                                       int(d_sums) if d_sums else None, k, pp, pl, ps, _ptr(mu), 1))


def fr_witness_evals_device(d_out, n, d_w, w_len, d_x_evals, input_size):
    """Extension (no reference counterpart): the gather of Varuna's round 1 over vectors that live in device memory (`snarkvm_hip_fr_witness_evals`,
    on_device = 1; first.rs:127-161).  With ratio = n / input_size: d_out[k] = 0 when ratio divides k, d_w[k - k // ratio - 1] - d_x_evals[k]
    otherwise; d_w counts as zero from w_len <= n - input_size on.  d_out may equal d_x_evals (in place).  Inside a scope the call is only
    enqueued."""
    n, w_len, input_size = int(n), int(w_len), int(input_size)
    if input_size <= 0 or n % input_size:
        raise ValueError("input_size must divide n")
    if w_len < 0 or w_len > n - input_size:
        raise ValueError("w is longer than n - input_size")
    _lib.check(_lib.lib().snarkvm_hip_fr_witness_evals(_dp(d_out), n, _dp(d_w) if w_len else None, w_len, _dp(d_x_evals), input_size, 1))


def fr_assignment_evals_device(d_out, n, d_vars, num_vars, input_size, count=1, stride_out=0, stride_vars=0):
    """Extension (no reference counterpart): the gather of Varuna's round 1 in lock step over rows that live in device memory
    (`snarkvm_hip_fr_assignment_evals`, on_device = 1).  Member m reads the row d_vars + m * stride_vars - padded_public (input_size values) ++
    private (num_vars - input_size values), the x operand of `fr_spmv_device` - and writes the n evaluations of its assignment z on the variable
    domain to d_out + m * stride_out (strides in elements): with ratio = n / input_size, row[k // ratio] when ratio divides k,
    row[input_size + k - k // ratio - 1] elsewhere, zero from num_vars on.  d_out must not overlap d_vars.  Inside a scope the call is only
    enqueued."""
    _lib.check(_lib.lib().snarkvm_hip_fr_assignment_evals(_dp(d_out), int(n), _dp(d_vars), int(num_vars), int(input_size), int(count), int(stride_out), int(stride_vars), 1))


FR_ROWCHECK_CHUNK = 24  # members per kernel launch of snarkvm_hip_fr_rowcheck_fold (include/snarkvm_hip.h; csrc/poly.hip.h FR_ROWCHECK_CHUNK)


def fr_rowcheck_fold_device(d_out, n, d_a, d_b, d_c, multipliers, violations=True):
    """Extension (no reference counterpart): the sums of Varuna's round 2 over members that live in device memory (`snarkvm_hip_fr_rowcheck_fold`,
    on_device = 1; second.rs:76-142 with apply_randomized_selector, selectors.rs:88-99).  Member k = the n-element vectors d_a[k], d_b[k], d_c[k]
    with multiplier multipliers[k] ((k, 4) Montgomery limbs on the host; may be None when d_out is None):
        d_out[i]      = sum_k mu_k (a_k[i] b_k[i] - c_k[i])          i < n        (skipped when d_out is None: the check alone)
        violations[k] = the number of i < n with a_k[i] b_k[i] != c_k[i]           (skipped with violations=False: the fold alone)
    -> the counts as a (len(d_a),) uint64 array, or None.  No member is written.  Inside a scope the call is only enqueued and the returned array
    is filled when the scope ends: keep it alive until then."""
    k = len(d_a)
    if len(d_b) != k or len(d_c) != k:
        raise ValueError("length mismatch")
    mu = None
    if d_out:
        mu = np.ascontiguousarray(multipliers, dtype=np.uint64).reshape(-1, 4) if k else np.zeros((0, 4), dtype=np.uint64)
        if mu.shape[0] != k:
            raise ValueError("length mismatch")
    counts = np.zeros(k, dtype=np.uint64) if violations else None
    lists = [(ctypes.c_void_p * max(1, k))(*[_dp(p) for p in ps]) for ps in (d_a, d_b, d_c)]
    _lib.check(_lib.lib().snarkvm_hip_fr_rowcheck_fold(_dp(d_out), _ptr(counts) if violations and k else None, int(n), k, lists[0], lists[1], lists[2],
                                                       _ptr(mu) if mu is not None and k else None, 1))
    return counts


FR_REDUCE_SUM, FR_REDUCE_DOT = 0, 1  # include/snarkvm_hip.h: SNARKVM_HIP_FR_REDUCE_*


def _dp(p):
    return int(p) if p else None


def fr_reduce_device(op, d_a, d_b, n):
    """Extension (no reference counterpart): sum_i a[i] (op FR_REDUCE_SUM, d_b ignored) or sum_i a[i] * b[i] (FR_REDUCE_DOT) over n-element
    vectors that live in device memory (`snarkvm_hip_fr_reduce`, on_device = 1) -> (1, 4) Montgomery limbs on the host.  No operand is
    written; d_a may equal d_b.  Inside a scope the call is only enqueued and the returned array is filled when the scope ends: keep it
    alive until then."""
    out = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_reduce(int(op), _ptr(out), _dp(d_a), _dp(d_b), int(n), 1))
    return out


def fr_reduce_strided_device(op, d_a, d_b, n, count, stride, b_shared=False):
    """The same over `count` vectors `stride` >= n elements apart (`snarkvm_hip_fr_reduce_strided`) -> (count, 4).  b_shared: every member
    is multiplied by the one vector at d_b (the three `evaluate_with_coeffs` of one matrix); otherwise d_b advances like d_a."""
    out = np.zeros((int(count), 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_reduce_strided(int(op), _ptr(out), _dp(d_a), _dp(d_b), int(n), int(count), int(stride), 1 if b_shared else 0))
    return out


def fr_support_device(d_v, n):
    """Extension: (trimmed_len, leading_zeros, nonzero) of an n-element device vector as a (3,) uint64 array (`snarkvm_hip_fr_support`,
    on_device = 1): index of the last non-zero element + 1 (0: the zero vector), index of the first non-zero element (n: the zero vector),
    number of non-zero elements.  Inside a scope the array is filled when the scope ends."""
    out = np.zeros(3, dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_support(_ptr(out), _dp(d_v), int(n), 1))
    return out


def fr_support_strided_device(d_v, n, count, stride):
    """The same over `count` vectors `stride` >= n elements apart (`snarkvm_hip_fr_support_strided`) -> (count, 3) uint64."""
    out = np.zeros((int(count), 3), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_support_strided(_ptr(out), _dp(d_v), int(n), int(count), int(stride)))
    return out


FR_EVALUATE_MEMBERS, FR_EVALUATE_POINTS = 64, 3  # members / distinct points per kernel launch of snarkvm_hip_fr_evaluate (csrc/poly.hip.h)


def _fr_evaluate(ptrs, lens, points, on_device):
    k = len(ptrs)
    if len(lens) != k:
        raise ValueError("length mismatch")
    zs = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4) if k else np.zeros((0, 4), dtype=np.uint64)
    if zs.shape[0] != k:
        raise ValueError("length mismatch")
    out = np.zeros((k, 4), dtype=np.uint64)
    pp = (ctypes.c_void_p * max(1, k))(*ptrs)
    pl = (ctypes.c_size_t * max(1, k))(*[int(n) for n in lens])
    _lib.check(_lib.lib().snarkvm_hip_fr_evaluate(_ptr(out), k, pp, pl, _ptr(zs), on_device))
    return out


def fr_evaluate_device(d_polys, lens, points):
    """Extension (no reference counterpart): result[k] = sum_{i < lens[k]} d_polys[k][i] * points[k]^i over coefficient vectors that live in device
    memory (`snarkvm_hip_fr_evaluate`, on_device = 1; DensePolynomial::evaluate, dense.rs:98-114) -> (len(d_polys), 4) Montgomery limbs on the
    host.  points: (k, 4) Montgomery limbs on the host, one per member; equal points share their powers.  Members may repeat and overlap; none
    is written; a member of length 0 may be None.  Inside a scope the call is only enqueued and the returned array is filled when the scope
    ends: keep it alive until then."""
    return _fr_evaluate([_dp(p) for p in d_polys], lens, points, 1)


def fr_evaluate(polys, points):
    """The same on host arrays (on_device = 0): polys[k] an (n_k, 4) array of coefficients -> (len(polys), 4).  Every distinct buffer is
    uploaded once; the values are there on return."""
    ps = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
    return _fr_evaluate([p.ctypes.data if p.shape[0] else None for p in ps], [p.shape[0] for p in ps], points, 0)


def fr_spmv_device(handle, d_y, n_out, d_x, count=1, stride_x=0, stride_y=0):
    """Extension (no reference counterpart): y = M x over a matrix registered with `snarkvm_hip_fr_matrix_register` (`handle`: its address, see
    matrices.RegisteredMatrix) and vectors that live in device memory (`snarkvm_hip_fr_spmv`, on_device = 1).  All n_out >= rows elements of y are
    written, the tail as zeros.  Member m of a batch reads d_x + m * stride_x elements (stride_x = 0: the one shared x) and writes
    d_y + m * stride_y.  y must not overlap x.  Inside a scope the call is only enqueued."""
    _lib.check(_lib.lib().snarkvm_hip_fr_spmv(_dp(d_y), int(n_out), _dp(handle), _dp(d_x), int(count), int(stride_x), int(stride_y), 1))


def _fr_scalar(x, n=1):
    v = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    if v.shape[0] != n:
        raise ValueError("length mismatch")
    return v


def _ptr_list(ptrs, count):
    if ptrs is None:
        return None
    if len(ptrs) != count:
        raise ValueError("length mismatch")
    return (ctypes.c_void_p * max(1, count))(*[_dp(p) for p in ptrs])


def fr_sumcheck_evals_device(handles, d_a, d_b, d_f, alpha, beta, scales):
    """Extension (no reference counterpart): the evaluations on K of a, b and f of the Varuna matrix sumcheck (round_functions/fourth.rs:155-245)
    for `len(handles)` <= 16 arithmetizations registered with `snarkvm_hip_fr_arith_register` (`handles`: their addresses, see
    matrices.RegisteredArithmetization) into device vectors, in one launch (`snarkvm_hip_fr_matrix_sumcheck_evals`, on_device = 1).  d_a, d_b, d_f:
    one device pointer per member (k_m elements are written), a None entry or a None list skips that output.  alpha, beta: (4,) Montgomery limbs on
    the host; scales: (3, 4) = a_scale, b_scale, f_scale.  Inside a scope the call is only enqueued."""
    k = len(handles)
    hs = (ctypes.c_void_p * max(1, k))(*[_dp(h) for h in handles])
    al, be, sc = _fr_scalar(alpha), _fr_scalar(beta), _fr_scalar(scales, 3)
    _lib.check(_lib.lib().snarkvm_hip_fr_matrix_sumcheck_evals(hs, k, _ptr_list(d_a, k), _ptr_list(d_b, k), _ptr_list(d_f, k), _ptr(al), _ptr(be), _ptr(sc), 1))


def fr_sumcheck_evals(handles, sizes, alpha, beta, scales, want="abf"):
    """The same on host arrays (on_device = 0): -> three lists (a, b, f) of (sizes[m], 4) arrays, None for the outputs not in `want`.  sizes[m]: the k
    the m-th handle was registered with."""
    k = len(handles)
    if len(sizes) != k:
        raise ValueError("length mismatch")
    hs = (ctypes.c_void_p * max(1, k))(*[_dp(h) for h in handles])
    al, be, sc = _fr_scalar(alpha), _fr_scalar(beta), _fr_scalar(scales, 3)
    outs = {w: [np.zeros((int(n), 4), dtype=np.uint64) for n in sizes] if w in want else None for w in "abf"}
    lists = [(ctypes.c_void_p * max(1, k))(*[o.ctypes.data if o.size else None for o in outs[w]]) if outs[w] is not None else None for w in "abf"]
    _lib.check(_lib.lib().snarkvm_hip_fr_matrix_sumcheck_evals(hs, k, lists[0], lists[1], lists[2], _ptr(al), _ptr(be), _ptr(sc), 0))
    return outs["a"], outs["b"], outs["f"]


def fr_arithmetize_device(d_row, d_col, d_row_col, d_row_col_val, k, rows, d_row_ptr, d_col_idx, d_vals, lg_constraint, lg_variable, lg_input):
    """Extension (no reference counterpart): the arithmetization on K of a CSR matrix that lives in device memory (`snarkvm_hip_fr_arithmetize`,
    on_device = 1; `matrix_evals` of ahp/matrices.rs:138-195).  d_row_ptr: rows + 1 uint64, d_col_idx: uint32 and d_vals: Montgomery limbs per entry.
    For entry e = (val, j) of row i: d_row[e] = w_R^i, d_col[e] = w_C^reindex_by_subdomain(j), d_row_col[e] their product, d_row_col_val[e] = val
    times it; the places from the number of entries up to k hold (1, 1, 1, 0).  Each output (k elements) may be None (skipped).  The contents of the
    CSR arrays are the caller's contract (include/snarkvm_hip.h).  Inside a scope the call is only enqueued."""
    _lib.check(_lib.lib().snarkvm_hip_fr_arithmetize(_dp(d_row), _dp(d_col), _dp(d_row_col), _dp(d_row_col_val), int(k), int(rows), _dp(d_row_ptr), _dp(d_col_idx),
                                                     _dp(d_vals), int(lg_constraint), int(lg_variable), int(lg_input), 1))


def fr_arithmetize(k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, want=("row", "col", "row_col", "row_col_val")):
    """The same on host arrays (on_device = 0): -> (row, col, row_col, row_col_val) as (k, 4) arrays, None for the outputs not in `want`."""
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64).reshape(-1)
    col_idx = np.ascontiguousarray(col_idx, dtype=np.uint32).reshape(-1)
    vals = np.ascontiguousarray(vals, dtype=np.uint64).reshape(-1, 4)
    if row_ptr.shape[0] != int(rows) + 1 or col_idx.shape[0] != vals.shape[0]:
        raise ValueError("length mismatch")
    outs = [np.zeros((int(k), 4), dtype=np.uint64) if w in want else None for w in ("row", "col", "row_col", "row_col_val")]
    p = lambda x: _ptr(x) if x is not None and x.size else None  # noqa: E731
    _lib.check(_lib.lib().snarkvm_hip_fr_arithmetize(p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), int(k), int(rows), _ptr(row_ptr), p(col_idx), p(vals),
                                                     int(lg_constraint), int(lg_variable), int(lg_input), 0))
    return tuple(outs)


def msm(points, scalars):
    """lib.rs:148-168.  points: G1_AFFINE array (Rust layout, 104 B stride); scalars: (n, 4) u64 canonical
    integers.  npoints = len(scalars); fewer points than scalars is the caller's bug (lib.rs:150-152 panics)."""
    points = np.ascontiguousarray(points, dtype=G1_AFFINE).reshape(-1)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    npoints = scalars.shape[0]
    if npoints > points.shape[0]:
        raise ValueError(f"length mismatch {points.shape[0]} points < {npoints} scalars")
    ret = np.zeros(1, dtype=G1_PROJECTIVE)
    err = _lib.lib().snarkvm_msm(_ptr(ret), _ptr(points), npoints, _ptr(scalars), G1_AFFINE.itemsize)
    _lib.check(err)
    return ret


BASE_CACHE_STATS = ("lookups", "hits", "registrations", "mismatches", "bytes_compared", "wait_us", "tables", "verified")


def set_base_cache(tables, verified=False):
    """Extension: the API form of SNARKVM_HIP_BASE_CACHE for `msm` (snarkvm_hip_set_base_cache / _verified).  tables 0 (off, drops every
    cached range), 1, 2, 4, 8 or 16; verified=True compares every byte of every hit with a host copy taken at registration, so the
    caller need not promise that its base vector never changes.  Overrides the environment; needs no device."""
    L = _lib.lib()
    fn = L.snarkvm_hip_set_base_cache_verified if verified else L.snarkvm_hip_set_base_cache
    _lib.check(fn(int(tables)))


def base_cache_stats(reset=False):
    """Extension: what the base cache of `msm` did since the last reset (snarkvm_hip_base_cache_stats) as a dict with the keys of
    BASE_CACHE_STATS; reset=True clears the counters (not `tables` / `verified`, the mode in effect)."""
    v = (ctypes.c_uint64 * 8)()
    _lib.lib().snarkvm_hip_base_cache_stats(v, 1 if reset else 0)
    return dict(zip(BASE_CACHE_STATS, (int(x) for x in v)))
