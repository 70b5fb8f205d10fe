"""Prover-round polynomial operations on the gfx950 backend (SURVEY.md §8f N2 and the `open` half of row a15).

Host mirror of the reference functions the Varuna prover runs between its NTTs and its commitments:

    DensePolynomial::{evaluate, mul_by_vanishing_poly, divide_by_vanishing_poly}   fft/polynomial/dense.rs:98-114, 153-169
    `polynomial / (X - point)` (Polynomial::divide_with_q_and_r)                    fft/polynomial/mod.rs:222-256
    `poly += (coeff, cur_poly)` over the terms of a linear combination              polycommit/sonic_pc/mod.rs:413-473, 548-564
    apply_randomized_selector summed over the members of round 3 (`selector_fold`)  ahp/selectors.rs:100-121, round_functions/third.rs:179-213
    the gather of calculate_w between its two transforms (`witness_evals`)          round_functions/first.rs:127-161
    the evaluations of z, whose inverse transform yields z, w and x_poly (`assignment_evals`)  first.rs:147-152, fft/domain.rs:322-344
    calculate_rowcheck_witness's sum and divisibility test (`rowcheck_fold`)        round_functions/second.rs:76-142, ahp/selectors.rs:88-99
    Evaluations::evaluate_with_coeffs (an inner product), sums over a domain        fft/evaluations.rs:90-92, round_functions/first.rs:119
    DensePolynomial::{degree, is_zero}, skip_leading_zeros_and_convert_to_bigints   fft/polynomial/dense.rs:66-96, kzg10/mod.rs:455-467
    batch_inversion / batch_inversion_and_mul                                       fields/src/lib.rs:66-129
    EvaluationDomain::{distribute_powers_and_mul_by_const,
                       evaluate_all_lagrange_coefficients}                          fft/domain.rs:224-292

Vectors are (n, 4) u64 arrays of Montgomery limbs (the Rust `Vec<Fr>` memory image); scalars are (4,) / (1, 4).
Every function runs on the device - there is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib

VEC_OPS = {"add": 0, "sub": 1, "mul": 2, "mul_sub": 3, "scale": 4, "sub_scalar": 5, "axpy": 6, "rsub_scalar": 7}


def _v(x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)


def _p(a):
    return a.ctypes.data if a is not None else None


def trim(coeffs):
    """DensePolynomial::from_coefficients_vec (dense.rs:76-86): drop trailing zero coefficients."""
    coeffs = _v(coeffs)
    nz = np.nonzero(coeffs.any(axis=1))[0]
    return coeffs[: (int(nz[-1]) + 1 if nz.size else 0)]


def vec_op(op, a, b=None, c=None, scalar=None):
    """Element-wise Fr arithmetic: add, sub, mul, mul_sub (a*b-c), scale (a*s), sub_scalar (a-s), axpy (a+b*s), rsub_scalar (s-a)."""
    a = _v(a)
    n = a.shape[0]
    b = None if b is None else _v(b)
    c = None if c is None else _v(c)
    for other in (b, c):
        if other is not None and other.shape[0] != n:
            raise ValueError("length mismatch")  # the reference zips with zip_eq
    s = None if scalar is None else _v(scalar)
    out = np.empty_like(a)
    _lib.check(_lib.lib().snarkvm_hip_fr_vec_op(VEC_OPS[op], _p(out), _p(a), _p(b), _p(c), _p(s), n, 0))
    return out


def lincomb(coeffs, polys):
    """sum_k coeffs[k] * polys[k] over polynomials of any lengths in ONE device pass (`snarkvm_hip_fr_lincomb`): what the reference builds
    term by term with `poly += (coeff, cur_poly)` (sonic_pc/mod.rs:427-447, 548-564).  Trimmed like a DensePolynomial."""
    polys = [_v(p) for p in polys]
    k = len(polys)
    cs = _v(coeffs) if k else np.zeros((0, 4), dtype=np.uint64)
    if cs.shape[0] != k:
        raise ValueError("length mismatch")
    n = max([p.shape[0] for p in polys] + [0])
    out = np.empty((n, 4), dtype=np.uint64)
    ptrs = (ctypes.c_void_p * max(1, k))(*[p.ctypes.data if p.shape[0] else None for p in polys])
    lens = (ctypes.c_size_t * max(1, k))(*[p.shape[0] for p in polys])
    _lib.check(_lib.lib().snarkvm_hip_fr_lincomb(_p(out), n, k, ptrs, lens, _p(cs), 0))
    return trim(out)


def open_fold(coeffs, polys, point):
    """(quotient, value) of (sum_k coeffs[k] * polys[k]) / (X - point) in one sweep up and one down (`snarkvm_hip_fr_open_fold`): the combination
    is formed once and never leaves the device.  The same values as `divide_by_linear(lincomb(coeffs, polys), point)` (sonic_pc/mod.rs:286-342
    into kzg10/mod.rs:213-236); the quotient is trimmed like a DensePolynomial, the value is (1, 4)."""
    polys = [_v(p) for p in polys]
    k = len(polys)
    cs = _v(coeffs) if k else np.zeros((0, 4), dtype=np.uint64)
    if cs.shape[0] != k:
        raise ValueError("length mismatch")
    n = max([p.shape[0] for p in polys] + [0])
    q = np.zeros((n, 4), dtype=np.uint64)
    rem = np.zeros((1, 4), dtype=np.uint64)
    ptrs = (ctypes.c_void_p * max(1, k))(*[p.ctypes.data if p.shape[0] else None for p in polys])
    lens = (ctypes.c_size_t * max(1, k))(*[p.shape[0] for p in polys])
    _lib.check(_lib.lib().snarkvm_hip_fr_open_fold(_p(q) if n else None, _p(rem), n, k, ptrs, lens, _p(cs) if k else None, _p(_v(point)), 0))
    return trim(q), rem


def selector_fold(polys, src_sizes, multipliers, target_size, h_len=None, want="hxs"):
    """The sums of Varuna's round 3 over host arrays in ONE device pass (`snarkvm_hip_fr_selector_fold`): per member k the reference scales
    polys[k] by multipliers[k], divides by X^n_k - 1 (n_k = src_sizes[k]), multiplies the remainder by X^target_size - 1 and divides by X^n_k - 1
    again (apply_randomized_selector, selectors.rs:100-121), adds the quotients into h_1 and the tiled remainders into x g_1 (third.rs:179-213) and
    takes the sum of the unscaled member over its source domain (third.rs:317).  -> (h, xg, sums): h of h_len coefficients (default: the longest
    quotient), xg of target_size, sums (len(polys), 4); None for the outputs whose letter is not in `want` ("h", "x", "s").  Untrimmed."""
    polys = [_v(p) for p in polys]
    k = len(polys)
    mu = _v(multipliers) if k else np.zeros((0, 4), dtype=np.uint64)
    if mu.shape[0] != k or len(src_sizes) != k:
        raise ValueError("length mismatch")
    if h_len is None:
        h_len = max([max(p.shape[0] - int(n), 0) for p, n in zip(polys, src_sizes)] + [0])
    h = np.empty((int(h_len), 4), dtype=np.uint64) if "h" in want else None
    xg = np.empty((int(target_size), 4), dtype=np.uint64) if "x" in want else None
    sums = np.empty((k, 4), dtype=np.uint64) if "s" in want else None
    ptrs = (ctypes.c_void_p * max(1, k))(*[p.ctypes.data if p.shape[0] else None for p in polys])
    lens = (ctypes.c_size_t * max(1, k))(*[p.shape[0] for p in polys])
    srcs = (ctypes.c_size_t * max(1, k))(*[int(n) for n in src_sizes])
    nz = lambda a: a.ctypes.data if a is not None and a.size else None
    _lib.check(_lib.lib().snarkvm_hip_fr_selector_fold(nz(h), int(h_len), nz(xg), int(target_size), nz(sums), k, ptrs, lens, srcs, _p(mu), 0))
    return h, xg, sums


def witness_evals(w, x_evals, input_size):
    """The gather of Varuna's round 1 over host arrays in one device pass (`snarkvm_hip_fr_witness_evals`; calculate_w, first.rs:127-161): x_evals =
    the n evaluations of x_poly over the variable domain, w = the private variables (at most n - input_size).  -> (n, 4): zero where
    ratio = n / input_size divides k, w[k - k // ratio - 1] - x_evals[k] elsewhere (w zero past its end)."""
    w, x = _v(w), _v(x_evals)
    n = x.shape[0]
    if int(input_size) <= 0 or n % int(input_size) or w.shape[0] > n - int(input_size):
        raise ValueError("input_size must divide n and w hold at most n - input_size elements")
    out = np.empty_like(x)
    _lib.check(_lib.lib().snarkvm_hip_fr_witness_evals(_p(out) if n else None, n, _p(w) if w.shape[0] else None, w.shape[0], _p(x) if n else None, int(input_size), 0))
    return out


def assignment_evals(rows, n, input_size):
    """The gather of Varuna's round 1 in lock step over host arrays in one device pass (`snarkvm_hip_fr_assignment_evals`): rows = one
    (num_vars, 4) array per instance, or one (instances, num_vars, 4) array - padded_public (input_size values) ++ private.  -> (instances, n, 4):
    the evaluations of every assignment z on the variable domain of n elements, rows[m][k // ratio] where ratio = n / input_size divides k,
    rows[m][input_size + k - k // ratio - 1] elsewhere (zero from num_vars on).  Its inverse transform is z; z div (X^input_size - 1) is w and
    z mod (X^input_size - 1) is x_poly."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    rows = rows.reshape(1, -1, 4) if rows.ndim < 3 else rows.reshape(rows.shape[0], -1, 4)
    count, num_vars, n, input_size = rows.shape[0], rows.shape[1], int(n), int(input_size)
    if input_size <= 0 or n % input_size or not input_size <= num_vars <= max(n, input_size):
        raise ValueError("input_size must divide n and a row hold between input_size and n elements")
    out = np.empty((count, n, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_assignment_evals(_p(out) if out.size else None, n, _p(rows) if rows.size else None, num_vars, input_size, count, n, num_vars, 0))
    return out


def rowcheck_fold(a, b, c, multipliers=None, want="ov"):
    """The sums of Varuna's round 2 over host arrays in ONE device pass (`snarkvm_hip_fr_rowcheck_fold`; calculate_rowcheck_witness,
    second.rs:76-142): a, b, c = one (n, 4) array per member each.  -> (out, violations): out[i] = sum_k multipliers[k] (a_k[i] b_k[i] - c_k[i])
    as (n, 4), violations[k] = the number of i with a_k[i] b_k[i] != c_k[i] as (len(a),) uint64; None for the outputs whose letter is not in `want`
    ("o", "v").  multipliers is needed for "o" only."""
    a, b, c = ([_v(x) for x in xs] for xs in (a, b, c))
    k = len(a)
    n = a[0].shape[0] if k else 0
    if len(b) != k or len(c) != k or any(x.shape[0] != n for x in a + b + c):
        raise ValueError("length mismatch")  # the reference zips with zip_eq
    mu = None
    if "o" in want:
        mu = _v(multipliers) if k else np.zeros((0, 4), dtype=np.uint64)
        if mu.shape[0] != k:
            raise ValueError("length mismatch")
    out = np.empty((n, 4), dtype=np.uint64) if "o" in want else None
    counts = np.zeros(k, dtype=np.uint64) if "v" in want else None
    lists = [(ctypes.c_void_p * max(1, k))(*[x.ctypes.data if n else None for x in xs]) for xs in (a, b, c)]
    nz = lambda v: v.ctypes.data if v is not None and v.size else None
    _lib.check(_lib.lib().snarkvm_hip_fr_rowcheck_fold(nz(out), nz(counts), n, k, lists[0], lists[1], lists[2], nz(mu), 0))
    return out, counts


def inner_product(a, b):
    """sum_i a[i] * b[i] in one device pass (`snarkvm_hip_fr_reduce`, op DOT): Evaluations::evaluate_with_coeffs (evaluations.rs:90-92,
    which zips with zip_eq).  -> (1, 4)."""
    a, b = _v(a), _v(b)
    if a.shape[0] != b.shape[0]:
        raise ValueError("length mismatch")
    out = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_reduce(1, _p(out), _p(a) if a.shape[0] else None, _p(b) if a.shape[0] else None, a.shape[0], 0))
    return out


def vec_sum(a):
    """sum_i a[i] in one device pass (`snarkvm_hip_fr_reduce`, op SUM) -> (1, 4)."""
    a = _v(a)
    out = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_reduce(0, _p(out), _p(a) if a.shape[0] else None, None, a.shape[0], 0))
    return out


def support(v):
    """(trimmed_len, leading_zeros, nonzero) of a coefficient vector in one device pass (`snarkvm_hip_fr_support`): the length
    DensePolynomial::from_coefficients_vec would keep (degree = max(trimmed_len, 1) - 1, is_zero = trimmed_len == 0), the number of leading
    zero coefficients a commitment skips (len(v) for the zero vector), the number of non-zero coefficients."""
    v = _v(v)
    out = np.zeros(3, dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_support(_p(out), _p(v) if v.shape[0] else None, v.shape[0], 0))
    return tuple(int(x) for x in out)


def divide_by_linear(coeffs, point):
    """(quotient, p(point)) of p / (X - point); the quotient is trimmed like a DensePolynomial."""
    coeffs = trim(coeffs)
    n = coeffs.shape[0]
    q = np.zeros((max(n - 1, 0), 4), dtype=np.uint64)
    rem = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_divide_by_linear(_p(q) if n > 1 else None, _p(rem), _p(coeffs), n, _p(_v(point)), 0))
    return trim(q), rem


def evaluate(coeffs, point):
    """DensePolynomial::evaluate (dense.rs:98-114)."""
    coeffs = trim(coeffs)
    rem = np.zeros((1, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_divide_by_linear(None, _p(rem), _p(coeffs), coeffs.shape[0], _p(_v(point)), 0))
    return rem


def batch_inversion_and_mul(v, coeff):
    """fields/src/lib.rs:73-129: returns coeff / v_i (zeros stay zero)."""
    v = np.array(v, dtype=np.uint64, copy=True).reshape(-1, 4)
    _lib.check(_lib.lib().snarkvm_hip_fr_batch_inversion_and_mul(_p(v), v.shape[0], _p(_v(coeff)), 0))
    return v


def distribute_powers_and_mul_by_const(v, g, c):
    """fft/domain.rs:229-254: v_i * c * g^i."""
    v = np.array(v, dtype=np.uint64, copy=True).reshape(-1, 4)
    _lib.check(_lib.lib().snarkvm_hip_fr_distribute_powers(_p(v), v.shape[0], _p(_v(g)), _p(_v(c)), 0))
    return v


def evaluate_all_lagrange_coefficients(domain_size, tau):
    """fft/domain.rs:258-292 for the power-of-two domain of `domain_size` elements."""
    lg = domain_size.bit_length() - 1
    if domain_size <= 0 or 1 << lg != domain_size:
        raise ValueError("domain_size is not power of 2")
    out = np.zeros((domain_size, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_lagrange_coefficients(_p(out), lg, _p(_v(tau)), 0))
    return out


def divide_by_vanishing_poly(coeffs, domain_size):
    """dense.rs:161-169: (quotient, remainder) of p / (X^domain_size - 1), both trimmed."""
    coeffs = trim(coeffs)
    n = coeffs.shape[0]
    if n == 0:
        return coeffs, coeffs
    q = np.zeros((max(n - domain_size, 0), 4), dtype=np.uint64)
    r = np.zeros((min(n, domain_size), 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_divide_by_vanishing(_p(q) if q.shape[0] else None, _p(r), _p(coeffs), n, domain_size, 0))
    return trim(q), trim(r)


def mul_by_vanishing_poly(coeffs, domain_size):
    """dense.rs:153-159: p * (X^domain_size - 1), trimmed."""
    coeffs = _v(coeffs)
    out = np.zeros((coeffs.shape[0] + domain_size, 4), dtype=np.uint64)
    _lib.check(_lib.lib().snarkvm_hip_fr_mul_by_vanishing(_p(out), _p(coeffs) if coeffs.shape[0] else None, coeffs.shape[0], domain_size, 0))
    return trim(out)
