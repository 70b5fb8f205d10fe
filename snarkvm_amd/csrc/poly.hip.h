// poly.hip.h - the prover-round Fr vector kernels that sit between the NTTs and the MSMs (SURVEY.md §8 N2 and the
// `open` half of row a15).  All of them are O(n) streaming passes over 32-byte Fr elements in the reference's memory
// form (a * 2^256 mod r), so that data produced by an NTT can feed a commitment without leaving HBM:
//
//   fr_vec_op_kernel            a+b, a-b, a*b, a*b-c, a*s, a-s, a+b*s, s-a       second.rs:104-122 (rowcheck), kzg10/mod.rs:295-300
//   fr_horner(2)_up/down_kernel suffix Horner sums h_i = sum_{k>=i} a_k z^(k-i)  -> p / (X - z) and p(z); templates over a span policy
//                                                                                 kzg10/mod.rs:213-236, dense.rs:98-114
//   fr_batch_inverse_kernel     v_i <- coeff / v_i, zeros stay zero              fields/src/lib.rs:66-129
//   fr_distribute_powers_kernel v_i <- v_i * c * g^i                             fft/domain.rs:224-254
//   fr_fold_vanishing_kernel    quotient / remainder by X^D - 1                  dense.rs:161-169 (divide_by_vanishing_poly)
//   fr_mul_vanishing_kernel     p * (X^D - 1)                                    dense.rs:153-159
//   fr_selector_fold_kernel     sum_k mu_k (quotient, tiled remainder) of p_k by X^n_k - 1, and the sums over the n_k-th roots
//                                                                                 third.rs:126-327, selectors.rs:100-121 (round 3)
//   fr_witness_evals_kernel     w's evaluations on the variable domain: the interleaving gather minus x     first.rs:127-161 (round 1)
//   fr_assignment_evals_kernel  z's evaluations on the variable domain: public and private variables interleaved   first.rs:127-161, fft/domain.rs:322-344 (round 1, lock step)
//   fr_rowcheck_fold_kernel     sum_k mu_k (a_k b_k - c_k) and the per-member counts of a_k b_k != c_k      second.rs:76-142, selectors.rs:88-99 (round 2)
//   fr_lincomb_kernel           sum_k c_k p_k over ragged lengths, one pass          sonic_pc/mod.rs:413-473, 548-564 (open_combinations)
//   fr_span_fold_t              (sum_k c_k p_k) / (X - z) and its value at z, the combination formed once: the same sweeps over the fold's policy
//                                                                                 sonic_pc/mod.rs:286-342, varuna.rs:572-605
//   fr_reduce_kernel            sum_i a_i, sum_i a_i b_i -> one element              fft/evaluations.rs:85-92 (evaluate_with_coeffs), first.rs:119
//   fr_support_kernel           trimmed length, leading zeros, non-zero count        dense.rs:66-96 (degree, is_zero), kzg10/mod.rs:455-467
//   fr_spmv_seg_kernel          y = M x over a registered CSR matrix, segment by segment  round_functions/mod.rs:131-188 (z_M), third.rs:303-306 (M(alpha, .))
//   fr_sumcheck_evals_kernel    a, b, f of the matrix sumcheck on K over a registered arithmetization  round_functions/fourth.rs:155-245
//
// Representation note (ff.hip.h): the raw memory limbs of a, read as an internal value, are the internal Montgomery form of
// a * 2^-5 ("shifted").  Sums and differences of shifted values are shifted values; the product of a TRUE internal
// value (x.from_mem_mont()) with a shifted value is the shifted product.  So a kernel converts only its broadcast
// operand (z, g, c, coeff) and streams the vectors untouched; only a product of two vector elements needs one fix-up.
#pragma once
#include "ff.hip.h"

namespace sv {

enum { FR_OP_ADD = 0, FR_OP_SUB = 1, FR_OP_MUL = 2, FR_OP_MUL_SUB = 3, FR_OP_SCALE = 4, FR_OP_SUB_SCALAR = 5, FR_OP_AXPY = 6, FR_OP_RSUB_SCALAR = 7 };

// Strided batches (lock-step proving: the same pass over vector v of every proof of a batch): blockIdx.y selects the vector, every
// vector operand of batch member y starts `stride` elements after that of member y - 1.  A single call is a batch of one.
static __global__ void fr_vec_op_kernel(int op, fr_mem_t* out, const fr_mem_t* a, const fr_mem_t* b, const fr_mem_t* c, fr_mem_t s_mem, size_t n, size_t stride) {
    {
        const size_t off = (size_t)blockIdx.y * stride;
        out += off, a += off;
        if (b) b += off;
        if (c) c += off;
    }
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    const fr_t s_shift = fr_t::load(&s_mem);
    const fr_t s = (op == FR_OP_SCALE || op == FR_OP_AXPY) ? s_shift.from_mem_mont() : s_shift;
    for (; i < n; i += st) {
        const fr_t x = fr_t::load(&a[i]);
        fr_t r;
        switch (op) {
            case FR_OP_ADD: r = x + fr_t::load(&b[i]); break;
            case FR_OP_SUB: r = x - fr_t::load(&b[i]); break;
            case FR_OP_MUL: r = (x * fr_t::load(&b[i])).from_mem_mont(); break;
            case FR_OP_MUL_SUB: r = (x * fr_t::load(&b[i])).from_mem_mont() - fr_t::load(&c[i]); break;
            case FR_OP_SCALE: r = x * s; break;
            case FR_OP_SUB_SCALAR: r = x - s; break;
            case FR_OP_AXPY: r = x + fr_t::load(&b[i]) * s; break;
            default: r = s - x; break;
        }
        r.store(&out[i]);
    }
}

// ---- suffix Horner sums --------------------------------------------------------------------------------------------
// h_i = sum_{k >= i} a_k m^(k-i) satisfies h_i = a_i + m h_(i+1): a linear recurrence, parallelised over chunks of
// POLY_CHUNK consecutive coefficients.  `up` evaluates each chunk on its own (cv_t = chunk polynomial at m); the chunk
// values form the same problem with multiplier m^POLY_CHUNK (solved recursively, api_poly.hip: fr_horner_sweep); `down` replays
// each chunk from its incoming carry h_(end of chunk) and writes every h_i.  A thread walks its chunk downwards, so consecutive
// reads of one thread share a cache line.
static constexpr int POLY_CHUNK = 32;

// mult[k] = m^(POLY_CHUNK^k), memory form, k < levels (single thread: a handful of multiplications)
static __global__ void fr_horner_multipliers_kernel(fr_mem_t m_mem, fr_mem_t* mult, int levels) {
    if (blockIdx.x | threadIdx.x) return;
    fr_t m = fr_t::load(&m_mem).from_mem_mont();
    for (int k = 0; k < levels; k++) {
        m.to_mem_mont().store(&mult[k]);
        m = m.pow_u64(POLY_CHUNK);
    }
}

// The sweeps are written once, as scaffolds over a SPAN POLICY: a small struct, passed by kernel argument, that says how a thread walks its own
// span [lo, hi) of the coefficients.  The scaffold owns everything around the walk - which span is whose, the chunk values or the workgroup's
// scan, a thread's incoming h, where h_0 goes.  A policy offers
//   at(y)                  the policy of batch member y (blockIdx.y of the strided entry points)
//   up(m, lo, hi)          -> sum_(lo <= i < hi) a_i m^(i - lo), the span's polynomial at m
//   down(m, h_hi, lo, hi)  -> h_lo, every h_i of the span delivered on the way
// all SV_HD, so the host replay (snarkvm_hip_selftest_fr_open_fold) runs the same bodies.  fr_span_plain_t: the division of a vector;
// fr_span_fold_t (below, with the opening fold): the division of a combination formed on the way.

// The span of the thread that owns coefficients th C .. th C + C - 1 of n; empty, at n, behind the end.
struct fr_horner_span_t {
    size_t lo, hi;
    SV_HD bool empty() const { return lo == hi; }
};
SV_HD fr_horner_span_t fr_horner_span(size_t th, size_t C, size_t n) {
    const size_t lo = th * C < n ? th * C : n;
    return {lo, lo + C < n ? lo + C : n};
}
// reads in[i], writes out[i - shift] = h_i for i >= shift (the quotient by X - m is shift 1: q_(i-1) = h_i, and h_0 the remainder, which the
// scaffold delivers).  in == out is allowed when shift == 0: the levels above the input run in place.  `out` is not read by `up`.
struct fr_span_plain_t {
    const fr_mem_t* in;
    fr_mem_t* out;
    size_t in_stride, out_stride;
    int shift;
    SV_HD fr_span_plain_t at(size_t y) const { return {in + y * in_stride, out ? out + y * out_stride : nullptr, in_stride, out_stride, shift}; }
    SV_HD fr_t up(const fr_t& m, size_t lo, size_t hi) const {
        fr_t h = fr_t::zero();
        for (size_t i = hi; i-- > lo;) h = fr_t::load(&in[i]) + m * h;
        return h;
    }
    SV_HD fr_t down(const fr_t& m, fr_t h, size_t lo, size_t hi) const {
        for (size_t i = hi; i-- > lo;) {
            h = fr_t::load(&in[i]) + m * h;
            if (i >= (size_t)shift) h.store(&out[i - shift]);
        }
        return h;
    }
};

// cv[t] = the value of chunk t at m (one level of the recursion; cv of batch member y starts cv_stride elements behind that of y - 1)
template <class S>
static __global__ void __launch_bounds__(256) fr_horner_up_kernel(S walk, size_t n, const fr_mem_t* __restrict__ m_mem, fr_mem_t* __restrict__ cv, size_t T,
                                                                  size_t cv_stride) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= T) return;
    const fr_t m = fr_t::load(m_mem).from_mem_mont();
    const fr_horner_span_t sp = fr_horner_span(t, POLY_CHUNK, n);
    walk.at(blockIdx.y).up(m, sp.lo, sp.hi).store(&cv[(size_t)blockIdx.y * cv_stride + t]);
}
// h behind chunk t of T: carry[t + 1] = h at the first index of chunk t + 1 (the level above, after its own down sweep)
SV_HD fr_t fr_horner_chunk_carry(const fr_mem_t* carry, size_t t, size_t T) { return t + 1 < T ? fr_t::load(&carry[t + 1]) : fr_t::zero(); }
// first[y] = h_0 unless null
template <class S>
static __global__ void __launch_bounds__(256) fr_horner_down_kernel(S walk, size_t n, const fr_mem_t* __restrict__ m_mem, const fr_mem_t* __restrict__ carry, size_t T,
                                                                    size_t carry_stride, fr_mem_t* __restrict__ first) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= T) return;
    const fr_t m = fr_t::load(m_mem).from_mem_mont();
    const fr_horner_span_t sp = fr_horner_span(t, POLY_CHUNK, n);
    const fr_t h = walk.at(blockIdx.y).down(m, fr_horner_chunk_carry(carry + (size_t)blockIdx.y * carry_stride, t, T), sp.lo, sp.hi);
    if (t == 0 && first) h.store(&first[blockIdx.y]);
}

// ---- the same sums with a scan inside every workgroup (round 5) --------------------------------------------------------
// The chunk recursion above is four dependent levels of 32 serial products each for the 2^17 coefficients of an opening, run by
// 4 096 threads: eight launches of 50 - 100 us, 1.3 ms of the 9.5 ms of kernels of one proof (profiles/r05_proof1_timeline.md).
// Here a workgroup of 256 threads owns 256 C consecutive coefficients (C = 8 up to 2^19 coefficients): every thread folds its C
// coefficients (C serial products), the 256 thread values are turned into their suffix sums by a Kogge-Stone scan through LDS
// (8 steps of one product, multipliers m^(C 2^j)), and a workgroup gets the carry of everything behind it as ONE product per
// thread against a table of m^(256 C j) plus a tree of additions.  Three launches (tables, up, down), 17 dependent products.
// Exact field arithmetic in another order: the same values bit for bit.
static constexpr int HORNER2_B = 256;
// tab: [0, 8) step[j] = m^(C 2^j) | [8, 8 + 257) pw[j] = m^(C j) | [265, 265 + 256) pwB[j] = m^(256 C j); internal form
enum { HORNER2_STEP = 0, HORNER2_PW = 8, HORNER2_PWB = 8 + 257, HORNER2_TAB = 8 + 257 + 256 };
// what thread t of the one workgroup writes (m: the true internal form)
SV_HD void fr_horner2_tables_thread(const fr_t& m, fr_mem_t* tab, uint32_t C, uint32_t t) {
    const fr_t mC = m.pow_u64(C);
    const fr_t mB = mC.pow_u64(HORNER2_B);
    mC.pow_u64(t).store(&tab[HORNER2_PW + t]);
    mB.pow_u64(t).store(&tab[HORNER2_PWB + t]);
    if (t == 0) mB.store(&tab[HORNER2_PW + HORNER2_B]);
    if (t < 8) mC.pow_u64(1u << t).store(&tab[HORNER2_STEP + t]);
}
static __global__ void __launch_bounds__(HORNER2_B) fr_horner2_tables_kernel(fr_mem_t m_mem, fr_mem_t* __restrict__ tab, uint32_t C) {
    fr_horner2_tables_thread(fr_t::load(&m_mem).from_mem_mont(), tab, C, threadIdx.x);
}
// The arithmetic of the workgroup scan and of a workgroup's incoming carry, thread by thread; `behind(s)` reads what thread s of the workgroup
// put into the exchange before the barrier (LDS in the kernels, a copy of the threads' values in the host replay).
// Kogge-Stone step j < 8 of thread t
template <class Get>
SV_HD fr_t fr_horner_scan_step(const fr_mem_t* tab, int j, uint32_t t, const fr_t& h, Get behind) {
    return t + (1u << j) < HORNER2_B ? h + fr_t::load(&tab[HORNER2_STEP + j]) * behind(t + (1u << j)) : h;
}
// carry of workgroup b = h at the first coefficient of workgroup b + 1 = sum_(s > b) bv[s] m^(256 C (s - b - 1)): thread t's term of it, and
// one step of the tree that adds the terms up into thread 0 (off = 128, 64 .. 1)
SV_HD fr_t fr_horner_carry_term(const fr_mem_t* tab, const fr_mem_t* bv, uint32_t b, uint32_t t, uint32_t nblocks) {
    return b + 1 + t < nblocks ? fr_t::load(&tab[HORNER2_PWB + t]) * fr_t::load(&bv[b + 1 + t]) : fr_t::zero();
}
template <class Get>
SV_HD fr_t fr_horner_carry_step(uint32_t off, uint32_t t, const fr_t& term, Get behind) {
    return t < off ? term + behind(t + off) : term;
}
// h behind the span of thread t of workgroup b: the workgroup's own suffix sum from thread t + 1 on, plus the carry moved across the threads
// in between
SV_HD fr_t fr_horner_thread_carry(const fr_mem_t* tab, const fr_mem_t* hs, uint32_t b, uint32_t t, const fr_t& carry) {
    const fr_t h = fr_t::load(&tab[HORNER2_PW + HORNER2_B - 1 - t]) * carry;
    return t + 1 < HORNER2_B ? h + fr_t::load(&hs[(size_t)b * HORNER2_B + t + 1]) : h;
}
__device__ __forceinline__ void horner2_lds_put(uint32_t* sh, uint32_t t, const fr_t& x) {
#pragma unroll
    for (int l = 0; l < 9; l++) sh[l * HORNER2_B + t] = x.v[l];
}
__device__ __forceinline__ fr_t horner2_lds_get(const uint32_t* sh, uint32_t t) {
    fr_t x;
#pragma unroll
    for (int l = 0; l < 9; l++) x.v[l] = sh[l * HORNER2_B + t];
    return x;
}
// hs[block * 256 + t] = the suffix sum of the block's thread values from thread t on (= h at the first coefficient of thread t, the
// block taken alone); bv[block] = hs[block * 256] (the block's polynomial at m); those of batch member y start hs_stride and bv_stride
// elements behind those of y - 1
template <class S>
static __global__ void __launch_bounds__(HORNER2_B) fr_horner2_up_kernel(S walk, size_t n, fr_mem_t m_mem, const fr_mem_t* __restrict__ tab, fr_mem_t* __restrict__ hs,
                                                                         fr_mem_t* __restrict__ bv, uint32_t C, size_t hs_stride, size_t bv_stride) {
    __shared__ uint32_t sh[9 * HORNER2_B];
    const uint32_t t = threadIdx.x;
    const auto behind = [&](uint32_t s) { return horner2_lds_get(sh, s); };
    hs += (size_t)blockIdx.y * hs_stride;
    bv += (size_t)blockIdx.y * bv_stride;
    const fr_t m = fr_t::load(&m_mem).from_mem_mont();
    const fr_horner_span_t sp = fr_horner_span((size_t)blockIdx.x * HORNER2_B + t, C, n);
    fr_t h = walk.at(blockIdx.y).up(m, sp.lo, sp.hi);
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
        horner2_lds_put(sh, t, h);
        __syncthreads();
        h = fr_horner_scan_step(tab, j, t, h, behind);
        __syncthreads();
    }
    h.store(&hs[(size_t)blockIdx.x * HORNER2_B + t]);
    if (t == 0) h.store(&bv[blockIdx.x]);
}
// first[y] = h_0 unless null.  nblocks <= 256 + 1.
template <class S>
static __global__ void __launch_bounds__(HORNER2_B) fr_horner2_down_kernel(S walk, size_t n, fr_mem_t m_mem, const fr_mem_t* __restrict__ tab,
                                                                           const fr_mem_t* __restrict__ hs, const fr_mem_t* __restrict__ bv, uint32_t C, size_t hs_stride,
                                                                           size_t bv_stride, fr_mem_t* __restrict__ first) {
    __shared__ uint32_t sh[9 * HORNER2_B];
    const uint32_t t = threadIdx.x, b = blockIdx.x, nblocks = gridDim.x;
    const auto behind = [&](uint32_t s) { return horner2_lds_get(sh, s); };
    hs += (size_t)blockIdx.y * hs_stride;
    bv += (size_t)blockIdx.y * bv_stride;
    const fr_t m = fr_t::load(&m_mem).from_mem_mont();
    fr_t term = fr_horner_carry_term(tab, bv, b, t, nblocks);
#pragma unroll 1
    for (uint32_t off = HORNER2_B / 2; off >= 1; off >>= 1) {
        horner2_lds_put(sh, t, term);
        __syncthreads();
        term = fr_horner_carry_step(off, t, term, behind);
        __syncthreads();
    }
    horner2_lds_put(sh, t, term);
    __syncthreads();
    const fr_t carry = behind(0);
    const fr_horner_span_t sp = fr_horner_span((size_t)b * HORNER2_B + t, C, n);
    if (sp.empty()) return;
    const fr_t h = walk.at(blockIdx.y).down(m, fr_horner_thread_carry(tab, hs, b, t, carry), sp.lo, sp.hi);
    if (sp.lo == 0 && first) h.store(&first[blockIdx.y]);
}

// ---- batch inversion -----------------------------------------------------------------------------------------------
// Montgomery's trick per thread over the strided set {t, t + T, t + 2T, ...} (any partition gives the same values; a
// strided one keeps every access coalesced).  Prefix products are parked in `scratch` (n elements, internal form); one
// Fermat inversion per thread is amortised over ceil(n / T) elements.
static __global__ void fr_batch_inverse_kernel(fr_mem_t* __restrict__ v, size_t n, fr_mem_t coeff_mem, fr_mem_t* __restrict__ scratch, size_t T) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= T) return;
    fr_t tmp = fr_t::one();
    bool any = false;
    for (size_t i = t; i < n; i += T) {
        const fr_t x = fr_t::load(&v[i]);
        if (!x.is_zero()) {
            tmp = tmp * x.from_mem_mont();
            any = true;
        }
        tmp.store(&scratch[i]);
    }
    if (!any) return;
    tmp = tmp.inverse() * fr_t::load(&coeff_mem).from_mem_mont();
    const size_t cnt = (n - t + T - 1) / T;
    for (size_t k = cnt; k-- > 0;) {
        const size_t i = t + k * T;
        const fr_t xs = fr_t::load(&v[i]);
        if (xs.is_zero()) continue;
        const fr_t s = k ? fr_t::load(&scratch[i - T]) : fr_t::one();
        (tmp * s).to_mem_mont().store(&v[i]);
        tmp = tmp * xs.from_mem_mont();
    }
}

// v_i <- v_i * c * g^i; thread t owns i = t, t + T, ... with running power c g^t (g^T)^k
static __global__ void fr_distribute_powers_kernel(fr_mem_t* __restrict__ v, size_t n, fr_mem_t g_mem, fr_mem_t c_mem, size_t T) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= T || t >= n) return;
    const fr_t g = fr_t::load(&g_mem).from_mem_mont();
    fr_t pw = fr_t::load(&c_mem).from_mem_mont() * g.pow_u64(t);
    const fr_t step = g.pow_u64(T);
    for (size_t i = t; i < n; i += T) {
        (fr_t::load(&v[i]) * pw).store(&v[i]);
        pw = pw * step;
    }
}
static __global__ void fr_fill_kernel(fr_mem_t* v, size_t n, fr_mem_t x) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) v[i] = x;
}
// v_i <- (v_i == x) ? one : zero   (the tau-in-domain branch of evaluate_all_lagrange_coefficients, domain.rs:265-275)
static __global__ void fr_onehot_kernel(fr_mem_t* v, size_t n, fr_mem_t x_mem, fr_mem_t one_mem) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    const fr_t x = fr_t::load(&x_mem);
    fr_mem_t zero_mem;
    fr_t::zero().store(&zero_mem);
    for (; i < n; i += st) v[i] = (fr_t::load(&v[i]) == x) ? one_mem : zero_mem;
}

// ---- linear combination of polynomials ------------------------------------------------------------------------------
// out[i] = sum_k c_k p_k[i] for i < n_out, p_k[i] = 0 from len_k on: every linear combination SonicKZG10::open_combinations materialises
// (`poly += (coeff, cur_poly)` per term, sonic_pc/mod.rs:413-473) and the fold of batch_open (combine_polynomials, mod.rs:548-564), in ONE pass
// over K + 1 vectors where a chain of AXPY passes moves 3K - 1.  The operand table travels BY KERNEL ARGUMENT: nothing is staged or retained (an
// enqueue-only call inside a scope has no later moment to release a table), and pointers, lengths and coefficients are wave-uniform - scalar
// loads from the kernel-argument segment.  Coefficients arrive in the TRUE internal form (the host ran from_mem_mont, ff.hip.h compiles for it),
// vector elements are read raw ("shifted", see above): every product c_k * p_k[i], and so the sum, is a shifted value and is stored raw.
// Terms are taken FR_LINCOMB_G at a time through Fp::sum_of_products: one Montgomery reduction per group instead of one per term (72 of the
// 153 multiply-adds of a product).  What has been timed of that choice, and what is still an estimate, is stated in DESIGN.md section 4
// (tools/bench_fr_lincomb.py is the tool).
// The host sorts the operands by length, longest first (fr_lincomb_plan): the live operands at index i are a prefix of the table, a group whose
// first operand has ended is skipped with everything behind it, and a shorter operand inside a live group reads as zero.
static constexpr int FR_LINCOMB_G = 6;
static_assert(FR_LINCOMB_G == 6, "fr_lincomb_at dispatches the short last group over 1 .. 5");
static constexpr int FR_LINCOMB_CHUNK = 24;  // operands per launch: four groups; 24 x (8 + 8 + 36) B + 4 = 1252 B of the 4 KB of kernel arguments
struct fr_lincomb_t {
    const fr_mem_t* p[FR_LINCOMB_CHUNK];
    size_t len[FR_LINCOMB_CHUNK];      // non-increasing over k < count
    uint32_t c[FR_LINCOMB_CHUNK][9];   // limbs of c_k, true internal form
    int count;
};
template <int G>
SV_HD fr_t fr_lincomb_group(const fr_lincomb_t& t, int k0, size_t i) {
    fr_t c[G], x[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        c[g] = fr_t::from_table(t.c[k0 + g]);
        x[g] = i < t.len[k0 + g] ? fr_t::load(&t.p[k0 + g][i]) : fr_t::zero();
    }
    return fr_t::sum_of_products<G>(c, x);
}
// the per-element routine: the kernel below and the host replay (snarkvm_hip_selftest_fr_lincomb) both call it
SV_HD fr_t fr_lincomb_at(const fr_lincomb_t& t, size_t i) {
    fr_t acc = fr_t::zero();
#pragma unroll 1
    for (int k0 = 0; k0 < t.count && i < t.len[k0]; k0 += FR_LINCOMB_G) {
        fr_t s;
        switch (t.count - k0) {  // only the last group of a launch is short
            case 1: s = fr_lincomb_group<1>(t, k0, i); break;
            case 2: s = fr_lincomb_group<2>(t, k0, i); break;
            case 3: s = fr_lincomb_group<3>(t, k0, i); break;
            case 4: s = fr_lincomb_group<4>(t, k0, i); break;
            case 5: s = fr_lincomb_group<5>(t, k0, i); break;
            default: s = fr_lincomb_group<FR_LINCOMB_G>(t, k0, i); break;
        }
        acc = acc + s;
    }
    return acc;
}
// out may be the start of one operand: a thread reads every operand at i before it writes out[i], and no other thread touches index i
static __global__ void __launch_bounds__(256) fr_lincomb_kernel(fr_mem_t* out, size_t n_out, fr_lincomb_t t) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n_out; i += st) fr_lincomb_at(t, i).store(&out[i]);
}

// ---- opening fold: the combination and its quotient by X - m in one sweep up and one sweep down --------------------------------------
// comb[i] = sum_k c_k p_k[i] is formed ONCE, in the up sweep of the suffix Horner sums above: a thread evaluates fr_lincomb_at over its
// chunk, parks every comb[i] in q[i] and folds it into its chunk value.  The down sweep then runs IN PLACE on q with the ownership shifted
// by one: walking downwards from its incoming h_hi, a thread reads comb[i] from q[i], writes q[i] = h_(i+1) - its running value BEFORE the
// step - and forms h_i.  A thread writes only indices of its own chunk [lo, hi), each after its one read of it, and nobody else touches
// them: no hazard across threads, no staging; q[n - 1] = h_n = 0 falls out for the thread that owns the end, and the thread that owns
// index 0 is left with h_0 = comb(m), the remainder.  q == nullptr: the up sweep alone, nothing is stored (the value only).
// q may be the START of one table entry (a list longer than FR_LINCOMB_CHUNK takes the sum so far back in as a term): index i of every
// entry is read before q[i] is written.
// A thread of the up sweep walks its own C (or POLY_CHUNK) consecutive coefficients, so its reads of a member are 32-byte pieces 32 C bytes
// away from its neighbour's, and a proof-sized polynomial gives the sweep a quarter of the chip's lanes at most: forming a long combination
// there loses to fr_lincomb_kernel's coalesced full grid.  Measured (profiles/fr_open_fold.md) with the sweep taking up to 24, 12, 6 and 1
// terms - of a longer list the launcher sends the other members through accumulating fr_lincomb_kernel launches into q first and the sweep
// takes that sum in as its first term: with 24 (everything in the sweep) 10 and 19 members ran at 0.80 - 0.93 of the speed of the chain of
// calls this pass replaces, with 12 at 0.91 - 0.99, with 6 at 1.01 - 1.24, with 1 at 1.18 - 1.44 (1.26 - 1.54 since the sweep reads the
// parked sum as it is, below); every shape was fastest with 1.  So
// FR_OPEN_FUSE = 1: a single member is combined inside the sweep (three launches); of two or more ALL go through fr_lincomb_kernel, and the
// sweep finds the combination parked in q (one launch more, K + 4 vector passes, still formed once and divided in place, no vector beside
// q).  Without a quotient there is no q to park in: the sweep takes a whole table (fr_open_plan).
static constexpr int FR_OPEN_FUSE = 1;
static_assert(FR_OPEN_FUSE >= 1 && FR_OPEN_FUSE <= FR_LINCOMB_CHUNK, "the fused sweep takes one table");
// The span policy of the fold: the sweeps themselves are the scaffolds of the suffix Horner sums above, in either route; the fold has no batch.
struct fr_span_fold_t {
    fr_mem_t* q;
    fr_lincomb_t t;
    SV_HD const fr_span_fold_t& at(size_t) const { return *this; }
    SV_HD fr_t up(const fr_t& m, size_t lo, size_t hi) const {
        // the table holds the parked sum alone (every member has gone through fr_lincomb_kernel): comb[i] is in q[i] already
        const bool parked = q && t.count == 1 && t.p[0] == q;
        fr_t h = fr_t::zero();
        for (size_t i = hi; i-- > lo;) {
            const fr_t x = parked ? fr_t::load(&q[i]) : fr_lincomb_at(t, i);
            if (q && !parked) x.store(&q[i]);
            h = x + m * h;
        }
        return h;
    }
    // q[i] = h_(i+1) for lo <= i < hi on return
    SV_HD fr_t down(const fr_t& m, fr_t h, size_t lo, size_t hi) const {
        for (size_t i = hi; i-- > lo;) {
            const fr_t x = fr_t::load(&q[i]);
            h.store(&q[i]);
            h = x + m * h;
        }
        return h;
    }
};
// first[0] = vals[0] + vals[1] + ... in list order (the values of the launches of a member list longer than one table, evaluation only)
static __global__ void fr_open_sum_kernel(const fr_mem_t* __restrict__ vals, uint32_t count, fr_mem_t* __restrict__ first) {
    if (blockIdx.x | threadIdx.x) return;
    fr_t s = fr_t::zero();
    for (uint32_t k = 0; k < count; k++) s = s + fr_t::load(&vals[k]);
    s.store(first);
}

// ---- X^D - 1 -------------------------------------------------------------------------------------------------------
// Long division of a (len coefficients) by X^D - 1 folds the coefficient classes mod D:
//   quotient_i = sum_{k >= 1} a_(i + kD)   (i < len - D),   remainder_i = sum_{k >= 0} a_(i + kD)   (i < min(D, len)).
static __global__ void fr_fold_vanishing_kernel(const fr_mem_t* __restrict__ a, size_t len, size_t D, fr_mem_t* __restrict__ quot,
                                         fr_mem_t* __restrict__ rem, size_t stride) {
    {
        const size_t off = (size_t)blockIdx.y * stride;
        a += off, rem += off;
        if (quot) quot += off;
    }
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t qlen = len > D ? len - D : 0;
    const size_t rlen = len < D ? len : D;
    if (i >= qlen && i >= rlen) return;
    fr_t acc = fr_t::zero();
    // walk the class from the top so that the running sum at index i + D is the quotient and at i the remainder
    size_t top = i + ((len - 1 - i) / D) * D;
    for (size_t j = top; j > i; j -= D) acc = acc + fr_t::load(&a[j]);
    if (i < qlen) acc.store(&quot[i]);
    if (i < rlen) (acc + fr_t::load(&a[i])).store(&rem[i]);
}
// out (len + D elements) = a * (X^D - 1)
static __global__ void fr_mul_vanishing_kernel(const fr_mem_t* __restrict__ a, size_t len, size_t D, fr_mem_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= len + D) return;
    const fr_t hi = (i >= D) ? fr_t::load(&a[i - D]) : fr_t::zero();
    const fr_t lo = (i < len) ? fr_t::load(&a[i]) : fr_t::zero();
    (hi - lo).store(&out[i]);
}

// ---- selector fold: Varuna round 3 -----------------------------------------------------------------------------------
// apply_randomized_selector (ahp/selectors.rs:100-121) per (instance, matrix) member k of the lineval sumcheck (third.rs:280-327): scale the
// product p_k by mu_k = combiner * n_k / N, divide by X^n_k - 1 (quotient -> h_1, remainder = x g), multiply x g by X^N - 1 and divide by
// X^n_k - 1 again.  The last two steps are a TILING - the quotient of xg (X^N - 1) by X^n - 1 is q[i] = xg[i mod n] for i < N and the
// remainder is identically zero when n | N - and the scaling commutes with the class sums, so the whole sequence, summed over the members, is
//   h[i]  = sum_k mu_k sum_{j >= 1, i + j n_k < L_k} p_k[i + j n_k]        i < h_len
//   xg[i] = sum_k mu_k sum_{j >= 0} p_k[(i mod n_k) + j n_k]               i < N
//   sums[k] = n_k sum_j p_k[j n_k]    (= sum of p_k over the n_k-th roots of unity, third.rs:317: no transform needed)
// ONE streaming pass where the reference's sequence is seven launches per member.  One thread per output index walks each member's residue
// class from the top, as fr_fold_vanishing_kernel does: the running sum when the walk passes i is the h term, at the bottom the class sum;
// the thread that owns index 0 has walked class 0 of every member and writes sums.  The member table travels BY KERNEL ARGUMENT like
// fr_lincomb_t (nothing staged, nothing retained: an enqueue-only call has no later moment to release a table); multipliers and the n_k
// arrive in the TRUE internal form, the vectors are streamed raw, so every product is a raw memory-form value.  Members go FR_SELECTOR_G at
// a time through Fp::sum_of_products (class sums are canonical, the multipliers are the first factor).  A list longer than
// FR_SELECTOR_CHUNK takes further launches with `accumulate` set: those add to what the outputs hold.
// Class sums and N > n: xg has the period P = lcm_k n_k, which divides N.  With FR_SELECTOR_TILE the fold runs over i < P only and
// fr_tile_kernel copies xg[i mod P] to the rest - every class sum is formed once; without, every i < N recomputes its class sum (reads that
// hit L2, redundant by N / n_k).  Both, and the group sizes, give the same bytes: field addition is exact and results canonical, there are
// no atomics, and a thread's order of additions depends on neither the grid nor the split.  tools/bench_fr_selector.py times the variants
// (-DFR_SELECTOR_G=1|2|3|6, -DFR_SELECTOR_TILE=0|1); what has been measured is in profiles/fr_selector.md.
// Indices are 32-bit: lengths <= 2^29, N <= 2^28, and an n_k above 2^30 behaves like 2^30 for every index that exists (the host clamps it;
// ns keeps the true value).  Registers (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): fr_selector_fold_kernel 159 VGPRs, 106 SGPRs, no
// scratch, 3 waves per SIMD at G = 6 (G = 3: 104 VGPRs, 100 SGPRs, no scratch, 4 waves; G = 1: 68 VGPRs); fr_tile_kernel 20 VGPRs, 25 SGPRs, no
// scratch.  No call (tools/device_calls.sh).
#ifndef FR_SELECTOR_G
#define FR_SELECTOR_G 6  // members per Montgomery reduction: measured against 1 and 3 (profiles/fr_selector.md)
#endif
#ifndef FR_SELECTOR_TILE
#define FR_SELECTOR_TILE 1  // 1: class sums once, then tiled; 0: every index recomputes its class sum (about 3x slower at N = 4 n with 24 members of 2^21)
#endif
static_assert(FR_SELECTOR_G >= 1 && FR_SELECTOR_G <= 6, "Fp::sum_of_products takes at most 6 terms");
static constexpr int FR_SELECTOR_CHUNK = 24;  // members per launch: 24 x (8 + 8 + 4 + 4 + 36 + 36) B + 8 = 2312 B of the 4 KB of kernel arguments
struct fr_selector_t {
    const fr_mem_t* p[FR_SELECTOR_CHUNK];
    fr_mem_t* sum[FR_SELECTOR_CHUNK];     // where sums[k] goes; nullptr: not wanted
    uint32_t len[FR_SELECTOR_CHUNK];      // L_k
    uint32_t n[FR_SELECTOR_CHUNK];        // min(n_k, 2^30)
    uint32_t mu[FR_SELECTOR_CHUNK][9];    // limbs of mu_k, true internal form
    uint32_t ns[FR_SELECTOR_CHUNK][9];    // limbs of n_k as a field element, true internal form
    int count;
    int accumulate;  // the outputs already hold the sum over earlier members
};
SV_HD uint32_t fr_selector_mod(uint32_t x, uint32_t n) { return (n & (n - 1)) ? x % n : x & (n - 1); }
// member (p, L, n) at index i: hs = sum_{j >= 1, i + j n < L} p[i + j n]; with want_class also cs = sum_{j >= 0} p[(i mod n) + j n]
SV_HD void fr_selector_walk(const fr_mem_t* p, uint32_t L, uint32_t n, uint32_t i, bool want_class, fr_t& hs, fr_t& cs) {
    hs = fr_t::zero(), cs = fr_t::zero();
    const uint32_t lo = want_class ? fr_selector_mod(i, n) : i;
    if (lo >= L) return;
    fr_t acc = fr_t::zero();
    uint32_t j = (L - 1) - fr_selector_mod(L - 1 - lo, n);  // the top of the class: j = lo mod n, so j > x >= lo implies j - n >= x
    for (; j > i; j -= n) acc = acc + fr_t::load(&p[j]);
    hs = acc;
    if (!want_class) return;
    for (; j > lo; j -= n) acc = acc + fr_t::load(&p[j]);
    cs = acc + fr_t::load(&p[lo]);
}
// members k0 + g .. k0 + G - 1 of a group, by recursion: a loop that holds the walks is not always unrolled, and an array indexed by a
// loop counter that survives lives in scratch
template <int G, int g>
SV_HD void fr_selector_members(const fr_selector_t& t, int k0, uint32_t i, bool want_xg, fr_t* mu, fr_t* hs, fr_t* cs) {
    if constexpr (g < G) {
        const int k = k0 + g;
        mu[g] = fr_t::from_table(t.mu[k]);
        const bool want_sum = i == 0 && t.sum[k];
        fr_selector_walk(t.p[k], t.len[k], t.n[k], i, want_xg || want_sum, hs[g], cs[g]);
        if (want_sum) (fr_t::from_table(t.ns[k]) * cs[g]).store(t.sum[k]);
        fr_selector_members<G, g + 1>(t, k0, i, want_xg, mu, hs, cs);
    }
}
template <int G>
SV_HD void fr_selector_group(const fr_selector_t& t, int k0, uint32_t i, bool want_h, bool want_xg, fr_t& h, fr_t& xg) {
    fr_t mu[G], hs[G], cs[G];
    fr_selector_members<G, 0>(t, k0, i, want_xg, mu, hs, cs);
    if (want_h) h = h + fr_t::sum_of_products<G>(mu, hs);
    if (want_xg) xg = xg + fr_t::sum_of_products<G>(mu, cs);
}
// the per-index routine: the kernel below and the host replay (snarkvm_hip_selftest_fr_selector_fold) both call it.  h_out / xg_out may be
// nullptr (skipped); xg is written for i < span.
SV_HD void fr_selector_at(const fr_selector_t& t, fr_mem_t* h_out, uint32_t h_len, fr_mem_t* xg_out, uint32_t span, uint32_t i) {
    const bool want_h = h_out && i < h_len, want_xg = xg_out && i < span;
    fr_t h = fr_t::zero(), xg = fr_t::zero();
    if (t.accumulate) {
        if (want_h) h = fr_t::load(&h_out[i]);
        if (want_xg) xg = fr_t::load(&xg_out[i]);
    }
    // Whole groups, then what is left in groups of 3, 2 or 1: four instantiations at most.  Every use of the table in an instantiation counts
    // towards the limit up to which the compiler reads a by-value kernel argument in place (more, and it copies the table to scratch).
    constexpr int S = FR_SELECTOR_G > 3 ? 3 : FR_SELECTOR_G;
    int step;
#pragma unroll 1
    for (int k0 = 0; k0 < t.count; k0 += step) {
        const int left = t.count - k0;
        if (left >= FR_SELECTOR_G)
            fr_selector_group<FR_SELECTOR_G>(t, k0, i, want_h, want_xg, h, xg), step = FR_SELECTOR_G;
        else if (left >= 3)
            fr_selector_group<S>(t, k0, i, want_h, want_xg, h, xg), step = S;
        else if (left == 2)
            fr_selector_group<(S >= 2 ? 2 : 1)>(t, k0, i, want_h, want_xg, h, xg), step = S >= 2 ? 2 : 1;
        else
            fr_selector_group<1>(t, k0, i, want_h, want_xg, h, xg), step = 1;
    }
    if (want_h) h.store(&h_out[i]);
    if (want_xg) xg.store(&xg_out[i]);
}
// threads = max(h_len if h_out, span if xg_out, 1): index 0 always has an owner (the sums)
static __global__ void __launch_bounds__(256) fr_selector_fold_kernel(fr_mem_t* h_out, uint32_t h_len, fr_mem_t* xg_out, uint32_t span, uint32_t threads, fr_selector_t t) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < threads; i += st) fr_selector_at(t, h_out, h_len, xg_out, span, (uint32_t)i);
}
// v[i] = v[i mod period] for period <= i < n: reads [0, period), writes the rest
SV_HD void fr_tile_at(fr_mem_t* v, uint32_t period, uint32_t i) { v[i] = v[fr_selector_mod(i, period)]; }
static __global__ void fr_tile_kernel(fr_mem_t* v, uint32_t period, uint32_t n) {
    size_t i = period + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) fr_tile_at(v, period, (uint32_t)i);
}

// ---- rounds 1 and 2: the witness gather and the rowcheck fold ---------------------------------------------------------------------
// Round 1 (calculate_w, first.rs:127-161): between the forward and the inverse transform at |V| the reference interleaves the private
// variables with the input subgroup - position k of the variable domain is an input position when ratio = |V| / |X| divides k (there w is
// zero), otherwise it holds private variable k - k / ratio - 1 (zero past the end of the witness) minus x_poly's evaluation at k.  A map:
// one thread per element, which reads x[k] before it writes out[k], so out may BE x.
SV_HD void fr_witness_at(fr_mem_t* out, const fr_mem_t* w, uint32_t w_len, const fr_mem_t* x, uint32_t ratio, uint32_t k) {
    const uint32_t q = k / ratio;
    if (k == q * ratio) {
        fr_t::zero().store(&out[k]);
        return;
    }
    const uint32_t j = k - q - 1;
    const fr_t wv = j < w_len ? fr_t::load(&w[j]) : fr_t::zero();
    (wv - fr_t::load(&x[k])).store(&out[k]);
}
static __global__ void __launch_bounds__(256) fr_witness_evals_kernel(fr_mem_t* out, uint32_t n, const fr_mem_t* w, uint32_t w_len, const fr_mem_t* x, uint32_t ratio) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) fr_witness_at(out, w, w_len, x, ratio, (uint32_t)i);
}
// Round 1 in lock step: the evaluations of z ITSELF on the variable domain.  Adding x_poly's evaluations back to the vector above leaves the
// padded public input on the input subgroup and the private variables elsewhere - the interleaving of reindex_by_subdomain
// (fft/domain.rs:322-344) over the row v = public (input_size values) ++ private (num_vars - input_size values), the x operand of the
// circuit's sparse products - and since z = w (X^|X| - 1) + x_poly with deg x_poly < |X|, ONE inverse transform of it yields z, whose quotient
// by X^|X| - 1 is w and whose remainder is x_poly.  No arithmetic: position k takes v[k / ratio] when ratio divides k, otherwise
// v[input_size + k - k / ratio - 1], zero from num_vars on.  An element travels as its two 16-byte halves, untouched (no limb unpacking); a
// wave's stores cover 2 KB of consecutive bytes and both read streams only move forward with k.  blockIdx.y is the batch member (instance):
// its row starts stride_vars elements after the previous one's, its output stride_out elements.  Indices are 32-bit: n <= 2^28, and the
// launch stays under 2^21 threads per member, so i + st cannot wrap.  Registers (gfx950, -O3, -Rpass-analysis=kernel-resource-usage):
// fr_assignment_evals_kernel 14 VGPRs, 26 SGPRs, 8 waves per SIMD, no scratch, no LDS.
SV_HD void fr_assignment_at(fr_mem_t* out, const fr_mem_t* v, uint32_t num_vars, uint32_t input_size, uint32_t ratio, uint32_t k) {
    const uint32_t q = k / ratio;
    const uint32_t j = k == q * ratio ? q : input_size + (k - q - 1);
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (j < num_vars) {
        const uint4* src = (const uint4*)&v[j];
        lo = src[0], hi = src[1];
    }
    uint4* dst = (uint4*)&out[k];
    dst[0] = lo, dst[1] = hi;
}
static __global__ void __launch_bounds__(256) fr_assignment_evals_kernel(fr_mem_t* __restrict__ out, uint32_t n, const fr_mem_t* __restrict__ vars, uint32_t num_vars,
                                                                         uint32_t input_size, uint32_t ratio, size_t stride_out, size_t stride_vars) {
    out += (size_t)blockIdx.y * stride_out, vars += (size_t)blockIdx.y * stride_vars;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t st = gridDim.x * blockDim.x;
    for (; i < n; i += st) fr_assignment_at(out, vars, num_vars, input_size, ratio, i);
}
// Round 2 (calculate_rowcheck_witness, second.rs:76-142, with apply_randomized_selector without a remainder witness, selectors.rs:88-99):
// h_0 = sum over every instance k of every circuit of mu_k (z_a z_b - z_c) / v_R.  z_a z_b - z_c has degree <= 2 |R| - 2, its quotient by v_R
// degree <= |R| - 2, so the quotient is fixed by its values on ONE coset g R, where v_R is the constant g^|R| - 1: no doubled domain.  Folded
// into mu_k, the constant leaves
//   out[i] = sum_k mu_k (a_k[i] b_k[i] - c_k[i])                                         (FR_ROWCHECK_FOLD; over coset evaluations)
//   violations[k] = #{i < n : a_k[i] b_k[i] != c_k[i]}                                     (FR_ROWCHECK_CHECK; over evaluations on R itself:
//                                                                                            the remainder by v_R is zero iff every count is)
// and, the inverse transform being linear, ONE inverse coset transform of `out` where the reference runs one per instance.
// The member table travels BY KERNEL ARGUMENT like fr_selector_t.  Vectors are streamed raw: raw(a) * raw(b) is the internal form of
// a b 2^-10, so the host passes mu_k * MEM2INT beside -mu_k (both true internal form) and the member's term is the sum of TWO wide products,
// (mu_k MEM2INT) (a b) + (-mu_k) c, a raw memory-form value: FR_ROWCHECK_G members = 2 G wide products go through one
// Fp::sum_of_products (its conditions hold: the multipliers are canonical, a b is a canonical product and c a memory image).  The check
// compares (a b).from_mem_mont() with c limb for limb: both canonical.  A list longer than FR_ROWCHECK_CHUNK takes further launches with
// `accumulate` set, which add to `out`.  Counts: a wave's violating lanes of member m are counted by one ballot and added to the member's
// 64-bit counter by one integer atomic of the lowest such lane - integer sums, so the counts do not depend on the order; a wave without a
// violation (every wave of a valid proof) issues none.  The Fr output has no atomics and a fixed order of additions.
// Indices are 32-bit: n <= 2^28.  Registers (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): fr_rowcheck_fold_kernel<FOLD> 131 VGPRs, 102 SGPRs,
// 3 waves per SIMD at G = 3; <CHECK> 52 VGPRs, 8 waves; <FOLD | CHECK> 144 VGPRs and 10 SGPRs spilled to VGPR lanes; fr_witness_evals_kernel 28 VGPRs;
// no scratch in any of them.  tools/bench_fr_rowcheck.py times G = 3 against G = 1 (-DFR_ROWCHECK_G=1); what has been measured is in
// profiles/fr_rowcheck.md.
enum { FR_ROWCHECK_FOLD = 1, FR_ROWCHECK_CHECK = 2 };
#ifndef FR_ROWCHECK_G
#define FR_ROWCHECK_G 3  // members per Montgomery reduction (two wide products each): measured against 1 (profiles/fr_rowcheck.md)
#endif
static_assert(FR_ROWCHECK_G >= 1 && FR_ROWCHECK_G <= 3, "Fp::sum_of_products takes at most 6 terms: two per member");
static constexpr int FR_ROWCHECK_CHUNK = 24;  // members per launch: 24 x (3 x 8 + 36 + 36) B + 8 = 2312 B of the 4 KB of kernel arguments
static_assert(FR_ROWCHECK_CHUNK <= 32, "fr_rowcheck_at returns one bit per member of a launch");
struct fr_rowcheck_t {
    const fr_mem_t* a[FR_ROWCHECK_CHUNK];
    const fr_mem_t* b[FR_ROWCHECK_CHUNK];
    const fr_mem_t* c[FR_ROWCHECK_CHUNK];
    uint32_t mu[FR_ROWCHECK_CHUNK][9];   // limbs of mu_k * MEM2INT, true internal form
    uint32_t nmu[FR_ROWCHECK_CHUNK][9];  // limbs of -mu_k, true internal form
    int count;
    int accumulate;  // out already holds the sum over earlier members
};
// members k0 + g .. k0 + G - 1 of a group, by recursion (see fr_selector_members)
template <int MODE, int G, int g>
SV_HD void fr_rowcheck_members(const fr_rowcheck_t& t, int k0, uint32_t i, fr_t* f, fr_t* x, uint32_t& bad) {
    if constexpr (g < G) {
        const int k = k0 + g;
        const fr_t ab = fr_t::load(&t.a[k][i]) * fr_t::load(&t.b[k][i]);
        const fr_t c = fr_t::load(&t.c[k][i]);
        if (MODE & FR_ROWCHECK_CHECK) bad |= (ab.from_mem_mont() != c ? 1u : 0u) << k;
        if (MODE & FR_ROWCHECK_FOLD) {
            f[2 * g] = fr_t::from_table(t.mu[k]), x[2 * g] = ab;
            f[2 * g + 1] = fr_t::from_table(t.nmu[k]), x[2 * g + 1] = c;
        }
        fr_rowcheck_members<MODE, G, g + 1>(t, k0, i, f, x, bad);
    }
}
template <int MODE, int G>
SV_HD void fr_rowcheck_group(const fr_rowcheck_t& t, int k0, uint32_t i, fr_t& acc, uint32_t& bad) {
    fr_t f[2 * G], x[2 * G];
    fr_rowcheck_members<MODE, G, 0>(t, k0, i, f, x, bad);
    if (MODE & FR_ROWCHECK_FOLD) acc = acc + fr_t::sum_of_products<2 * G>(f, x);
}
// the per-index routine: the kernel below and the host replay (snarkvm_hip_selftest_fr_rowcheck_fold) both call it.  -> bit m set: member m
// of this launch is violated at i (MODE without CHECK: 0).  out is written only with FOLD.
template <int MODE>
SV_HD uint32_t fr_rowcheck_at(const fr_rowcheck_t& t, fr_mem_t* out, uint32_t i) {
    fr_t acc = fr_t::zero();
    uint32_t bad = 0;
    if ((MODE & FR_ROWCHECK_FOLD) && t.accumulate) acc = fr_t::load(&out[i]);
    int step;
#pragma unroll 1
    for (int k0 = 0; k0 < t.count; k0 += step) {  // whole groups, then what is left in groups of 2 or 1
        const int left = t.count - k0;
        if (left >= FR_ROWCHECK_G)
            fr_rowcheck_group<MODE, FR_ROWCHECK_G>(t, k0, i, acc, bad), step = FR_ROWCHECK_G;
        else if (left == 2)
            fr_rowcheck_group<MODE, (FR_ROWCHECK_G >= 2 ? 2 : 1)>(t, k0, i, acc, bad), step = FR_ROWCHECK_G >= 2 ? 2 : 1;
        else
            fr_rowcheck_group<MODE, 1>(t, k0, i, acc, bad), step = 1;
    }
    if (MODE & FR_ROWCHECK_FOLD) acc.store(&out[i]);
    return bad;
}
#if defined(__HIPCC__)
// viol: the counters of this launch's members, zeroed by the host before the first launch
template <int MODE>
static __global__ void __launch_bounds__(256) fr_rowcheck_fold_kernel(fr_mem_t* out, unsigned long long* viol, uint32_t n, fr_rowcheck_t t) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) {
        const uint32_t bad = fr_rowcheck_at<MODE>(t, out, (uint32_t)i);
        if ((MODE & FR_ROWCHECK_CHECK) && __ballot(bad != 0)) {
            for (int m = 0; m < t.count; m++) {
                const unsigned long long who = __ballot((bad >> m) & 1);
                if (who && (int)(threadIdx.x & 63) == __ffsll(who) - 1) atomicAdd(&viol[m], (unsigned long long)__popcll(who));
            }
        }
    }
}
#endif

// ---- reductions: a vector -> a value ----------------------------------------------------------------------------------------
// The third family of Fr passes beside the maps and the scans: ONE streaming read with a tree at the end, so that a question about a
// device-resident vector - its inner product with the Lagrange coefficients (Evaluations::evaluate_with_coeffs, fft/evaluations.rs:85-92), its sum
// over a domain (first.rs:119), its degree, whether it is zero, how many leading zeros a commitment may skip (dense.rs:66-96, kzg10/mod.rs:455-467)
// - costs a 32-byte or 24-byte answer instead of a download.
//   launch 1  fr_reduce_kernel / fr_support_kernel: grid (blocks, batch members).  Threads stride over the vector through the grid and accumulate
//             privately; a wave folds its 64 values by a butterfly of __shfl_xor exchanges (every lane ends with the wave's value), the waves of the
//             workgroup meet through LDS (one value per wave, the same butterfly over the first lanes); thread 0 writes ONE partial per workgroup
//             and batch member into lane workspace.
//   launch 2  fr_reduce_final_kernel / fr_support_final_kernel: one workgroup per batch member folds the partials by the same routines.
// Two launches and no "last block done" counter: which workgroup finishes last never enters the result, not even as the shape of the tree.  Field
// addition is exact and Fr elements have one representation, so ANY tree gives the same 32 bytes; min, max and integer sums likewise.  The trees
// here are chosen for speed alone.
// Inner product: both operands are streamed raw ("shifted", see the top of this file); raw(a) * raw(b) is the internal form of a b 2^-10, sums of
// such values are such values, and ONE from_mem_mont at the very end (launch 2, thread 0) turns the total into the memory form of sum a_i b_i.
// Terms go FR_REDUCE_G at a time through Fp::sum_of_products: one Montgomery reduction per group (its operand conditions hold: memory images of
// field elements are canonical, so the first factor is < r and the second < 2^256).  G = 4 and not the 6 the accumulator allows: both factors are
// vector registers here (fr_lincomb keeps its coefficients in scalar registers), 2 x 9 x G limbs in flight: 122 VGPRs.  Measured at 2^24 elements:
// 0.232 ms against 0.301 (G = 1), 0.243 (G = 2) and 0.233 (G = 6); the grid cap makes no measurable difference between 512 and 8192
// (profiles/fr_reduce.md; tools/bench_fr_reduce.py is the tool).
// Geometry: FR_REDUCE_B threads, ceil(n / FR_REDUCE_B) workgroups up to FR_REDUCE_BLOCKS_MAX (2048 x 256 threads = every wave slot of the 256 CUs
// once); the kernels themselves take any power-of-two number of waves up to FR_REDUCE_B / 64 and any number of workgroups (the host replay,
// snarkvm_hip_selftest_fr_reduce / _fr_support, walks a given geometry through the same per-thread and combine routines).
enum { FR_REDUCE_SUM = 0, FR_REDUCE_DOT = 1 };
static constexpr int FR_REDUCE_B = 256;
static constexpr int FR_REDUCE_G = 4;
static constexpr unsigned FR_REDUCE_BLOCKS_MAX = 2048;
SV_HD unsigned fr_reduce_blocks(size_t n) {
    const size_t b = (n + FR_REDUCE_B - 1) / FR_REDUCE_B;
    return (unsigned)(b < 1 ? 1 : (b > FR_REDUCE_BLOCKS_MAX ? FR_REDUCE_BLOCKS_MAX : b));
}
// G terms at i, i + step, ...: their sum (OP = SUM) or the sum of their products, unreduced to memory form (OP = DOT)
template <int OP, int G>
SV_HD fr_t fr_reduce_group(const fr_mem_t* a, const fr_mem_t* b, size_t i, size_t step) {
    fr_t x[G], y[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        x[g] = fr_t::load(&a[i + g * step]);
        if (OP == FR_REDUCE_DOT) y[g] = fr_t::load(&b[i + g * step]);
    }
    if (OP == FR_REDUCE_DOT) return fr_t::sum_of_products<G>(x, y);
    fr_t s = x[0];
#pragma unroll
    for (int g = 1; g < G; g++) s = s + x[g];
    return s;
}
// the private accumulation of one thread over i = first, first + step, ... < n: whole groups, then single terms
template <int OP>
SV_HD fr_t fr_reduce_thread(const fr_mem_t* a, const fr_mem_t* b, size_t n, size_t first, size_t step) {
    fr_t acc = fr_t::zero();
    size_t i = first;
#pragma unroll 1
    for (; i < n && n - i > (FR_REDUCE_G - 1) * step; i += FR_REDUCE_G * step) acc = acc + fr_reduce_group<OP, FR_REDUCE_G>(a, b, i, step);
#pragma unroll 1
    for (; i < n; i += step) acc = acc + fr_reduce_group<OP, 1>(a, b, i, step);
    return acc;
}
// what launch 2 does to the total
SV_HD fr_t fr_reduce_finish(int op, const fr_t& total) { return op == FR_REDUCE_DOT ? total.from_mem_mont() : total; }

// trimmed_len: index of the last non-zero element + 1 (0: the zero vector; degree = max(trimmed_len, 1) - 1); leading_zeros: index of the first
// non-zero element (n: the zero vector); nonzero: how many.  An element is zero iff all of its 8 words are (Montgomery 0 is 0).
struct fr_support_t {
    uint64_t trimmed_len, leading_zeros, nonzero;
};
SV_HD fr_support_t fr_support_identity(size_t n) { return fr_support_t{0, (uint64_t)n, 0}; }
SV_HD fr_support_t fr_support_combine(const fr_support_t& x, const fr_support_t& y) {
    return fr_support_t{x.trimmed_len > y.trimmed_len ? x.trimmed_len : y.trimmed_len, x.leading_zeros < y.leading_zeros ? x.leading_zeros : y.leading_zeros,
                        x.nonzero + y.nonzero};
}
SV_HD bool fr_mem_is_zero(const fr_mem_t* p) {
    const uint4* q = (const uint4*)p;
    const uint4 lo = q[0], hi = q[1];
    return ((lo.x | lo.y | lo.z | lo.w) | (hi.x | hi.y | hi.z | hi.w)) == 0;
}
SV_HD fr_support_t fr_support_thread(const fr_mem_t* v, size_t n, size_t first, size_t step) {
    fr_support_t s = fr_support_identity(n);
    for (size_t i = first; i < n; i += step) {
        if (fr_mem_is_zero(&v[i])) continue;
        if (!s.nonzero) s.leading_zeros = i;  // a thread walks upwards
        s.trimmed_len = i + 1;
        s.nonzero++;
    }
    return s;
}
// launch 2's walk over the partials of launch 1
SV_HD fr_support_t fr_support_fold(const uint64_t* parts, size_t nparts, size_t n, size_t first, size_t step) {
    fr_support_t s = fr_support_identity(n);
    for (size_t k = first; k < nparts; k += step) s = fr_support_combine(s, fr_support_t{parts[3 * k], parts[3 * k + 1], parts[3 * k + 2]});
    return s;
}

#if defined(__HIPCC__)
// Butterfly over the lanes l ^ off, off = from .. 1: every lane ends with the combination of its aligned group of 2 * from lanes.  All 64 lanes of
// the wave take part (no thread of these kernels leaves before the trees).  The nine 29-bit limbs travel as they are: packing them into the 8
// memory words and back costs more VALU work than the ninth exchange saves.
__device__ __forceinline__ fr_t fr_lanes_sum(fr_t v, int from) {
#pragma unroll 1
    for (int off = from; off >= 1; off >>= 1) {
        fr_t o;
#pragma unroll
        for (int l = 0; l < 9; l++) o.v[l] = (uint32_t)__shfl_xor((int)v.v[l], off);
        v = v + o;
    }
    return v;
}
__device__ __forceinline__ fr_support_t fr_lanes_support(fr_support_t s, int from) {
#pragma unroll 1
    for (int off = from; off >= 1; off >>= 1) {
        fr_support_t o;
        o.trimmed_len = (uint64_t)__shfl_xor((unsigned long long)s.trimmed_len, off);
        o.leading_zeros = (uint64_t)__shfl_xor((unsigned long long)s.leading_zeros, off);
        o.nonzero = (uint64_t)__shfl_xor((unsigned long long)s.nonzero, off);
        s = fr_support_combine(s, o);
    }
    return s;
}
// the workgroup's value in (at least) thread 0; blockDim.x = 64, 128 or 256; sh: 9 words per wave, limb-major like horner2_lds_put
__device__ __forceinline__ fr_t fr_block_sum(fr_t v, uint32_t* sh) {
    v = fr_lanes_sum(v, 32);
    const uint32_t nw = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (nw == 1) return v;
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < 9; l++) sh[l * nw + w] = v.v[l];
    }
    __syncthreads();
    fr_t u = fr_t::zero();
    if (lane < nw) {
#pragma unroll
        for (int l = 0; l < 9; l++) u.v[l] = sh[l * nw + lane];
    }
    return fr_lanes_sum(u, (int)(nw >> 1));
}
__device__ __forceinline__ fr_support_t fr_block_support(fr_support_t s, uint64_t* sh, size_t n) {
    s = fr_lanes_support(s, 32);
    const uint32_t nw = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (nw == 1) return s;
    if (lane == 0) sh[3 * w] = s.trimmed_len, sh[3 * w + 1] = s.leading_zeros, sh[3 * w + 2] = s.nonzero;
    __syncthreads();
    fr_support_t u = fr_support_identity(n);
    if (lane < nw) u = fr_support_t{sh[3 * lane], sh[3 * lane + 1], sh[3 * lane + 2]};
    return fr_lanes_support(u, (int)(nw >> 1));
}
// partials[y * gridDim.x + x]: the value of workgroup x over batch member y, internal limbs stored raw; b == nullptr for OP = SUM;
// stride_b == 0: every member is multiplied by the same b
template <int OP>
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_reduce_kernel(const fr_mem_t* __restrict__ a, const fr_mem_t* __restrict__ b, size_t n, size_t stride_a,
                                                                       size_t stride_b, fr_mem_t* __restrict__ partials) {
    __shared__ uint32_t sh[9 * (FR_REDUCE_B / 64)];
    a += (size_t)blockIdx.y * stride_a;
    if (OP == FR_REDUCE_DOT) b += (size_t)blockIdx.y * stride_b;
    fr_t v = fr_reduce_thread<OP>(a, b, n, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
    v = fr_block_sum(v, sh);
    if (threadIdx.x == 0) v.store(&partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x]);
}
// out[y] = the sum of member y's nparts partials, as a memory-form element; grid (1, members)
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_reduce_final_kernel(int op, const fr_mem_t* __restrict__ partials, size_t nparts, fr_mem_t* __restrict__ out) {
    __shared__ uint32_t sh[9 * (FR_REDUCE_B / 64)];
    fr_t v = fr_reduce_thread<FR_REDUCE_SUM>(partials + (size_t)blockIdx.y * nparts, nullptr, nparts, threadIdx.x, blockDim.x);
    v = fr_block_sum(v, sh);
    if (threadIdx.x == 0) fr_reduce_finish(op, v).store(&out[blockIdx.y]);
}
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_support_kernel(const fr_mem_t* __restrict__ v, size_t n, size_t stride, uint64_t* __restrict__ partials) {
    __shared__ uint64_t sh[3 * (FR_REDUCE_B / 64)];
    fr_support_t s = fr_support_thread(v + (size_t)blockIdx.y * stride, n, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
    s = fr_block_support(s, sh, n);
    if (threadIdx.x == 0) {
        uint64_t* p = partials + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        p[0] = s.trimmed_len, p[1] = s.leading_zeros, p[2] = s.nonzero;
    }
}
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_support_final_kernel(const uint64_t* __restrict__ partials, size_t nparts, size_t n, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh[3 * (FR_REDUCE_B / 64)];
    fr_support_t s = fr_support_fold(partials + 3 * (size_t)blockIdx.y * nparts, nparts, n, threadIdx.x, blockDim.x);
    s = fr_block_support(s, sh, n);
    if (threadIdx.x == 0) {
        uint64_t* p = out + 3 * (size_t)blockIdx.y;
        p[0] = s.trimmed_len, p[1] = s.leading_zeros, p[2] = s.nonzero;
    }
}
#endif

// ---- evaluation: many polynomials, each at its point -> one value each ----------------------------------------------------------
// p_k(z_k) = sum_i c_k[i] z_k^i (DensePolynomial::evaluate, dense.rs:98-114; the `evaluations` of a proof, varuna.rs:583-592, and by linearity
// every get_lc_eval, ahp.rs:469-487): the member of the reduction family above that carries the powers of the point.  The same two launches:
//   launch 1  fr_evaluate_kernel: grid (blocks, members of this launch), T = blocks x blockDim threads per member.  Thread t owns the indices
//             t, t + T, t + 2T, ... of its member - coalesced like fr_reduce_thread - and forms sum_j c[t + jT] Z^j with Z = z^T by a Horner walk
//             from the top: FR_EVALUATE_G coefficients and the accumulator per step through ONE Fp::sum_of_products with {1, Z, .., Z^G}
//             (G + 1 products and one Montgomery reduction per G coefficients; the partial top group goes by single Horner steps).  The factor
//             z^t is split by linearity: a thread multiplies its value by z^threadIdx.x, the workgroup's sum - fr_block_sum, as in
//             fr_reduce_kernel - is multiplied by z^(blockIdx.x blockDim.x) ONCE, by thread 0, and that is the partial it writes.  Both factors
//             are ONE product each against a table in lane workspace (per point blockDim + gridDim entries, 72 KB for the full grid), which
//   launch 0  fr_evaluate_powers_kernel fills from the set bits of the exponent against z^(2^i): at most 18 products per entry, once per point
//             and launch instead of 8 per thread and 11 per workgroup of launch 1 - at proof sizes a thread owns one to eight coefficients, and
//             forming its power in place (FR_EVALUATE_POW 0, measured: profiles/fr_evaluate.md) costs more than its whole walk.
//   launch 2  fr_reduce_final_kernel (op SUM) folds the `blocks` partials of every member: the existing combine, no twin.
// A workgroup that lies wholly behind the end of its member sums zeros and writes a zero partial; no atomics; field addition is exact, so the 32
// bytes of a result depend on neither T, the split into launches nor the grouping of the points.
// Representation.  Coefficients are streamed RAW: the memory image of c, read as an internal value, is "shifted" (the top of this file).  Every
// power of a point in the table (z^(2^i), Z^g, and the 1 of the group) is in the TRUE internal form - the host ran from_mem_mont on the point
// ONCE per distinct point, the single fix-up of this pass - so every product here is (true) x (shifted) = shifted, sums of shifted values are
// shifted, and what thread 0 stores is the memory image of the result: neither kernel converts anything (launch 2 runs with op SUM, whose
// fr_reduce_finish is the identity).  sum_of_products' operand conditions hold: the first factors are table entries (canonical), the second
// are memory images (< 2^256) or the accumulator (canonical).
// 0^0 = 1 falls out: for z = 0 every table entry but the group's 1 is zero, thread 0 of workgroup 0 has no bit set and keeps c[0], everything
// else is multiplied by zero.  Length 0: every thread is behind the end.
// The table travels BY KERNEL ARGUMENT like fr_lincomb_t: a member is its pointer, its length, the index of its point in the launch and the row
// of its partials (its place in the caller's list, < 65536); pointers, lengths and powers are wave-uniform scalar loads.  A list with more
// members or more distinct points than one table holds takes further launches; launch 2 runs once over all rows.
#ifndef FR_EVALUATE_G
#define FR_EVALUATE_G 4  // coefficients per Montgomery reduction; a -D override (with the one below) builds the variants tools/bench_fr_evaluate.py compares
#endif
#ifndef FR_EVALUATE_POW
#define FR_EVALUATE_POW 2  // how z^t is formed - 2: the two factors from the table of launch 0; 0: the same two factors from the set bits, in place; 1: every thread forms all of z^t
#endif
static_assert(FR_EVALUATE_POW >= 0 && FR_EVALUATE_POW <= 2, "FR_EVALUATE_POW: 0, 1 or 2");
static_assert(FR_EVALUATE_G >= 1 && FR_EVALUATE_G <= 5, "fr_evaluate_walk: G coefficients and the accumulator share one sum_of_products (at most 6 terms)");
static constexpr int FR_EVALUATE_MEMBERS = 64;  // per launch
static constexpr int FR_EVALUATE_POINTS = 3;    // distinct points per launch
static constexpr int FR_EVALUATE_BITS = 19;     // t < FR_REDUCE_BLOCKS_MAX x FR_REDUCE_B = 2^19
static_assert((uint64_t)FR_REDUCE_BLOCKS_MAX * FR_REDUCE_B <= (uint64_t)1 << FR_EVALUATE_BITS, "fr_evaluate_scale: every thread index must fit the table of z^(2^i)");
struct fr_evaluate_point_t {
    uint32_t pw[FR_EVALUATE_BITS][9];   // z^(2^i), true internal form
    uint32_t Z[FR_EVALUATE_G + 1][9];   // Z^g, g = 0 .. G, Z = z^T: true internal form (Z[0] is the internal 1)
};
struct fr_evaluate_t {  // 64 x 16 B + 3 x (19 + 5) x 36 B + 8 = 3624 B of the 4 KB of kernel arguments
    const fr_mem_t* p[FR_EVALUATE_MEMBERS];
    uint32_t len[FR_EVALUATE_MEMBERS];
    uint16_t point[FR_EVALUATE_MEMBERS];  // index into pt
    uint16_t row[FR_EVALUATE_MEMBERS];    // partials[row * blocks + workgroup]
    fr_evaluate_point_t pt[FR_EVALUATE_POINTS];
    uint32_t count, points;  // members and points in use
};
// sum_j c[first + j step] Z^j over the indices below n, a shifted value; zero for a thread behind the end
SV_HD fr_t fr_evaluate_walk(const fr_mem_t* c, size_t n, size_t first, size_t step, const fr_evaluate_point_t& P) {
    constexpr int G = FR_EVALUATE_G;
    if (first >= n) return fr_t::zero();
    const size_t cnt = (n - first + step - 1) / step;  // the indices this thread owns
    size_t j = cnt;
    fr_t acc = fr_t::zero();
    if (j % G) {  // the partial top group by single Horner steps, down to a multiple of G; the top coefficient itself costs no product
        const fr_t Z1 = fr_t::from_table(P.Z[1]);
        acc = fr_t::load(&c[first + --j * step]);
#pragma unroll 1
        for (; j % G; j--) acc = fr_t::load(&c[first + (j - 1) * step]) + acc * Z1;
    }
    fr_t x[G + 1], y[G + 1];
#pragma unroll
    for (int g = 0; g <= G; g++) x[g] = fr_t::from_table(P.Z[g]);
#pragma unroll 1
    for (; j; j -= G) {  // whole groups below: acc <- acc Z^G + sum_g c[j - G + g] Z^g
#pragma unroll
        for (int g = 0; g < G; g++) y[g] = fr_t::load(&c[first + (j - G + g) * step]);
        y[G] = acc;
        acc = fr_t::sum_of_products<G + 1>(x, y);
    }
    return acc;
}
// v z^e over the set bits of e < 2^FR_EVALUATE_BITS
SV_HD fr_t fr_evaluate_scale(fr_t v, const fr_evaluate_point_t& P, uint32_t e) {
#pragma unroll 1
    for (int i = 0; e >> i; i++)
        if ((e >> i) & 1) v = v * fr_t::from_table(P.pw[i]);
    return v;
}
// The table of launch 0 for a grid of gdim workgroups of bdim threads: point q owns the bdim + gdim entries from q (bdim + gdim) on - entry
// e < bdim is z^e (thread e's factor), entry bdim + x is z^(x bdim) (workgroup x's factor).  Entries are TRUE internal values, bit-packed
// into 32 bytes by store() and taken back by load() (pure repacking of a canonical value: not a memory-form element).
SV_HD size_t fr_evaluate_table_size(uint32_t bdim, uint32_t gdim) { return FR_EVALUATE_POW == 2 ? (size_t)FR_EVALUATE_POINTS * (bdim + gdim) : 0; }
SV_HD fr_t fr_evaluate_table_entry(const fr_evaluate_point_t& P, uint32_t e, uint32_t bdim) {
    return fr_evaluate_scale(fr_t::one(), P, e < bdim ? e : (e - bdim) * bdim);
}
// what thread `tid` of workgroup x (bdim threads, gdim workgroups) contributes for member y of the table, and what thread 0 does to the
// workgroup's sum: the kernel below and the host replay (snarkvm_hip_selftest_fr_evaluate) both call them
SV_HD fr_t fr_evaluate_thread(const fr_evaluate_t& t, const fr_mem_t* tab, uint32_t y, uint32_t x, uint32_t tid, uint32_t bdim, uint32_t gdim) {
    const fr_evaluate_point_t& P = t.pt[t.point[y]];
    const fr_t v = fr_evaluate_walk(t.p[y], t.len[y], (size_t)x * bdim + tid, (size_t)gdim * bdim, P);
    if (FR_EVALUATE_POW == 2) return v * fr_t::load(&tab[(size_t)t.point[y] * (bdim + gdim) + tid]);
    return fr_evaluate_scale(v, P, FR_EVALUATE_POW == 0 ? tid : x * bdim + tid);
}
SV_HD fr_t fr_evaluate_block(const fr_evaluate_t& t, const fr_mem_t* tab, uint32_t y, uint32_t x, uint32_t bdim, uint32_t gdim, const fr_t& sum) {
    if (FR_EVALUATE_POW == 2) return sum * fr_t::load(&tab[(size_t)t.point[y] * (bdim + gdim) + bdim + x]);
    return FR_EVALUATE_POW == 0 ? fr_evaluate_scale(sum, t.pt[t.point[y]], x * bdim) : sum;
}
#if defined(__HIPCC__)
// launch 0: grid (ceil((bdim + gdim) / blockDim), points of the table); bdim, gdim: the geometry of launch 1
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_evaluate_powers_kernel(fr_mem_t* __restrict__ tab, uint32_t bdim, uint32_t gdim, fr_evaluate_t t) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < bdim + gdim) fr_evaluate_table_entry(t.pt[blockIdx.y], e, bdim).store(&tab[(size_t)blockIdx.y * (bdim + gdim) + e]);
}
// partials[row * gridDim.x + x]: the value of workgroup x over the member, stored raw (the memory image of its share of the result)
static __global__ void __launch_bounds__(FR_REDUCE_B) fr_evaluate_kernel(fr_mem_t* __restrict__ partials, const fr_mem_t* __restrict__ tab, fr_evaluate_t t) {
    __shared__ uint32_t sh[9 * (FR_REDUCE_B / 64)];
    fr_t v = fr_evaluate_thread(t, tab, blockIdx.y, blockIdx.x, threadIdx.x, blockDim.x, gridDim.x);
    v = fr_block_sum(v, sh);
    if (threadIdx.x == 0)
        fr_evaluate_block(t, tab, blockIdx.y, blockIdx.x, blockDim.x, gridDim.x, v).store(&partials[(size_t)t.row[blockIdx.y] * gridDim.x + blockIdx.x]);
}
#endif

// ---- sparse matrix times vector over a registered matrix -----------------------------------------------------------------
// y = M x for an R1CS matrix M in CSR form (z_M = M z, snark/varuna/ahp/prover/round_functions/mod.rs:131-188) or for its transpose
// (M(alpha, .) = M^T l_alpha, third.rs:303-306).  R1CS rows hold a handful of entries, but a transposed matrix has a few rows - the column of
// the constant one, of heavily used variables - that collect a large share of all non-zeros, so work is laid out by ENTRIES, on the host, once,
// when the matrix is registered (api_varuna.hip: fr_spmv_layout):
//   segments  every row is cut into segments of at most `seg` entries: table of fr_spmv_seg_t {row, first entry, count, part}.  part ==
//             FR_SPMV_SOLE: the only segment of its row; otherwise the slot of this segment's partial sum (a row's slots are consecutive, in
//             segment order).
//   fix-ups   table of fr_spmv_fix_t {row, first slot, slots}: every row that has no segment (slots == 0) or more than one.
//   launch 1  fr_spmv_seg_kernel<W>: one group of W lanes (4, 8, 16 or 64: chosen per matrix from its mean segment length, fr_spmv_width) per
//             segment.  Lanes stride over the segment's entries: vals[k] is read coalesced (32 B per lane), x[col_idx[k]] is gathered; raw
//             products go FR_REDUCE_G at a time through Fp::sum_of_products like the inner product's (fr_reduce_group: the same operand
//             conditions, the value is the first factor), the group folds by the butterfly of fr_lanes_sum.  A sole segment's lane 0 stores
//             y[row]; any other stores its partial, internal limbs raw.
//   launch 2  fr_spmv_fix_kernel<W>: one group per fix-up adds that row's partials (none: zero) and stores y[row]; the groups behind the table
//             store the zeros of the tail y[rows .. n_out).  So every element of y is written exactly once, by exactly one lane, without a fill.
// blockIdx.y is the batch member (x + y * stride_x, stride_x == 0: one shared x; y + y * stride_y; partial slots + y * nparts).  No atomics: which
// group finishes first never enters a result, and since field addition is exact and results canonical the 32 bytes of y[r] depend on neither
// `seg`, W nor the grid (the host replay, snarkvm_hip_selftest_fr_spmv, walks any seg and W through the routines below).
// As in fr_reduce, raw(val) * raw(x) is the internal form of val x 2^-10 and one from_mem_mont per stored y[r] undoes it (multiplication by a
// constant commutes with the sums, so partials stay raw).
// Registers (gfx950, -O3): fr_spmv_seg_kernel 128 VGPRs for every W, fr_spmv_fix_kernel 62, no scratch, no call (tools/device_calls.sh).
static constexpr uint32_t FR_SPMV_SOLE = 0xFFFFFFFFu;
static constexpr int FR_SPMV_B = 256;  // threads per workgroup of both launches
#ifndef FR_SPMV_SEG
#define FR_SPMV_SEG 128  // entries per segment: measured against 256 and 512 (profiles/fr_spmv.md); a -D override builds the variants tools/bench_fr_spmv.py compares
#endif
struct fr_spmv_seg_t {
    uint32_t row, first, count, part;
};
struct fr_spmv_fix_t {
    uint32_t row, first, count, pad;
};
// lanes per segment for a matrix of nnz entries in nseg segments: the narrowest group whose lanes each get at most one sum_of_products group
// out of a segment of the mean length
SV_HD uint32_t fr_spmv_width(size_t nnz, size_t nseg) {
#ifdef FR_SPMV_WIDTH  // a -D override, like FR_SPMV_SEG: one width for every matrix
    return FR_SPMV_WIDTH;
#else
    const size_t mean = nseg ? (nnz + nseg - 1) / nseg : 0;
    return mean <= 4 * FR_REDUCE_G ? 4 : (mean <= 8 * FR_REDUCE_G ? 8 : (mean <= 16 * FR_REDUCE_G ? 16 : 64));
#endif
}
// G entries at k, k + step, ... of one segment: sum of vals[k] * x[col[k]], unreduced to memory form
template <int G>
SV_HD fr_t fr_spmv_group(const fr_mem_t* vals, const uint32_t* col, const fr_mem_t* x, size_t k, size_t step) {
    fr_t a[G], b[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        a[g] = fr_t::load(&vals[k + g * step]);
        b[g] = fr_t::load(&x[col[k + g * step]]);
    }
    return fr_t::sum_of_products<G>(a, b);
}
// the private accumulation of lane `lane` of a group of `width` over a segment of `count` entries (vals, col: at the segment's first entry):
// whole groups, then single entries
SV_HD fr_t fr_spmv_lane(const fr_mem_t* vals, const uint32_t* col, const fr_mem_t* x, size_t count, size_t lane, size_t width) {
    fr_t acc = fr_t::zero();
    size_t k = lane;
#pragma unroll 1
    for (; k < count && count - k > (FR_REDUCE_G - 1) * width; k += FR_REDUCE_G * width) acc = acc + fr_spmv_group<FR_REDUCE_G>(vals, col, x, k, width);
#pragma unroll 1
    for (; k < count; k += width) acc = acc + fr_spmv_group<1>(vals, col, x, k, width);
    return acc;
}
// what turns a (sum of) raw product(s) into the memory form of y[r]
SV_HD fr_t fr_spmv_finish(const fr_t& total) { return total.from_mem_mont(); }

#if defined(__HIPCC__)
// grid (ceil(nseg / (FR_SPMV_B / W)), members).  Every lane stays until after the butterfly (groups behind the table add zeros).
template <int W>
static __global__ void __launch_bounds__(FR_SPMV_B) fr_spmv_seg_kernel(const fr_spmv_seg_t* __restrict__ segs, size_t nseg, const fr_mem_t* __restrict__ vals,
                                                                       const uint32_t* __restrict__ col, const fr_mem_t* __restrict__ x, size_t stride_x,
                                                                       fr_mem_t* __restrict__ y, size_t stride_y, fr_mem_t* __restrict__ parts, size_t nparts) {
    const size_t g = (blockIdx.x * (size_t)FR_SPMV_B + threadIdx.x) / W;
    const uint32_t lane = threadIdx.x % W;
    const bool live = g < nseg;
    fr_spmv_seg_t s{0, 0, 0, FR_SPMV_SOLE};
    if (live) s = segs[g];
    fr_t v = fr_spmv_lane(vals + s.first, col + s.first, x + (size_t)blockIdx.y * stride_x, s.count, lane, W);
    v = fr_lanes_sum(v, W / 2);
    if (!live || lane) return;
    if (s.part == FR_SPMV_SOLE)
        fr_spmv_finish(v).store(&y[(size_t)blockIdx.y * stride_y + s.row]);
    else
        v.store(&parts[(size_t)blockIdx.y * nparts + s.part]);
}
// grid (ceil((nfix + n_out - rows) / (FR_SPMV_B / W)), members): group g < nfix folds fix-up g, group nfix + t zeroes y[rows + t]
template <int W>
static __global__ void __launch_bounds__(FR_SPMV_B) fr_spmv_fix_kernel(const fr_spmv_fix_t* __restrict__ fix, size_t nfix, const fr_mem_t* __restrict__ parts,
                                                                       size_t nparts, fr_mem_t* __restrict__ y, size_t stride_y, size_t rows, size_t n_out) {
    const size_t g = (blockIdx.x * (size_t)FR_SPMV_B + threadIdx.x) / W;
    const uint32_t lane = threadIdx.x % W;
    fr_spmv_fix_t f{0, 0, 0, 0};
    if (g < nfix) f = fix[g];
    fr_t v = fr_reduce_thread<FR_REDUCE_SUM>(parts + (size_t)blockIdx.y * nparts + f.first, nullptr, f.count, lane, W);
    v = fr_lanes_sum(v, W / 2);
    if (lane) return;
    if (g < nfix)
        fr_spmv_finish(v).store(&y[(size_t)blockIdx.y * stride_y + f.row]);
    else if (g - nfix < n_out - rows)
        fr_t::zero().store(&y[(size_t)blockIdx.y * stride_y + rows + (g - nfix)]);
}
#endif

// ---- Varuna round 4: the matrix-sumcheck evaluations on K over a registered arithmetization ---------------------------------
// calculate_matrix_sumcheck_witness (round_functions/fourth.rs:155-245) per matrix M: with r, c, v = row, col, row_col_val at kappa in K
// (ahp/matrices.rs:101-195) and d = (alpha - r)(beta - c) - the reference forms this element twice, as the product for f and expanded as
// alpha beta - beta r - alpha c + r c for b -
//   a = a_scale v,   b = b_scale d,   f = f_scale v / d   (f = 0 where d = 0: batch_inversion_and_mul leaves zeros, fields/src/lib.rs:66-129).
// One fused pass instead of a dozen fr_vec_op / fr_batch_inversion_and_mul launches: Montgomery's trick per thread over the strided set
// {t, t + T, ...} as in fr_batch_inverse_kernel, the forward sweep forming d from row and col and parking the running product, the backward
// sweep emitting a, b and f.  The running products are parked IN THE f OUTPUT ITSELF: a thread owns its indices, reads slot i - T before it
// writes f[i] and has read slot i one step earlier, so the pass needs no workspace at all; a call that wants no f skips the sweep and the inversion.
// blockIdx.y is the batch member (the matrices A, B, C of one circuit: members of different lengths, the same alpha, beta and scales); the member
// table and the constants travel BY KERNEL ARGUMENT like fr_lincomb_t (nothing staged, nothing to release after an enqueue-only call).
// Forms (top of this file): alpha - r and beta - c are differences of raw ("shifted") values, their product p is the internal form of d 2^-10.
// The chain of products, its Fermat inverse and the unwinding run on p as it is; the powers of two this leaves behind are folded into the three
// constants ONCE, on the host (fr_sumcheck_consts): a = raw(v) * A, b = p * B, f = raw(v) * (inv_i * F-carried) are memory-form values, canonical
// like every product.  7 products per element and one inversion (~300) per thread.
// Geometry (fr_sumcheck_share): the Fermat inversion is a chain of ~300 DEPENDENT products that every thread pays, so the pass is bound by that
// latency until the chip is full; a member gets FR_SUMCHECK_THREADS threads (three members: 768 waves over the 1024 SIMDs) and the share per thread
// grows with k between FR_SUMCHECK_E_MIN and FR_SUMCHECK_E_MAX - 8 at |K| = 2^17, 32 from 2^19 on, where the work and not the latency decides.
// Measured against the 32 per thread of fr_batch_inverse_run and against smaller shares: profiles/fr_sumcheck.md (tools/bench_fr_sumcheck.py).
static constexpr int FR_SUMCHECK_B = 256;       // threads per workgroup
static constexpr int FR_SUMCHECK_MEMBERS = 16;  // members per call: 16 x 64 B + 180 B of the 4 KB of kernel arguments
#ifndef FR_SUMCHECK_THREADS
#define FR_SUMCHECK_THREADS 16384  // threads per member the share is sized for; a -D override (with the two below) builds the variants tools/bench_fr_sumcheck.py compares
#endif
#ifndef FR_SUMCHECK_E_MIN
#define FR_SUMCHECK_E_MIN 4
#endif
#ifndef FR_SUMCHECK_E_MAX
#define FR_SUMCHECK_E_MAX 32
#endif
// elements per thread for a member of k elements; the member runs T = ceil(k / share) threads (no cap: 2^28 / 32 threads are 32 768 workgroups)
SV_HD size_t fr_sumcheck_share(size_t k) {
    const size_t e = (k + FR_SUMCHECK_THREADS - 1) / FR_SUMCHECK_THREADS;
    return e < FR_SUMCHECK_E_MIN ? FR_SUMCHECK_E_MIN : (e > FR_SUMCHECK_E_MAX ? FR_SUMCHECK_E_MAX : e);
}
SV_HD size_t fr_sumcheck_threads(size_t k) {
    const size_t e = fr_sumcheck_share(k);
    return (k + e - 1) / e;
}
struct fr_sumcheck_consts_t {
    uint32_t alpha[9], beta[9];  // raw limbs of the memory images
    uint32_t a[9];               // a_scale, true internal form:      raw(v) * a = memory form of a_scale v
    uint32_t b[9];               // b_scale 2^266:                    p * b      = memory form of b_scale d
    uint32_t f[9];               // f_scale 2^251:                    carried by the inverse, raw(v) * (f / p) = memory form of f_scale v / d
};
// alpha, beta: memory images; scales: a_scale, b_scale, f_scale
SV_HD fr_sumcheck_consts_t fr_sumcheck_consts(const fr_mem_t& alpha, const fr_mem_t& beta, const fr_mem_t* scales) {
    fr_sumcheck_consts_t cs;
    const fr_t al = fr_t::load(&alpha), be = fr_t::load(&beta);
    const fr_t a = fr_t::load(&scales[0]).from_mem_mont();
    const fr_t b = fr_t::load(&scales[1]).from_mem_mont().from_mem_mont();
    const fr_t f = fr_t::load(&scales[2]) * fr_t::one().to_mem_mont();  // raw(x) * 2^256 2^-261 = x 2^251
    for (int l = 0; l < 9; l++) cs.alpha[l] = al.v[l], cs.beta[l] = be.v[l], cs.a[l] = a.v[l], cs.b[l] = b.v[l], cs.f[l] = f.v[l];
    return cs;
}
struct fr_sumcheck_member_t {
    const fr_mem_t *row, *col, *rcv;  // the registered arithmetization, k elements each
    fr_mem_t *a, *b, *f;              // outputs, k elements each; nullptr: skipped
    size_t k, T;                      // thread t < T owns t, t + T, ... < k
};
struct fr_sumcheck_t {
    fr_sumcheck_member_t m[FR_SUMCHECK_MEMBERS];
    fr_sumcheck_consts_t cs;
};
// the whole work of thread t of a member: the kernel below and the host replay (snarkvm_hip_selftest_fr_sumcheck) both call it
SV_HD void fr_sumcheck_thread(const fr_sumcheck_member_t& m, const fr_sumcheck_consts_t& cs, size_t t) {
    const size_t k = m.k, T = m.T;
    if (t >= T || t >= k) return;
    const fr_t alpha = fr_t::from_table(cs.alpha), beta = fr_t::from_table(cs.beta);
    fr_t inv = fr_t::zero();
    if (m.f) {
        fr_t run = fr_t::one();
        bool any = false;
#pragma unroll 1
        for (size_t i = t; i < k; i += T) {
            const fr_t p = (alpha - fr_t::load(&m.row[i])) * (beta - fr_t::load(&m.col[i]));
            if (!p.is_zero()) {
                run = run * p;
                any = true;
            }
            run.store(&m.f[i]);
        }
        if (any) inv = run.inverse() * fr_t::from_table(cs.f);
    }
    const fr_t as = fr_t::from_table(cs.a), bs = fr_t::from_table(cs.b);
    const size_t cnt = (k - t + T - 1) / T;
#pragma unroll 1
    for (size_t j = cnt; j-- > 0;) {
        const size_t i = t + j * T;
        const fr_t v = fr_t::load(&m.rcv[i]);
        if (m.a) (v * as).store(&m.a[i]);
        if (!m.b && !m.f) continue;
        const fr_t p = (alpha - fr_t::load(&m.row[i])) * (beta - fr_t::load(&m.col[i]));
        if (m.b) (p * bs).store(&m.b[i]);
        if (!m.f) continue;
        fr_t fv = fr_t::zero();
        if (!p.is_zero()) {  // a zero neither entered the chain nor leaves it: its neighbours see the product of the others
            const fr_t s = j ? fr_t::load(&m.f[i - T]) : fr_t::one();
            fv = v * (inv * s);
            inv = inv * p;
        }
        fv.store(&m.f[i]);
    }
}
#if defined(__HIPCC__)
// grid (ceil(max_m T_m / FR_SUMCHECK_B), members): a workgroup behind its member's last thread leaves at once
static __global__ void __launch_bounds__(FR_SUMCHECK_B) fr_sumcheck_evals_kernel(fr_sumcheck_t tab) {
    fr_sumcheck_thread(tab.m[blockIdx.y], tab.cs, blockIdx.x * (size_t)FR_SUMCHECK_B + threadIdx.x);
}
#endif

// ---- the circuit index: the arithmetization of a CSR matrix on K ---------------------------------------------------------------------
// matrix_evals (ahp/matrices.rs:138-195): entry e = (val, j) of row i gives row[e] = w_R^i, col[e] = w_C^reindex(j) with
// EvaluationDomain::reindex_by_subdomain (fft/domain.rs:322-344), row_col[e] = row[e] col[e], row_col_val[e] = val row_col[e]; the places
// nnz <= e < k hold (1, 1, 1, 0).  A map: one thread per output element, grid-stride past the launch cap.
// Row lookup: the row of entry e is the one i with row_ptr[i] <= e < row_ptr[i + 1] - an upper-bound binary search over row_ptr, ~lg(rows)
// dependent 8-byte loads of an array that stays in cache (neighbouring threads walk the same path).  Runs of empty rows give equal pointers;
// the search keeps the SMALLEST i with row_ptr[i + 1] > e, which is the one row that owns the entry.
// Powers: w^x for an arbitrary x < 2^lg is lo[x & (2^s - 1)] * hi[x >> s] over two tables of 2^s and 2^(lg - s) entries (s = ceil(lg / 2):
// at most 2 * 2^14 elements per domain, cache-resident), built by fr_arith_tables_kernel in the calling lane's workspace.  Forms (top of this
// file): lo holds memory images (raw reads are shifted values), hi TRUE internal values, so lo * hi is the memory form of the power with no
// fix-up.  The product P of the two memory images row and col is the internal form of row col 2^-10: row_col = P * MEM2INT, and
// row_col_val = (raw(val) * P) * MEM2INT^2 with the second constant formed once on the host - row, col, P, row_col and two for row_col_val:
// SIX products per entry with all four outputs, five without row_col (registration), of which four are the function's own and the rest
// the price of streaming every vector in memory form.  The exponent is masked to the domain (w^(2^lg) = 1), so no index - whatever col_idx
// holds - reads outside a table.  Field arithmetic is exact and every product canonical: the bytes depend on neither s, the thread count nor
// the grid (the host twin, snarkvm_hip_selftest_fr_arithmetize, replays forced geometries through fr_arith_at).
// No atomics, no device-function call, no scratch.  Registers (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): fr_arithmetize_kernel 51 VGPRs,
// 106 SGPRs (3 spilled to VGPR lanes), 7 waves per SIMD; fr_arith_tables_kernel 38 VGPRs.
// Two measurement variants, built by tools/bench_fr_arithmetize.py alone (-D, never the product library and no tuning key): FR_ARITH_FULL_TABLE reads
// w_C^x from ONE table of |V| elements (fr_distribute_powers) without a product; FR_ARITH_ROW_INDEX reads the row of entry e from a host-expanded
// uint32 array laid behind row_ptr instead of searching.  What has been measured of both is in profiles/fr_arithmetize.md.
#ifndef FR_ARITH_FULL_TABLE
#define FR_ARITH_FULL_TABLE 0
#endif
#ifndef FR_ARITH_ROW_INDEX
#define FR_ARITH_ROW_INDEX 0
#endif
struct fr_arith_t {
    fr_mem_t *row, *col, *row_col, *rcv;  // outputs, k elements each; nullptr: skipped
    const uint64_t* row_ptr;              // rows + 1 values
    const uint32_t* col_idx;
    const fr_mem_t* vals;
    const fr_mem_t *r_lo, *r_hi, *c_lo, *c_hi;  // the power tables of the constraint and the variable domain
    fr_mem_t one;                               // memory image of 1 (padding)
    uint32_t fix2[9];                           // MEM2INT^2, true internal form
    uint32_t k, rows;
    uint32_t s_r, mask_r, s_c, mask_c;  // table split and 2^lg - 1 per domain
    uint32_t input_size, period;        // |X| and |V| / |X| >= 2
};
// ceil(lg / 2): the split the launch uses
SV_HD uint32_t fr_arith_split(uint32_t lg) { return (lg + 1) / 2; }
// entry t of the two tables of one domain (t < 2^s + 2^(lg - s)): lo[x] = w^x as a memory image, hi[y] = w^(y 2^s) in true internal form
SV_HD void fr_arith_table_at(fr_mem_t* lo, fr_mem_t* hi, const fr_t& omega, uint32_t s, uint32_t t) {
    const uint32_t n_lo = 1u << s;
    if (t < n_lo)
        omega.pow_u64(t).to_mem_mont().store(&lo[t]);
    else
        omega.pow_u64((uint64_t)(t - n_lo) << s).store(&hi[t - n_lo]);
}
SV_HD uint32_t fr_arith_reindex(uint32_t j, uint32_t input_size, uint32_t period) {
    if (j < input_size) return j * period;
    const uint32_t t = j - input_size;
    return t + t / (period - 1) + 1;
}
// the smallest i < rows with row_ptr[i + 1] > e; the caller vouches for e < row_ptr[rows]
SV_HD uint32_t fr_arith_row_of(const uint64_t* row_ptr, uint32_t rows, uint32_t e) {
    uint32_t lo = 0, hi = rows - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (row_ptr[mid + 1] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}
// output element e < k; nnz = min(row_ptr[rows], k)
SV_HD void fr_arith_at(const fr_arith_t& a, uint32_t nnz, uint32_t e) {
    if (e >= nnz) {
        if (a.row) a.row[e] = a.one;
        if (a.col) a.col[e] = a.one;
        if (a.row_col) a.row_col[e] = a.one;
        if (a.rcv) fr_t::zero().store(&a.rcv[e]);
        return;
    }
#if FR_ARITH_ROW_INDEX
    const uint32_t xr = ((const uint32_t*)(a.row_ptr + a.rows + 1))[e] & a.mask_r;
#else
    const uint32_t xr = fr_arith_row_of(a.row_ptr, a.rows, e) & a.mask_r;
#endif
    const uint32_t xc = fr_arith_reindex(a.col_idx[e], a.input_size, a.period) & a.mask_c;
    const fr_t row = fr_t::load(&a.r_lo[xr & ((1u << a.s_r) - 1)]) * fr_t::load(&a.r_hi[xr >> a.s_r]);
#if FR_ARITH_FULL_TABLE
    const fr_t col = fr_t::load(&a.c_lo[xc]);
#else
    const fr_t col = fr_t::load(&a.c_lo[xc & ((1u << a.s_c) - 1)]) * fr_t::load(&a.c_hi[xc >> a.s_c]);
#endif
    if (a.row) row.store(&a.row[e]);
    if (a.col) col.store(&a.col[e]);
    if (!a.row_col && !a.rcv) return;
    const fr_t p = row * col;
    if (a.row_col) p.from_mem_mont().store(&a.row_col[e]);
    if (a.rcv) ((fr_t::load(&a.vals[e]) * p) * fr_t::from_table(a.fix2)).store(&a.rcv[e]);
}
#if defined(__HIPCC__)
static __global__ void __launch_bounds__(256) fr_arith_tables_kernel(fr_mem_t* lo, fr_mem_t* hi, fr_mem_t omega_mem, uint32_t s, uint32_t entries) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < entries) fr_arith_table_at(lo, hi, fr_t::load(&omega_mem).from_mem_mont(), s, t);
}
static __global__ void __launch_bounds__(256) fr_arithmetize_kernel(fr_arith_t a) {
    const uint64_t total = a.row_ptr[a.rows];
    const uint32_t nnz = total < a.k ? (uint32_t)total : a.k;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < a.k; i += st) fr_arith_at(a, nnz, (uint32_t)i);
}
#endif

}  // namespace sv
