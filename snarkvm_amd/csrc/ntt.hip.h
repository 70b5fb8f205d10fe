// ntt.hip.h - radix-2 NTT / iNTT over BLS12-377 Fr for gfx950.
//
// Replaces (behaviour, not code): sppark's NTT::Base / NTT_internal / bit_rev as called from
// algorithms/cuda/cuda/snarkvm.cu:154-186 and polynomial.cuh:104-266, and the CPU transforms of
// algorithms/src/fft/domain.rs:374-443 (in_order_fft / ifft / coset_ifft), :691-773 (io/oi helpers).
//
// Structure (MI355X-first): a 2^lg transform is split into at most three passes of radix <= 2^9 up to 2^27, four passes of radix 2^7
// at 2^28 ("four-step" decomposition applied recursively).  One workgroup stages a [2^a rows] x [T columns]
// tile of 32-byte elements in LDS (<= 64 KiB), runs the a radix-2 DIF stages there with __syncthreads
// between stages, and writes the tile back:
//   * non-last pass: in place (same addresses), each element multiplied by the inter-pass twiddle
//     w_L^(inner*k) looked up from a two-level power table (2 x 8192 entries, L2-resident);
//   * last pass: rows are contiguous; the output index is digit-reversed so the result lands in
//     natural (NN) order.  This pass is out-of-place (another workgroup still needs the slots it
//     would overwrite), hence the ping-pong with a scratch buffer in ntt_run().
// Every pass reads and writes each element exactly once in >= 256-byte contiguous runs, so HBM traffic is
// passes * 2 * 32 * n bytes (algorithmic minimum 2 * 32 * n: SURVEY.md 8d).  Twiddles are never
// streamed from HBM: per-stage twiddles come from a 256-entry table of w_512 powers staged in LDS.
//
// Exponents: a twiddle exponent is counted in powers of W28 (primitive 2^28-th root, e < 2^28).  The two-level tables hold powers
// of W26 = W28^4 and cover e >> 2; a four-entry table W28^(0..3) covers e & 3.  That last factor is only ever != 1 in 2^27 and 2^28
// transforms, so every smaller transform reads the same table words with the same products as before.  Coset powers g^j likewise:
// j & 8191, (j >> 13) & 8191 from the two-level tables, g^(2^26 (j >> 26)) from a four-entry table.
// Data stays in the reference's memory form (Montgomery, R = 2^256) throughout; see ff.hip.h for why the
// 29-bit-limb arithmetic needs no conversion on this (linear) path.
#pragma once
#include <mutex>
#include <type_traits>
#include <vector>

#include "ff.hip.h"
#include "tuning.hip.h"

namespace sv {

static constexpr int NTT_LG_MAX = 28;     // the SRS maximum (8 GiB vectors); larger domains: the caller's CPU path
static constexpr int NTT_TW_LG = 26;      // the two-level tables hold powers of W26 = W28^4: exponents < 2^26
static constexpr int NTT_TW_BITS = 13;    // w^e = hi[e >> 13] * lo[e & 8191]
static constexpr int NTT_TW_SIZE = 1 << NTT_TW_BITS;
static constexpr int NTT_TOP = 1 << (NTT_LG_MAX - NTT_TW_LG);  // entries of the top tables: W28^t, g^(2^26 t)
static constexpr int NTT_MAX_PASSES = 4;
static constexpr int NTT_MAX_RADIX_LG = 9;  // passes of radix <= 2^8 up to 2^24; 2^25 - 2^27 use radix-2^9 passes on narrower tiles
static constexpr int NTT_LOCAL = 1 << (NTT_MAX_RADIX_LG - 1);  // per-stage twiddles: powers of w_512 staged in LDS

// order / direction / type enums: algorithms/cuda/src/lib.rs:22-40
enum { NTT_NN = 0, NTT_NR = 1, NTT_RN = 2, NTT_RR = 3 };
enum { NTT_FORWARD = 0, NTT_INVERSE = 1 };
enum { NTT_STANDARD = 0, NTT_COSET = 1 };

// Device-resident tables (internal Montgomery form, packed 32 B per entry).
struct ntt_tables_t {
    fr_mem_t* pow_lo[2];   // [dir][8192]  W26^(+-i)        W26 = primitive 2^26-th root of unity
    fr_mem_t* pow_hi[2];   // [dir][8192]  W26^(+-8192 i)
    fr_mem_t* pow_top[2];  // [dir][4]     W28^(+-t)        W28 = primitive 2^28-th root, W28^4 = W26
    fr_mem_t* local[2];    // [dir][NTT_LOCAL]   w_512^(+-i)
    fr_mem_t* g_lo[2];     // [0]: g^i  [1]: g^-i          g = 22 (fr.rs:126-135)
    fr_mem_t* g_hi[2];     //      g^(+-8192 i)
    fr_mem_t* g_top[2];    //      g^(+-2^26 t)
    fr_mem_t* size_inv;    // [NTT_LG_MAX + 1]  (2^lg)^-1
    fr_mem_t* consts;      // scratch for the set-up kernels
};

// TWO_ADIC_ROOT_OF_UNITY (fr.rs:115-120), memory form (a * 2^256), 32-bit words -> primitive 2^lg-th root, internal form
SV_HD fr_t ntt_root_of_unity(int lg) {
    const uint32_t FR_TWO_ADIC_ROOT_MEM[8] = {0xda3ad648u, 0xaf80da4du, 0xfc381dacu, 0x5e223adbu,
                                              0xb2f92525u, 0x03ba0666u, 0x3befb0ceu, 0x0f906c5bu};
    fr_t w = fr_t::unpack(FR_TWO_ADIC_ROOT_MEM).from_mem_mont();  // 2^47-th root
    for (int i = 0; i < 47 - lg; i++) w = w.sqr();
    return w;
}

// The table set-up, shared by the device (ntt_setup_consts / ntt_fill_tables) and the host self-test (snarkvm_hip_selftest_ntt_twiddle).
// consts[0] = W26, [1] = W26^-1, [2] = g, [3] = g^-1; the top tables and size_inv[0..NTT_LG_MAX]
SV_HD void ntt_setup_consts_on(const ntt_tables_t& t) {
    const fr_t w28 = ntt_root_of_unity(NTT_LG_MAX);
    fr_t w = w28;
    for (int i = 0; i < NTT_LG_MAX - NTT_TW_LG; i++) w = w.sqr();  // -> W26
    fr_t g = fr_t::from_u32(22);
    w.store(&t.consts[0]);
    w.inverse().store(&t.consts[1]);
    g.store(&t.consts[2]);
    g.inverse().store(&t.consts[3]);
    const fr_t w28i = w28.inverse(), g26 = g.pow_u64((uint64_t)1 << NTT_TW_LG), g26i = g26.inverse();
    fr_t p[4] = {fr_t::one(), fr_t::one(), fr_t::one(), fr_t::one()};
    for (int i = 0; i < NTT_TOP; i++) {
        p[0].store(&t.pow_top[0][i]);
        p[1].store(&t.pow_top[1][i]);
        p[2].store(&t.g_top[0][i]);
        p[3].store(&t.g_top[1][i]);
        p[0] = p[0] * w28, p[1] = p[1] * w28i, p[2] = p[2] * g26, p[3] = p[3] * g26i;
    }
    fr_t half = fr_t::from_u32(2).inverse();
    fr_t cur = fr_t::one();
    for (int lg = 0; lg <= NTT_LG_MAX; lg++) {
        cur.store(&t.size_inv[lg]);
        cur = cur * half;
    }
}
// lo[i] = b^i, hi[i] = b^(8192 i) for the four bases; local[dir][i] = (W26^+-1)^(2^17 i)
SV_HD void ntt_fill_tables_at(const ntt_tables_t& t, int i) {
    for (int which = 0; which < 4; which++) {
        fr_t b = fr_t::load(&t.consts[which]);
        fr_mem_t* lo = which < 2 ? t.pow_lo[which] : t.g_lo[which - 2];
        fr_mem_t* hi = which < 2 ? t.pow_hi[which] : t.g_hi[which - 2];
        b.pow_u64((uint64_t)i).store(&lo[i]);
        b.pow_u64((uint64_t)i << NTT_TW_BITS).store(&hi[i]);
        if (which < 2 && i < NTT_LOCAL) b.pow_u64((uint64_t)i << (NTT_TW_LG - NTT_MAX_RADIX_LG)).store(&t.local[which][i]);
    }
}
static __global__ void ntt_setup_consts(ntt_tables_t t) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ntt_setup_consts_on(t);
}
static __global__ void ntt_fill_tables(ntt_tables_t t) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NTT_TW_SIZE) return;
    ntt_fill_tables_at(t, i);
}

// ---- twiddle and coset-power composition (host and device) ----
// W28^e, e < 2^28: lo[(e >> 2) & 8191] * hi[e >> 15] * top[e & 3]; a factor whose index is 0 (the value one) is skipped, so an
// exponent that is a multiple of 4 and below 2^15 costs no product at all
struct ntt_pow_idx_t {
    uint32_t lo, hi, top;
};
SV_HD ntt_pow_idx_t ntt_tw_index(uint32_t e) {
    const uint32_t e26 = e >> (NTT_LG_MAX - NTT_TW_LG);
    return ntt_pow_idx_t{e26 & (NTT_TW_SIZE - 1), e26 >> NTT_TW_BITS, e & (NTT_TOP - 1)};
}
// g^j, j < 2^28: lo[j & 8191] * hi[(j >> 13) & 8191] * top[j >> 26]
SV_HD ntt_pow_idx_t ntt_coset_index(uint32_t j) {
    return ntt_pow_idx_t{j & (NTT_TW_SIZE - 1), (j >> NTT_TW_BITS) & (NTT_TW_SIZE - 1), j >> NTT_TW_LG};
}
SV_HD fr_t ntt_pow_compose(const fr_mem_t* lo, const fr_mem_t* hi, const fr_mem_t* top, ntt_pow_idx_t x) {
    fr_t w = fr_t::load(&lo[x.lo]);
    if (x.hi) w = w * fr_t::load(&hi[x.hi]);
    if (x.top) w = w * fr_t::load(&top[x.top]);
    return w;
}
// W28^(+-e) (dir) and g^(+-j) (inv) from the device's tables
SV_HD fr_t ntt_twiddle(const ntt_tables_t& tb, int dir, uint32_t e) { return ntt_pow_compose(tb.pow_lo[dir], tb.pow_hi[dir], tb.pow_top[dir], ntt_tw_index(e)); }
SV_HD fr_t ntt_coset_pow(const ntt_tables_t& tb, int inv, uint32_t j) { return ntt_pow_compose(tb.g_lo[inv], tb.g_hi[inv], tb.g_top[inv], ntt_coset_index(j)); }

struct ntt_pass_t {
    const fr_mem_t* in;
    fr_mem_t* out;
    int lg_n;        // transform size
    int a;           // log2 radix of this pass
    int s;           // log2 inner stride (non-last pass); 0 for the last pass
    int lgT;         // log2 tile width
    int last;        // 1: last pass
    int a1;          // last pass: log2 size of the leading digit (tile dimension); 0 for a single-pass transform
    int lg_mid;      // last pass: log2 size of the middle digits (three- and four-pass transforms), else 0
    int mid_lo;      // last pass of a four-pass transform: log2 size of the second middle digit (the lower one in memory), else 0
    int dir;         // NTT_FORWARD / NTT_INVERSE
    int coset_pre;   // multiply input j by g^j        (forward coset, first pass)
    int scale_post;  // last pass: 0 none, 1 * n^-1, 2 * g^-k n^-1   (inverse / coset inverse)
    int tw_shift;    // non-last: twiddle exponent (in powers of W28) = (inner * k) << tw_shift
    const fr_mem_t* tw_full;  // non-last, optional: the closing twiddles of this pass, tw_full[(k << s) + inner] (one product instead of two)
    int reduce_only; // last pass: the previous pass' closing table already carries 2^261 (and n^-1 when inverse): the final
                     // multiplication by one / n^-1 shrinks to a bare Montgomery reduction
};

SV_HD uint32_t bitrev32(uint32_t x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    return bits ? (__brev(x) >> (32 - bits)) : 0u;
#else
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
#endif
}

// ---- a non-last pass' tile (host and device): columns inner0 .. inner0 + 2^lgT - 1 of block `outer`; row j of column c is read from
// in_base + (j << s) + c, and output digit k is stored at in_base + (k << s) + c
struct ntt_inner_tile_t {
    size_t inner0, in_base;
};
SV_HD ntt_inner_tile_t ntt_inner_tile(const ntt_pass_t& p, size_t tile) {
    const size_t tiles_per_outer = (size_t)1 << (p.s - p.lgT);
    const size_t outer = tile / tiles_per_outer;
    ntt_inner_tile_t t;
    t.inner0 = (tile % tiles_per_outer) << p.lgT;
    t.in_base = (outer << (p.a + p.s)) + t.inner0;
    return t;
}

// ---- the last pass' index map (host and device) ----
// After the passes before it, position (k0 << (lg - a1)) + (mid << a) + j holds the partial sums of output digits k0 (the first pass'),
// the middle digits `mid` and input row j of the last pass.  Three passes: mid = k1.  Four passes: mid = k1 * 2^mid_lo + k2 in memory,
// and the output wants k1 + k2 * 2^(lg_mid - mid_lo).  Output index = k0 + (mid' + k * 2^lg_mid) * 2^a1 with k = bitrev_a(row).
struct ntt_last_tile_t {
    size_t d1_0;     // first leading digit (column 0) of the tile
    size_t in_base;  // input position of (row 0, column 0)
    size_t mid_out;  // the middle digits in output order
};
SV_HD ntt_last_tile_t ntt_last_tile(const ntt_pass_t& p, size_t tile) {
    const size_t tiles_per_mid = (size_t)1 << (p.a1 - p.lgT);
    const size_t mid = tile / tiles_per_mid;
    ntt_last_tile_t t;
    t.d1_0 = (tile % tiles_per_mid) << p.lgT;
    t.in_base = (t.d1_0 << (p.lg_n - p.a1)) + (mid << p.a);
    const size_t k2 = mid & (((size_t)1 << p.mid_lo) - 1);
    t.mid_out = (mid >> p.mid_lo) + (k2 << (p.lg_mid - p.mid_lo));
    return t;
}
SV_HD size_t ntt_last_out(const ntt_pass_t& p, const ntt_last_tile_t& t, int col, uint32_t k) {
    return (t.d1_0 + col) + ((t.mid_out + ((size_t)k << p.lg_mid)) << p.a1);
}
// (tile, row, column) -> output index, row = the tile row after the pass' DIF stages
SV_HD size_t ntt_last_out_index(const ntt_pass_t& p, size_t tile, int row, int col) {
    return ntt_last_out(p, ntt_last_tile(p, tile), col, bitrev32((uint32_t)row, p.a));
}

// ------------------------------------------------------------------------------------------
// v2 pass kernel: radix-4 butterflies in registers + lazy reduction.
//   * two DIF stages per LDS round trip (a = 8: 4 groups, 3 round trips instead of 8), the first group reads
//     straight from global memory and the last one writes straight back;
//   * the tile lives in LDS as 29-bit limbs, 9 consecutive words per element (no pack / unpack between stages);
//   * butterflies use lazy arithmetic (ff.hip.h): sums are only carry-normalised, differences add 2^s * r, products
//     skip the conditional subtraction.  Bound: entering local stage s every value is < 2^s * r (inputs canonical),
//     so after a <= 8 stages values are < 256 r < 2^261 (9 limbs).  The closing multiplication (inter-pass twiddle,
//     1/n scaling, or the constant one) brings the value below 2r and one conditional subtraction makes it
//     canonical again before it is stored.  (Radix-2^9 passes, used from 2^25: the top limb holds the 262nd bit and the
//     closing product is < 2.17 r - two conditional subtractions.)
// ------------------------------------------------------------------------------------------
struct ntt_lds_t {
    uint32_t* data;  // E elements of 9 limbs each (stride 9 words is coprime to the bank count; the limb offsets are immediates)
    uint32_t* tw;    // 9 planes of NL = 2^(a-1) limbs: the powers of this pass' own root w_(2^a) (internal form)
    int NL;
    int E;
    template <class E>  // fr_t: nine 32-bit words
    __device__ __forceinline__ E get(int e) const {
        E x;
#pragma unroll
        for (int l = 0; l < 9; l++) x.v[l] = static_cast<typename std::remove_reference<decltype(x.v[0])>::type>(data[e * 9 + l]);
        return x;
    }
    template <class E>
    __device__ __forceinline__ void put(int e, const E& x) const {
#pragma unroll
        for (int l = 0; l < 9; l++) data[e * 9 + l] = (uint32_t)x.v[l];
    }
    __device__ __forceinline__ fr_t twiddle(int idx) const {
        fr_t x;
#pragma unroll
        for (int l = 0; l < 9; l++) x.v[l] = tw[l * NL + idx];
        return x;
    }
};

// One DIF stage inside a register group: x[lo_m], x[lo_m | bit] -> (u + v, (u - v + 2^s r) * w)
__device__ __forceinline__ void lazy_butterfly(fr_t& u, fr_t& v, int s, int tw_idx, const ntt_lds_t& L) {
    uint32_t kp[9];
    fr_t::mod_shl(kp, s);  // 2^s * r
    const fr_t sum = fr_t::add_lazy(u, v);
    fr_t dif = fr_t::sub_lazy(u, v, kp);
    if (tw_idx != 0) dif = dif.mul_lazy(L.twiddle(tw_idx));
    u = sum;
    v = dif;
}

// The arithmetic of a pass: the unsigned lazy routines of round 3.  tw(): a word of the ff.hip.h twiddle tables (w * 2^261) in the
// form mul() wants.  (A signed-limb twin of this struct was measured and retired: HISTORY.md, "retired variants".)
struct ntt_arith_u {
    typedef fr_t elem;
    __device__ __forceinline__ static elem from_canonical(const fr_t& x) { return x; }
    __device__ __forceinline__ static void butterfly(elem& u, elem& v, int s, int tw_idx, const ntt_lds_t& L) { lazy_butterfly(u, v, s, tw_idx, L); }
    __device__ __forceinline__ static fr_t tw(const fr_t& w_int) { return w_int; }
    __device__ __forceinline__ static fr_t one() { return fr_t::one(); }
    __device__ __forceinline__ static elem mul(const elem& x, const fr_t& w) { return x.mul_lazy(w); }
    __device__ __forceinline__ static elem reduce_only(const elem& x) { return x.mont_reduce_lazy(); }
    // a radix-2^9 pass ends with values < 2^9 r = 1.17 * 2^261: the closing product is < 2.17 r, one more conditional subtraction
    __device__ __forceinline__ static fr_t finish(const elem& y, int a) {
        fr_t z = y.reduce_lazy();
        if (a > 8) z = z.reduce_lazy();
        return z;
    }
};

__device__ __forceinline__ fr_t load_fr_global(const fr_mem_t* p) {
    const uint4* src = (const uint4*)p;
    const uint4 x0 = src[0], x1 = src[1];
    const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    return fr_t::unpack(w);
}
__device__ __forceinline__ void store_fr_global(fr_mem_t* p, const fr_t& x) {
    uint32_t w[8];
    x.pack(w);
    uint4* dst = (uint4*)p;
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// K stages (1 or 2) on the 2^K rows {base_row + m * row_step}; s = index of the first of them within the pass.
template <int K, class A>
__device__ __forceinline__ void dif_group(typename A::elem* x, int s, int a, int lo, const ntt_lds_t& L) {
    // rows of the group differ in the K bits just below bit (a - s); `lo` = the row bits below them
    const int lo_bits = a - s - K;
#pragma unroll
    for (int t = 0; t < K; t++) {
        const int bit = 1 << (K - 1 - t);  // group-local index bit paired at stage s + t
#pragma unroll
        for (int m = 0; m < (1 << K); m++) {
            if (m & bit) continue;
            // pos = row mod half, half = 2^(a - 1 - (s + t)): the group-local bits below `bit`, then `lo`
            const int pos = ((m & (bit - 1)) << lo_bits) | lo;
            const int tw_idx = pos << (s + t);  // exponent of w_(2^a)
            A::butterfly(x[m], x[m | bit], s + t, tw_idx, L);
        }
    }
}

// Batched launches (snarkvm_hip_ntt_device_batch: the independent transforms of a prover round, or of many proofs in lock step):
// blockIdx.y selects the vector.  Vector y lives at v[y]; its private scratch copy at scratch + (y << lg_n).  The pointers travel
// as kernel arguments (no device-side table to keep alive while calls are in flight); more than NTT_BATCH_MAX vectors = several launches.
static constexpr int NTT_BATCH_MAX = 48;
struct ntt_batch_t {
    fr_mem_t* v[NTT_BATCH_MAX];
    fr_mem_t* scratch;
    int in_scratch, out_scratch;
};
struct ntt_no_batch_t {};

// Load policies: what the first stage group of a pass - the only place that touches global input - reads at global index g.
//   ntt_load_plain    in[g]: every transform of the NTT entry points.
//   ntt_load_bounded  in[g] for g < len, zero beyond: the forward transform of a coefficient-form operand of len <= 2^lg elements, read
//                     where the caller keeps it (never written, never read past len).  Batched form only: src[y] / len[y] per operand,
//                     the pass writes to scratch slot y or to v[y] like any batched pass.
//   ntt_load_product  v[0][g] * ... * v[m - 1][g] over m <= NTT_PROD_MAX full-length vectors in memory form: the inverse transform of a
//                     pointwise product without the pass that would materialise it.  A Montgomery product of two memory words is short of
//                     the memory form by 2^5 (fr_pointwise_mul_kernel); `fix` = 2^(5 (m - 1)) in internal form restores it with ONE
//                     product for the whole chain.  Every product is canonical, so A::from_canonical sees what a plain load gives it.
static constexpr int NTT_PROD_MAX = 4;
struct ntt_bounded_t : ntt_batch_t {
    const fr_mem_t* src[NTT_BATCH_MAX];
    size_t len[NTT_BATCH_MAX];
};
struct ntt_product_t {
    const fr_mem_t* v[NTT_PROD_MAX];
    int m;
    fr_mem_t fix;  // used when m >= 2
};
struct ntt_load_plain {
    template <bool BATCH>
    using args = typename std::conditional<BATCH, ntt_batch_t, ntt_no_batch_t>::type;
};
struct ntt_load_bounded {
    template <bool BATCH>
    using args = ntt_bounded_t;
};
struct ntt_load_product {
    template <bool BATCH>
    using args = ntt_product_t;
};
// 2^(5 (m - 1)) in internal form: MEM2INT = 2^266, and mont261(2^(261 + 5 i), 2^266) = 2^(261 + 5 (i + 1))
SV_HD ntt_product_t ntt_product_args(const fr_mem_t* const* v, int m) {
    ntt_product_t pa{};
    for (int j = 0; j < NTT_PROD_MAX; j++) pa.v[j] = j < m ? v[j] : nullptr;
    pa.m = m;
    fr_t fix = fr_t::from_table(FrP::MEM2INT);
    for (int j = 2; j < m; j++) fix = fix * fr_t::from_table(FrP::MEM2INT);
    fix.store(&pa.fix);
    return pa;
}
__device__ __forceinline__ fr_t ntt_product_at(const ntt_product_t& pa, size_t g) {
    fr_t x = load_fr_global(&pa.v[0][g]);
    if (pa.m > 1) {
#pragma unroll
        for (int j = 1; j < NTT_PROD_MAX; j++)
            if (j < pa.m) x = x * load_fr_global(&pa.v[j][g]);
        x = x * fr_t::load(&pa.fix);
    }
    return x;
}

template <bool BATCH, class A, class LD = ntt_load_plain>
__global__ void __launch_bounds__(512) ntt_pass_kernel_v2(ntt_pass_t p, ntt_tables_t tb, typename LD::template args<BATCH> bt) {
    typedef typename A::elem elem;
    constexpr bool BOUNDED = std::is_same<LD, ntt_load_bounded>::value, PRODUCT = std::is_same<LD, ntt_load_product>::value;
    static_assert(!BOUNDED || BATCH, "the bounded load takes its operands from the batch arguments");
    static_assert(!PRODUCT || !BATCH, "the product load is a single transform");
    extern __shared__ uint32_t lds32[];
    if constexpr (BATCH) {
        fr_mem_t* vec = bt.v[blockIdx.y];
        fr_mem_t* scr = bt.scratch + ((size_t)blockIdx.y << p.lg_n);
        p.in = bt.in_scratch ? scr : vec;
        p.out = bt.out_scratch ? scr : vec;
    }
    size_t in_len = 0;
    if constexpr (BOUNDED) {
        p.in = bt.src[blockIdx.y];
        in_len = bt.len[blockIdx.y];
    }
    (void)in_len;
    const int R = 1 << p.a, T = 1 << p.lgT, E = R << p.lgT;
    ntt_lds_t L;
    L.data = lds32;
    L.tw = lds32 + 9 * E;
    L.NL = p.a ? (1 << (p.a - 1)) : 1;
    L.E = E;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const size_t tile = blockIdx.x;

    // ---- addressing (as in v1)
    size_t in_base, in_rho_stride, in_col_stride;
    size_t inner0 = 0;
    ntt_last_tile_t lt{};
    if (!p.last) {
        const ntt_inner_tile_t it = ntt_inner_tile(p, tile);
        inner0 = it.inner0;
        in_base = it.in_base;
        in_rho_stride = (size_t)1 << p.s;
        in_col_stride = 1;
    } else {
        lt = ntt_last_tile(p, tile);
        in_base = lt.in_base;
        in_rho_stride = 1;
        in_col_stride = (size_t)1 << (p.lg_n - p.a1);
    }
    // local twiddles -> LDS planes
    for (int i = tid; i < L.NL; i += nthr) {  // w_(2^a)^i = w_512^(i << (9 - a))
        const fr_t w = A::tw(fr_t::load(&tb.local[p.dir][i << (NTT_MAX_RADIX_LG - p.a)]));
#pragma unroll
        for (int l = 0; l < 9; l++) L.tw[l * L.NL + i] = w.v[l];
    }
    __syncthreads();

    // ---- stage groups: pairs of stages, a single stage first when a is odd
    int s = 0;
    bool first = true;
    while (s < p.a) {
        const int K = ((p.a - s) & 1) ? 1 : 2;
        const bool last_group = (s + K == p.a);
        const int lo_bits = p.a - s - K;
        const int ngroups = E >> K;
        for (int gi = tid; gi < ngroups; gi += nthr) {
            // non-last passes keep `col` fastest (coalesced rows of T elements); the last pass keeps the row fastest
            int col, q;
            if (!p.last || !first) {
                col = gi & (T - 1);
                q = gi >> p.lgT;
            } else {
                q = gi & ((R >> K) - 1);
                col = gi >> (p.a - K);
            }
            const int lo = q & ((1 << lo_bits) - 1);
            const int hi = q >> lo_bits;
            const int row0 = (hi << (p.a - s)) | lo;
            const int row_step = 1 << lo_bits;
            elem x[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (m >= (1 << K)) break;
                const int row = row0 + m * row_step;
                if (first) {
                    const size_t g = in_base + row * in_rho_stride + col * in_col_stride;
                    fr_t xin;
                    if constexpr (BOUNDED)
                        xin = g < in_len ? load_fr_global(&p.in[g]) : fr_t::zero();
                    else if constexpr (PRODUCT)
                        xin = ntt_product_at(bt, g);
                    else
                        xin = load_fr_global(&p.in[g]);
                    if (p.coset_pre) xin = xin * ntt_coset_pow(tb, 0, (uint32_t)g);
                    x[m] = A::from_canonical(xin);
                } else {
                    x[m] = L.get<elem>(row * T + col);
                }
            }
            if (K == 2)
                dif_group<2, A>(x, s, p.a, lo, L);
            else
                dif_group<1, A>(x, s, p.a, lo, L);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (m >= (1 << K)) break;
                const int row = row0 + m * row_step;
                if (!last_group) {
                    L.put<elem>(row * T + col, x[m]);
                    continue;
                }
                // ---- closing multiplication + store; row `row` holds output digit k = bitrev_a(row)
                const uint32_t k = bitrev32((uint32_t)row, p.a);
                size_t g;
                elem y;
                if (!p.last) {
                    g = in_base + ((size_t)k << p.s) + col;
                    if (p.tw_full) {
                        y = A::mul(x[m], fr_t::load(&p.tw_full[((size_t)k << p.s) + inner0 + col]));  // the table holds the arithmetic's own form
                    } else {
                        // composed on the fly from the power tables (no table fits: the first pass of a 2^26 - 2^28 transform)
                        const uint32_t expo = (uint32_t)(((inner0 + col) * (size_t)k) << p.tw_shift);
                        y = A::mul(x[m], A::tw(ntt_twiddle(tb, p.dir, expo)));
                    }
                } else {
                    g = ntt_last_out(p, lt, col, k);
                    y = x[m];
                    if (!p.reduce_only) y = A::mul(y, p.scale_post == 0 ? A::one() : A::tw(fr_t::load(&tb.size_inv[p.lg_n])));
                    if (p.scale_post == 2) {  // times 22^-g for output index g: one closing product per table factor
                        const ntt_pow_idx_t gi = ntt_coset_index((uint32_t)g);
                        y = A::mul(y, A::tw(fr_t::load(&tb.g_lo[1][gi.lo])));
                        if (gi.hi) y = A::mul(y, A::tw(fr_t::load(&tb.g_hi[1][gi.hi])));
                        if (gi.top) y = A::mul(y, A::tw(fr_t::load(&tb.g_top[1][gi.top])));
                    }
                    if (p.reduce_only) y = A::reduce_only(y);
                }
                const fr_t z = A::finish(y, p.a);
                store_fr_global(&p.out[g], z);
            }
        }
        __syncthreads();
        s += K;
        first = false;
    }
}

// out[i] = in[bitrev(i)]   (sppark `bit_rev`, polynomial.cuh:128,189; domain.rs:797-804 derange)
static __global__ void ntt_bitrev_kernel(const fr_mem_t* in, fr_mem_t* out, int lg_n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << lg_n)) return;
    size_t r = lg_n ? (size_t)(__brevll((unsigned long long)i) >> (64 - lg_n)) : 0;
    const uint4* s = (const uint4*)&in[r];
    uint4* d = (uint4*)&out[i];
    d[0] = s[0];
    d[1] = s[1];
}
// polynomial_inner_multiply (polynomial.cuh:36-45): out[i] = a[i] * b[i] (memory Montgomery form, R = 2^256).
// mont261(x, y) = x y 2^-261 = (a b 2^256) 2^-5, so `fix` = 2^(5 + 261) mod r restores the form (see ff.hip.h);
// with fix_later the factor is left for the caller to fold into a later constant.
static __global__ void fr_pointwise_mul_kernel(fr_mem_t* out, const fr_mem_t* a, const fr_mem_t* b, size_t n, int fix_now) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) {
        fr_t x = fr_t::load(&a[i]) * fr_t::load(&b[i]);
        if (fix_now) x = x.from_mem_mont();  // * 2^266 * 2^-261 = * 2^5
        x.store(&out[i]);
    }
}
// out[i] = v[0][i] * ... * v[m - 1][i] in memory form, the product load of the pass kernel as a pass of its own: folds a group of factors
// into an accumulator when a product has more factors than one load takes.  `out` may be one of the factors.
static __global__ void fr_product_kernel(fr_mem_t* out, ntt_product_t pa, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) store_fr_global(&out[i], ntt_product_at(pa, i));
}
// Fr::to_bigint (fp_256.rs:380-413) / from_bigint (fp_256.rs:362-377) over a vector: kzg10 convert_to_bigints
static __global__ void fr_to_bigint_kernel(fr_mem_t* out, const fr_mem_t* in, size_t n, int to_bigint) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t st = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += st) {
        fr_t x = fr_t::load(&in[i]);
        // memory Montgomery a*2^256 -> a : internal(x) = mem * 2^5 ... use explicit forms:
        //   to_bigint:   a = mont261(mem, 2^261 * 2^-256 = 2^5)
        //   from_bigint: a -> internal a*2^261 (times R2) -> memory a*2^256 (times INT2MEM)
        if (to_bigint) {
            fr_t c = fr_t::zero();
            c.v[0] = 32;  // 2^5 as a plain integer
            x = x * c;
        } else {
            x = x.int_to_mont().to_mem_mont();  // a -> a*2^261 -> a*2^256
        }
        x.store(&out[i]);
    }
}

// ------------------------------------------------------------------------------------------
// Host-side driver
// ------------------------------------------------------------------------------------------
struct ntt_plan_t {
    int npass;
    int a[NTT_MAX_PASSES];
};
// npass = 0: lg is out of range
SV_HD ntt_plan_t ntt_make_plan(int lg) {
    ntt_plan_t pl;
    constexpr int R8 = 8;  // preferred pass radix: a [2^8 x 8] tile is 72 KiB of LDS, two workgroups per CU
    pl.npass = 0;
    for (int i = 0; i < NTT_MAX_PASSES; i++) pl.a[i] = 0;
    if (lg < 0 || lg > NTT_LG_MAX) {
        return pl;
    } else if (lg <= R8) {
        pl.npass = 1;
        pl.a[0] = lg;
    } else if (lg <= 2 * R8) {
        pl.npass = 2;
        pl.a[0] = lg / 2;
        pl.a[1] = lg - pl.a[0];
    } else if (lg <= 3 * NTT_MAX_RADIX_LG) {  // up to 3 * 9 = 27 bits; 2^25 - 2^27 get one to three radix-2^9 passes
        pl.npass = 3;
        pl.a[0] = lg / 3;
        pl.a[1] = (lg - pl.a[0]) / 2;
        pl.a[2] = lg - pl.a[0] - pl.a[1];
    } else {  // 2^28: 7 + 7 + 7 + 7 (the lazy bound and tile shapes of the 2^21 plan; a radix-2^10 pass would break the bound)
        pl.npass = 4;
        for (int i = 0; i < 4; i++) pl.a[i] = (lg + i) / 4;
    }
    return pl;
}
// the geometry of pass k of plan `pl` for a 2^lg transform (everything but the buffers, the tile width and the direction / type fields)
SV_HD ntt_pass_t ntt_pass_geometry(const ntt_plan_t& pl, int lg, int k) {
    ntt_pass_t p{};
    p.lg_n = lg;
    p.a = pl.a[k];
    p.last = (k == pl.npass - 1);
    int consumed = 0;
    for (int i = 0; i < k; i++) consumed += pl.a[i];
    if (!p.last) {
        p.s = lg - consumed - p.a;
        p.tw_shift = NTT_LG_MAX - (p.a + p.s);  // W28^(x << tw_shift) = w_(2^(a + s))^x
    } else {
        p.a1 = (pl.npass >= 2) ? pl.a[0] : 0;
        p.lg_mid = 0;
        for (int i = 1; i + 1 < pl.npass; i++) p.lg_mid += pl.a[i];
        p.mid_lo = (pl.npass == 4) ? pl.a[2] : 0;
    }
    return p;
}
// tile width (log2) of a pass of radix 2^a whose tile dimension offers `avail` bits: [2^a x 2^lgT] elements of 36 bytes must
// fit the 96 KiB the pass kernel may use
// Small transforms (the 2^14 - 2^18 domains of a proof) would fill only 8 ... 128 of the chip's 256 CUs with [2^a x 8] tiles, and a
// thread's work does not depend on the tile width (one radix-4 group per stage round): such passes take narrower tiles until
// the launch has ntt_min_tiles workgroups (tuning.hip.h; the data is L2 resident at these sizes, so the shorter
// coalesced runs of a narrow tile cost nothing).
static inline int ntt_min_tiles() {
    return tuning().ntt_min_tiles;
}
static inline int ntt_tile_lg(int a, int avail, int lg_n, size_t nvec = 1) {
    int lgT = avail < 3 ? avail : 3;
    while (lgT > 0 && a + lgT > 11) lgT--;
    while (lgT > 0 && (((size_t)1 << (lg_n - a - lgT)) * nvec) < (size_t)ntt_min_tiles()) lgT--;  // a batched launch covers the chip with wide tiles sooner
    return lgT;
}

// ---- full closing-twiddle tables ----------------------------------------------------------------------------------
// The closing multiplication of a non-last pass needs W^((inner * k) << tw_shift); composing it from the two 4096-entry
// tables costs a second Fr product per element, and the NTT is ALU-bound: skipping that product is worth 9 %
// of a 2^24 transform.  So the composed twiddles of a pass shape (a, s, direction) are materialised in HBM, in exactly the
// order the pass stores its outputs (coalesced 32-byte reads next to the 32-byte stores): 2^(a+s) entries - 512 MiB for the
// first pass of a 2^24 transform, 2 MiB for its second pass.  The tables live in a per-device cache bounded by
// SNARKVM_HIP_NTT_TW_MB (default 1536 MiB): least recently used tables that no running call holds are evicted; when nothing
// can be evicted (or tuning ntt_full_tw=0) the pass composes its twiddles on the fly.
struct ntt_tw_entry {
    fr_mem_t* p = nullptr;
    size_t bytes = 0;
    uint64_t last_use = 0;
    int users = 0;
};
struct ntt_tw_cache_t {
    ntt_tw_entry ptr[2][NTT_MAX_RADIX_LG + 1][NTT_LG_MAX + 1];  // [dir][a][a + s]
    // the table of the pass BEFORE the last one, with 2^261 (forward) or 2^261 / n (inverse) folded in, per transform size:
    // the last pass then ends with Fp::mont_reduce_lazy() instead of a product by one / by n^-1
    ntt_tw_entry prelast[2][NTT_LG_MAX + 1];
    std::mutex mu;
    size_t bytes = 0;
    uint64_t tick = 0;
    template <class Fn>
    void for_each(Fn fn) {
        for (auto& d : ptr)
            for (auto& a : d)
                for (auto& e : a) fn(e);
        for (auto& d : prelast)
            for (auto& e : d) fn(e);
    }
};
// what a transform needs from its caller: the stream, the device's small tables, its twiddle cache, and the list of cache
// entries the call holds until its stream has been synchronised (released by ntt_tw_release)
struct ntt_ctx_t {
    hipStream_t st;
    const ntt_tables_t* tb;
    ntt_tw_cache_t* cache;
    std::vector<void*>* leases;
};
// fold: 0 plain, 1 times 2^261, 2 times 2^261 * size_inv (size_inv points at the Montgomery form of n^-1)
static __global__ void ntt_fill_full_tw_kernel(fr_mem_t* __restrict__ out, int a, int s, int tw_shift, const fr_mem_t* __restrict__ lo,
                                        const fr_mem_t* __restrict__ hi, const fr_mem_t* __restrict__ top, int fold, const fr_mem_t* __restrict__ size_inv) {
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= ((size_t)1 << (a + s))) return;
    const uint32_t k = (uint32_t)(idx >> s), inner = (uint32_t)(idx & (((size_t)1 << s) - 1));
    fr_t t = ntt_pow_compose(lo, hi, top, ntt_tw_index((inner * k) << tw_shift));
    if (fold) {
        t = t * fr_t::from_table(FrP::R2);  // Montgomery form of (2^261 mod r): the stored word becomes t * 2^522
        if (fold == 2) t = t * fr_t::load(size_inv);
    }
    t.store(&out[idx]);
}
static inline void ntt_tw_release_entries(ntt_tw_cache_t& cache, std::vector<void*>& leases) {
    std::lock_guard<std::mutex> lk(cache.mu);
    for (void* e : leases) ((ntt_tw_entry*)e)->users--;
    leases.clear();
}
// prelast_lg != 0: this is the pass before the last one of a 2^prelast_lg transform -> the folded variant
static inline const fr_mem_t* ntt_get_full_tw(const ntt_ctx_t& cx, int a, int s, int tw_shift, int dir, int prelast_lg = 0, bool* folded = nullptr) {
    if (folded) *folded = false;
    const int enabled = tuning().ntt_full_tw;
    if (!enabled || !cx.cache || a + s > NTT_LG_MAX || a > NTT_MAX_RADIX_LG) return nullptr;
    const int fold_enabled = tuning().ntt_fold;
    static const size_t cap = (getenv("SNARKVM_HIP_NTT_TW_MB") ? (size_t)atoll(getenv("SNARKVM_HIP_NTT_TW_MB")) : 1536) << 20;
    if (prelast_lg && !fold_enabled) prelast_lg = 0;
    ntt_tw_cache_t& cache = *cx.cache;
    std::lock_guard<std::mutex> lk(cache.mu);
    ntt_tw_entry& slot = prelast_lg ? cache.prelast[dir][prelast_lg] : cache.ptr[dir][a][a + s];
    if (!slot.p) {
        const size_t n = (size_t)1 << (a + s);
        const size_t need = n * sizeof(fr_mem_t);
        if (need > cap) return nullptr;
        while (cache.bytes + need > cap) {  // evict the least recently used table nobody holds
            ntt_tw_entry* lru = nullptr;
            cache.for_each([&](ntt_tw_entry& e) {
                if (e.p && e.users == 0 && (!lru || e.last_use < lru->last_use)) lru = &e;
            });
            if (!lru) return nullptr;  // everything is in use: compose on the fly
            (void)hipFree(lru->p);
            cache.bytes -= lru->bytes;
            *lru = ntt_tw_entry();
        }
        if (hipMalloc((void**)&slot.p, need) != hipSuccess) {
            (void)hipGetLastError();
            slot.p = nullptr;
            return nullptr;  // out of memory: compose on the fly
        }
        slot.bytes = need;
        cache.bytes += need;
        const int fold = !prelast_lg ? 0 : (dir == NTT_INVERSE ? 2 : 1);
        hipLaunchKernelGGL(ntt_fill_full_tw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cx.st, slot.p, a, s, tw_shift, cx.tb->pow_lo[dir],
                           cx.tb->pow_hi[dir], cx.tb->pow_top[dir], fold, (const fr_mem_t*)(cx.tb->size_inv + (prelast_lg ? prelast_lg : 0)));
        (void)hipStreamSynchronize(cx.st);  // other streams may use the table from now on
    }
    slot.last_use = ++cache.tick;
    slot.users++;
    if (cx.leases) cx.leases->push_back(&slot);
    if (folded) *folded = prelast_lg != 0;
    return slot.p;
}

struct ntt_launch_dims_t {
    unsigned ntiles;
    int threads;
    size_t shmem;
};
static inline ntt_launch_dims_t ntt_launch_dims(const ntt_pass_t& p) {
    const size_t E = (size_t)1 << (p.a + p.lgT);
    ntt_launch_dims_t d;
    d.ntiles = (unsigned)(((size_t)1 << p.lg_n) / E);
    d.threads = (int)(E / 4);  // one radix-4 group per thread
    if (d.threads < 64) d.threads = 64;
    if (d.threads > 512) d.threads = 512;
    d.shmem = (9 * E + 9 * ((size_t)1 << (p.a ? p.a - 1 : 0))) * sizeof(uint32_t);  // a [2^8 x 8] tile + its twiddles: 78 KB, two workgroups per CU
    return d;
}
static inline void ntt_launch_pass(hipStream_t st, const ntt_pass_t& p, const ntt_tables_t& tb, const ntt_batch_t* bt = nullptr, unsigned nvec = 1) {
    const ntt_launch_dims_t d = ntt_launch_dims(p);
    if (bt)
        hipLaunchKernelGGL((ntt_pass_kernel_v2<true, ntt_arith_u>), dim3(d.ntiles, nvec), dim3(d.threads), d.shmem, st, p, tb, *bt);
    else
        hipLaunchKernelGGL((ntt_pass_kernel_v2<false, ntt_arith_u>), dim3(d.ntiles), dim3(d.threads), d.shmem, st, p, tb, ntt_no_batch_t{});
}
// the first pass of nvec forward transforms of coefficient operands (bounded load); the first pass of an inverse transform of a product
static inline void ntt_launch_pass_bounded(hipStream_t st, const ntt_pass_t& p, const ntt_tables_t& tb, const ntt_bounded_t& bt, unsigned nvec) {
    const ntt_launch_dims_t d = ntt_launch_dims(p);
    hipLaunchKernelGGL((ntt_pass_kernel_v2<true, ntt_arith_u, ntt_load_bounded>), dim3(d.ntiles, nvec), dim3(d.threads), d.shmem, st, p, tb, bt);
}
static inline void ntt_launch_pass_product(hipStream_t st, const ntt_pass_t& p, const ntt_tables_t& tb, const ntt_product_t& pa) {
    const ntt_launch_dims_t d = ntt_launch_dims(p);
    hipLaunchKernelGGL((ntt_pass_kernel_v2<false, ntt_arith_u, ntt_load_product>), dim3(d.ntiles), dim3(d.threads), d.shmem, st, p, tb, pa);
}

// pass k of plan `pl` as the drivers launch it: geometry, direction / type fields, tile width for `nvec` vectors per launch, and the
// closing-twiddle table.  `folded` carries "the pass before the last one folded 2^261 [/ n] into its table" from pass to pass.
static inline ntt_pass_t ntt_pass_setup(const ntt_ctx_t& cx, const ntt_plan_t& pl, int lg, int k, int dir, int type, unsigned nvec, bool& folded) {
    ntt_pass_t p = ntt_pass_geometry(pl, lg, k);
    p.dir = dir;
    p.coset_pre = (k == 0 && dir == NTT_FORWARD && type == NTT_COSET) ? 1 : 0;
    p.scale_post = (p.last && dir == NTT_INVERSE) ? (type == NTT_COSET ? 2 : 1) : 0;
    p.tw_full = nullptr;
    p.reduce_only = 0;
    if (!p.last) {
        p.lgT = ntt_tile_lg(p.a, p.s, lg, nvec);
        const bool prelast = (k == pl.npass - 2);
        bool f = false;
        p.tw_full = ntt_get_full_tw(cx, p.a, p.s, p.tw_shift, dir, prelast ? lg : 0, &f);
        folded = f;
    } else {
        p.reduce_only = folded ? 1 : 0;
        p.lgT = ntt_tile_lg(p.a, p.a1, lg, nvec);
    }
    return p;
}

// NN-order transform of 2^lg elements held in `data`; `scratch` is a second buffer of the same size.
// The result is left in `data`.
// `vecs` != nullptr: the same transform of `nvec` (<= NTT_BATCH_MAX) distinct vectors in one launch per pass (needs >= 2 passes, i.e.
// lg > 8; `scratch` then holds nvec * 2^lg elements); `data` is ignored.
static inline void ntt_run_nn(const ntt_ctx_t& cx, fr_mem_t* data, fr_mem_t* scratch, int lg, int dir, int type, fr_mem_t* const* vecs = nullptr,
                              unsigned nvec = 1) {
    hipStream_t st = cx.st;
    const ntt_tables_t& tb = *cx.tb;
    if (lg == 0) {
        // size-1 transform: identity (coset shift g^0 = 1, n^-1 = 1)
        return;
    }
    const ntt_plan_t pl = ntt_make_plan(lg);
    ntt_batch_t bt;
    if (vecs) {
        for (unsigned i = 0; i < nvec; i++) bt.v[i] = vecs[i];
        bt.scratch = scratch;
    }
    bool folded = false;  // the pass before the last one used a table with 2^261 [/ n] folded in
    for (int k = 0; k < pl.npass; k++) {
        ntt_pass_t p = ntt_pass_setup(cx, pl, lg, k, dir, type, nvec, folded);
        if (pl.npass == 1) {
            p.in = data;
            p.out = scratch;
        } else if (k == 0) {
            p.in = data;
            p.out = scratch;
        } else if (!p.last) {
            p.in = scratch;
            p.out = scratch;
        } else {
            p.in = scratch;
            p.out = data;
        }
        if (vecs) {
            bt.in_scratch = (p.in == scratch);
            bt.out_scratch = (p.out == scratch);
            ntt_launch_pass(st, p, tb, &bt, nvec);
        } else {
            ntt_launch_pass(st, p, tb);
        }
    }
    if (pl.npass == 1)
        (void)hipMemcpyAsync(data, scratch, sizeof(fr_mem_t) << lg, hipMemcpyDeviceToDevice, st);
}

// ---- the transforms of a device-resident product (snarkvm_hip_polymul_device), 1 <= lg ------------------------------------------
// Forward NN transforms of nvec (<= NTT_BATCH_MAX) coefficient-form operands src[y] of len[y] <= 2^lg elements, read in place and never
// written, into dst[y].  `scratch` holds nvec * 2^lg elements.  The first pass (bounded load) and the middle passes are one launch
// for all operands; the last pass is out of place and runs per operand, in list order, so dst[y] may be scratch slot y' < y: the
// slot has been consumed by then.  That ring keeps the workspace of nvec transforms at nvec + 1 vectors.
static inline void ntt_forward_bounded(const ntt_ctx_t& cx, const fr_mem_t* const* src, const size_t* len, fr_mem_t* const* dst, unsigned nvec,
                                       fr_mem_t* scratch, int lg) {
    const ntt_tables_t& tb = *cx.tb;
    const ntt_plan_t pl = ntt_make_plan(lg);
    ntt_bounded_t bt{};
    bt.scratch = scratch;
    for (unsigned y = 0; y < nvec; y++) bt.src[y] = src[y], bt.len[y] = len[y];
    bool folded = false;
    for (int k = 0; k < pl.npass; k++) {
        const bool per_vector = (k == pl.npass - 1);
        ntt_pass_t p = ntt_pass_setup(cx, pl, lg, k, NTT_FORWARD, NTT_STANDARD, per_vector ? 1 : nvec, folded);
        if (pl.npass == 1) {  // operand -> destination, one launch each (the two are never the same memory)
            for (unsigned y = 0; y < nvec; y++) {
                ntt_bounded_t one{};
                one.v[0] = dst[y];
                one.src[0] = src[y];
                one.len[0] = len[y];
                ntt_launch_pass_bounded(cx.st, p, tb, one, 1);
            }
        } else if (k == 0) {
            bt.in_scratch = 0, bt.out_scratch = 1;
            ntt_launch_pass_bounded(cx.st, p, tb, bt, nvec);
        } else if (!p.last) {
            bt.in_scratch = 1, bt.out_scratch = 1;
            ntt_launch_pass(cx.st, p, tb, &bt, nvec);
        } else {
            for (unsigned y = 0; y < nvec; y++) {
                p.in = scratch + ((size_t)y << lg);
                p.out = dst[y];
                ntt_launch_pass(cx.st, p, tb);
            }
        }
    }
}
// out = the inverse NN transform of the pointwise product of pa.m evaluation vectors, none of which is written.  `work` holds 2^lg
// elements and is none of the factors; `out` may be one of them: every pass but the last reads the factors or `work` and writes
// `work`, and a single-pass transform goes through `work` as well.
static inline void ntt_inverse_product(const ntt_ctx_t& cx, const ntt_product_t& pa, fr_mem_t* work, fr_mem_t* out, int lg) {
    const ntt_plan_t pl = ntt_make_plan(lg);
    bool folded = false;
    for (int k = 0; k < pl.npass; k++) {
        ntt_pass_t p = ntt_pass_setup(cx, pl, lg, k, NTT_INVERSE, NTT_STANDARD, 1, folded);
        p.in = work;
        p.out = (p.last && pl.npass > 1) ? out : work;
        if (k == 0)
            ntt_launch_pass_product(cx.st, p, *cx.tb, pa);
        else
            ntt_launch_pass(cx.st, p, *cx.tb);
    }
    if (pl.npass == 1) (void)hipMemcpyAsync(out, work, sizeof(fr_mem_t) << lg, hipMemcpyDeviceToDevice, cx.st);
}

// Full FFI semantics (any order): bit-reversed inputs/outputs are handled with an explicit permutation pass.
static inline void ntt_run(const ntt_ctx_t& cx, fr_mem_t* data, fr_mem_t* scratch, int lg, int order, int dir, int type) {
    hipStream_t st = cx.st;
    const size_t n = (size_t)1 << lg;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (order == NTT_RN || order == NTT_RR) {
        hipLaunchKernelGGL(ntt_bitrev_kernel, dim3(blocks), dim3(256), 0, st, data, scratch, lg);
        (void)hipMemcpyAsync(data, scratch, sizeof(fr_mem_t) * n, hipMemcpyDeviceToDevice, st);
    }
    ntt_run_nn(cx, data, scratch, lg, dir, type);
    if (order == NTT_NR || order == NTT_RR) {
        hipLaunchKernelGGL(ntt_bitrev_kernel, dim3(blocks), dim3(256), 0, st, data, scratch, lg);
        (void)hipMemcpyAsync(data, scratch, sizeof(fr_mem_t) * n, hipMemcpyDeviceToDevice, st);
    }
}

}  // namespace sv
