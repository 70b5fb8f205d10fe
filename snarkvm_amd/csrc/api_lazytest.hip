// api_lazytest.hip - test hook for the lazily reduced signed-limb arithmetic of the bucket-accumulation loops (snarkvm_hip_selftest_lazy_ext /
// snarkvm_hip_devtest_lazy_ext): the field routines of ffl.hip.h, fqz_t's operators, xyzz_lazy_t::madd, and the lane-pair Fq2 product and mixed
// addition of ffl2p.hip.h with the helpers of ffl2.hip.h.  Operands and results are RAW limbs (13 int32 words per value, flags as words): nothing on
// the way in or out normalises or reduces, so a limb outside its range or a representative outside its promised interval shows.
// A translation unit of its own: these extra callers of madd / mul_core leave the inlining decisions inside the accumulate kernels as they were.
#include "runtime.hip.h"
#include "ffl2p.hip.h"

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

// One case per record, in 32-bit words; the same routine on the host and in the kernel.  The single-lane ops run one thread per case; the pair ops
// one DPP lane pair per case (even lane: the c0 component, odd lane: c1) through fq2p::xp_dev, and both lanes through fq2p::xp_host on the host.
enum { LX_MUL = 0, LX_SQR, LX_DOP, LX_NORM, LX_TO_EXACT, LX_FROM_EXACT, LX_RAW, LX_FQZ, LX_MADD, LX_PAIR_HELP, LX_PAIR_MUL, LX_PAIR_MADD, LX_OPS };
static constexpr uint32_t LX_IN_WORDS[LX_OPS] = {26, 13, 52, 13, 13, 13, 13, 39, 80, 65, 52, 158};
static constexpr uint32_t LX_OUT_WORDS[LX_OPS] = {13, 13, 13, 13, 13, 13, 25, 53, 54, 66, 106, 105};
static constexpr bool lx_is_pair(int op) { return op >= LX_PAIR_MUL; }

SV_HD fql_t lx_load(const int32_t* p) {
    fql_t r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.v[i] = p[i];
    return r;
}
SV_HD void lx_store(int32_t* p, const fql_t& a) {
#pragma unroll
    for (int i = 0; i < 13; i++) p[i] = a.v[i];
}

template <int OP>
__host__ __device__ inline void lazy_ext_op(const int32_t* in, int32_t* out) {
    if constexpr (OP == LX_MUL) {
        lx_store(out, fql_t::mul(lx_load(in), lx_load(in + 13)));
    } else if constexpr (OP == LX_SQR) {
        lx_store(out, fql_t::sqr(lx_load(in)));
    } else if constexpr (OP == LX_DOP) {
        lx_store(out, fql_t::diff_of_products(lx_load(in), lx_load(in + 13), lx_load(in + 26), lx_load(in + 39)));
    } else if constexpr (OP == LX_NORM) {
        lx_store(out, lx_load(in).normalized());
    } else if constexpr (OP == LX_TO_EXACT) {
        const fq_t e = lx_load(in).to_exact();
        for (int i = 0; i < 13; i++) out[i] = (int32_t)e.v[i];
    } else if constexpr (OP == LX_FROM_EXACT) {
        fq_t a;
        for (int i = 0; i < 13; i++) a.v[i] = (uint32_t)in[i];
        lx_store(out, fql_t::from_exact(a));
    } else if constexpr (OP == LX_RAW) {
        alignas(16) uint32_t raw[12];
        lx_load(in).store_raw(raw);
        for (int i = 0; i < 12; i++) out[i] = (int32_t)raw[i];
        lx_store(out + 12, fql_t::load_raw(raw));
    } else if constexpr (OP == LX_FQZ) {
        const fqz_t a{lx_load(in)}, b{lx_load(in + 13)};
        lx_store(out, (a + b).a);
        lx_store(out + 13, (a - b).a);
        lx_store(out + 26, a.dbl().a);
        lx_store(out + 39, a.neg().a);
        out[52] = fqz_t{lx_load(in + 26)}.is_zero() ? 1 : 0;
    } else if constexpr (OP == LX_MADD) {
        xyzz_lazy_t acc;
        acc.x = lx_load(in), acc.y = lx_load(in + 13), acc.zz = lx_load(in + 26), acc.zzz = lx_load(in + 39);
        acc.inf = in[52] != 0;
        const bool ok = acc.madd(lx_load(in + 53), lx_load(in + 66), in[79] != 0);
        out[0] = ok ? 1 : 0;
        lx_store(out + 1, acc.x), lx_store(out + 14, acc.y), lx_store(out + 27, acc.zz), lx_store(out + 40, acc.zzz);
        out[53] = acc.inf ? 1 : 0;
    } else {  // LX_PAIR_HELP: the per-lane helpers with the arguments the pair addition gives them
        const fql_t a = lx_load(in), p = fq2l::sub_norm(a, lx_load(in + 13), 1);
        lx_store(out, p);
        lx_store(out + 13, fq2l::sub_norm(a, lx_load(in + 26), -1));
        lx_store(out + 26, fq2p::norm_k(in + 39));
        lx_store(out + 39, fq2l::cond_neg_canonical(lx_load(in + 52), true));
        lx_store(out + 52, fq2l::cond_neg_canonical(lx_load(in + 52), false));
        out[65] = fq2p::is_zero_mod_q(p) ? 1 : 0;
    }
}
// The pair ops: lane l of the instance holds component c = XP::odd(l) of every value.
template <int OP, class XP>
__host__ __device__ inline void lazy_pair_op(const int32_t* in, int32_t* out) {
    constexpr int NL = XP::NL;
    if constexpr (OP == LX_PAIR_MUL) {
        fql_t a[NL], b[NL], r[NL];
        for (int l = 0; l < NL; l++) {
            const int c = XP::odd(l) ? 1 : 0;
            a[l] = lx_load(in + 13 * c), b[l] = lx_load(in + 26 + 13 * c);
        }
        fq2p::opa_t A[NL];
        fq2p::opb_t B[NL];
        fq2p::pair_ops<XP>::prep_a(a, A);
        fq2p::pair_ops<XP>::prep_b(b, B);
        fq2p::pair_ops<XP>::mul(A, B, r);
        for (int l = 0; l < NL; l++) {  // the product, then what the exchange left in this lane's prepared operands
            int32_t* o = out + 53 * (XP::odd(l) ? 1 : 0);
            lx_store(o, r[l]);
            for (int i = 0; i < 13; i++) o[13 + i] = A[l].X[i], o[26 + i] = A[l].Y[i];
            for (int i = 0; i < 14; i++) o[39 + i] = B[l].recv[i];
        }
    } else {
        fq2p::xyzz_pair_t<XP> acc;
        fql_t px[NL], py[NL];
        for (int l = 0; l < NL; l++) {
            const int c = XP::odd(l) ? 1 : 0;
            acc.x[l] = lx_load(in + 13 * c), acc.y[l] = lx_load(in + 26 + 13 * c), acc.zz[l] = lx_load(in + 52 + 13 * c), acc.zzz[l] = lx_load(in + 78 + 13 * c);
            px[l] = lx_load(in + 105 + 13 * c), py[l] = lx_load(in + 131 + 13 * c);
        }
        acc.inf = in[104] != 0;
        acc.madd(px, py, in[157] != 0);
        for (int l = 0; l < NL; l++) {
            const int c = XP::odd(l) ? 1 : 0;
            lx_store(out + 13 * c, acc.x[l]), lx_store(out + 26 + 13 * c, acc.y[l]), lx_store(out + 52 + 13 * c, acc.zz[l]), lx_store(out + 78 + 13 * c, acc.zzz[l]);
            if (!c) out[104] = acc.inf ? 1 : 0;
        }
    }
}
template <int OP>
static __global__ void __launch_bounds__(64) devtest_lazy_ext_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, size_t n) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if constexpr (lx_is_pair(OP)) {
        const size_t i = t >> 1;  // both lanes of a pair leave together
        if (i >= n) return;
        lazy_pair_op<OP, fq2p::xp_dev>(in + (size_t)LX_IN_WORDS[OP] * i, out + (size_t)LX_OUT_WORDS[OP] * i);
    } else {
        if (t >= n) return;
        lazy_ext_op<OP>(in + (size_t)LX_IN_WORDS[OP] * t, out + (size_t)LX_OUT_WORDS[OP] * t);
    }
}
template <int OP>
static void lazy_ext_host(const int32_t* in, int32_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if constexpr (lx_is_pair(OP))
            lazy_pair_op<OP, fq2p::xp_host>(in + (size_t)LX_IN_WORDS[OP] * i, out + (size_t)LX_OUT_WORDS[OP] * i);
        else
            lazy_ext_op<OP>(in + (size_t)LX_IN_WORDS[OP] * i, out + (size_t)LX_OUT_WORDS[OP] * i);
    }
}
template <int OP>
static void lazy_ext_launch(lane_t& c, const int32_t* in, int32_t* out, size_t n) {
    const size_t threads = lx_is_pair(OP) ? 2 * n : n;
    hipLaunchKernelGGL(devtest_lazy_ext_kernel<OP>, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, c.stream, in, out, n);
}
#define LX_DISPATCH(fn, ...)                                         \
    switch (op) {                                                    \
        case LX_MUL: fn<LX_MUL>(__VA_ARGS__); break;                 \
        case LX_SQR: fn<LX_SQR>(__VA_ARGS__); break;                 \
        case LX_DOP: fn<LX_DOP>(__VA_ARGS__); break;                 \
        case LX_NORM: fn<LX_NORM>(__VA_ARGS__); break;               \
        case LX_TO_EXACT: fn<LX_TO_EXACT>(__VA_ARGS__); break;       \
        case LX_FROM_EXACT: fn<LX_FROM_EXACT>(__VA_ARGS__); break;   \
        case LX_RAW: fn<LX_RAW>(__VA_ARGS__); break;                 \
        case LX_FQZ: fn<LX_FQZ>(__VA_ARGS__); break;                 \
        case LX_MADD: fn<LX_MADD>(__VA_ARGS__); break;               \
        case LX_PAIR_HELP: fn<LX_PAIR_HELP>(__VA_ARGS__); break;     \
        case LX_PAIR_MUL: fn<LX_PAIR_MUL>(__VA_ARGS__); break;       \
        default: fn<LX_PAIR_MADD>(__VA_ARGS__); break;               \
    }

extern "C" {

int snarkvm_hip_selftest_lazy_ext(int op, const void* in, void* out, size_t n) {
    if (op < 0 || op >= LX_OPS || (n && (!in || !out))) return 1;
    LX_DISPATCH(lazy_ext_host, (const int32_t*)in, (int32_t*)out, n)
    return 0;
}
RustError snarkvm_hip_devtest_lazy_ext(int op, const void* in, void* out, size_t n) {
    API_BEGIN
    if (op < 0 || op >= LX_OPS) throw hip_failure{hipErrorInvalidValue, "devtest_lazy_ext: op must be 0..11", __LINE__};
    if (n) {
        if (!in || !out) throw hip_failure{hipErrorInvalidValue, "devtest_lazy_ext: null argument", __LINE__};
        if (n > ((size_t)1 << 24)) throw hip_failure{hipErrorInvalidValue, "devtest_lazy_ext: at most 2^24 cases", __LINE__};
        const size_t in_bytes = n * LX_IN_WORDS[op] * 4, out_bytes = n * LX_OUT_WORDS[op] * 4;
        c.poly[0].ensure(in_bytes);
        c.poly[1].ensure(out_bytes);
        HIP_TRY(hipMemcpyAsync(c.poly[0].p, in, in_bytes, hipMemcpyHostToDevice, c.stream));
        LX_DISPATCH(lazy_ext_launch, c, c.poly[0].as<int32_t>(), c.poly[1].as<int32_t>(), n)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, c.poly[1].p, out_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}

}  // extern "C"
