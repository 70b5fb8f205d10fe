// api_fieldtest.hip - test hook for the field arithmetic that field_op's two operands cannot express (snarkvm_hip_selftest_field_ext /
// snarkvm_hip_devtest_field_ext): four-operand diff_of_products, Fq2, the square roots of serde.hip.h.  A translation unit of its own, so that
// these extra callers of fq_sqrt / fq2_sqrt leave the inlining decisions inside the decoder kernels of api_serde.hip as they were.
// runtime.hip.h brings the lanes and the API_BEGIN / API_END frame, serde.hip.h the square roots.
#include "runtime.hip.h"
#include "serde.hip.h"

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

// One case per record, operands and results in memory form, converted like field_op does; the same routine on the host and in the kernel.
enum { FX_FQ_DOP = 0, FX_FR_DOP, FX_FQ2_MUL, FX_FQ2_SQR, FX_FQ2_INV, FX_FQ2_DOP, FX_FQ_SQRT, FX_FQ2_SQRT, FX_FQ_RAW, FX_FR_RAW, FX_OPS };
static constexpr uint32_t FX_IN_WORDS[FX_OPS] = {48, 32, 48, 24, 24, 96, 12, 24, 24, 16};
static constexpr uint32_t FX_OUT_WORDS[FX_OPS] = {12, 8, 24, 24, 24, 24, 16, 28, 72, 48};
template <int OP>
__host__ __device__ inline void field_ext_op(const uint32_t* in, uint32_t* out) {
    if constexpr (OP == FX_FQ_DOP || OP == FX_FR_DOP) {
        typedef typename std::conditional<OP == FX_FQ_DOP, fq_t, fr_t>::type F;
        F x[4];
        for (int k = 0; k < 4; k++) x[k] = F::from_raw_words(in + F::WORDS * k);
        F::diff_of_products(x[0], x[1], x[2], x[3]).to_raw_words(out);
    } else if constexpr (OP == FX_FQ_RAW || OP == FX_FR_RAW) {
        // the internal limbs as the operation leaves them, packed without to_mem_mont (a multiplication, which would reduce a result that is
        // not canonical): a + b, a - b, -a, 2a, a * b, 0 * 0 - a * b
        typedef typename std::conditional<OP == FX_FQ_RAW, fq_t, fr_t>::type F;
        const F a = F::from_raw_words(in), b = F::from_raw_words(in + F::WORDS);
        (a + b).pack(out);
        (a - b).pack(out + F::WORDS);
        a.neg().pack(out + 2 * F::WORDS);
        a.dbl().pack(out + 3 * F::WORDS);
        (a * b).pack(out + 4 * F::WORDS);
        F::diff_of_products(F::zero(), F::zero(), a, b).pack(out + 5 * F::WORDS);
    } else if constexpr (OP == FX_FQ_SQRT) {
        fq_t root = fq_t::zero();
        const bool ok = fq_sqrt(fq_t::from_raw_words(in), root);
        (ok ? root : fq_t::zero()).to_raw_words(out);
        out[12] = ok ? 1u : 0u, out[13] = out[14] = out[15] = 0;
    } else if constexpr (OP == FX_FQ2_SQRT) {
        fq2_t root = fq2_t::zero();
        const bool ok = fq2_sqrt(fq2_t::from_raw_words(in), root);
        (ok ? root : fq2_t::zero()).to_raw_words(out);
        out[24] = ok ? 1u : 0u, out[25] = out[26] = out[27] = 0;
    } else {
        const fq2_t a = fq2_t::from_raw_words(in);
        fq2_t r;
        if constexpr (OP == FX_FQ2_MUL) r = a * fq2_t::from_raw_words(in + 24);
        if constexpr (OP == FX_FQ2_SQR) r = a.sqr();
        if constexpr (OP == FX_FQ2_INV) r = a.inverse();
        if constexpr (OP == FX_FQ2_DOP) r = fq2_t::diff_of_products(a, fq2_t::from_raw_words(in + 24), fq2_t::from_raw_words(in + 48), fq2_t::from_raw_words(in + 72));
        r.to_raw_words(out);
    }
}
template <int OP>
static __global__ void devtest_field_ext_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    field_ext_op<OP>(in + (size_t)FX_IN_WORDS[OP] * i, out + (size_t)FX_OUT_WORDS[OP] * i);
}
template <int OP>
static void field_ext_host(const uint32_t* in, uint32_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) field_ext_op<OP>(in + (size_t)FX_IN_WORDS[OP] * i, out + (size_t)FX_OUT_WORDS[OP] * i);
}
template <int OP>
static void field_ext_launch(lane_t& c, const uint32_t* in, uint32_t* out, size_t n) {
    hipLaunchKernelGGL(devtest_field_ext_kernel<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, in, out, n);
}
#define FX_DISPATCH(fn, ...)                                   \
    switch (op) {                                              \
        case FX_FQ_DOP: fn<FX_FQ_DOP>(__VA_ARGS__); break;     \
        case FX_FR_DOP: fn<FX_FR_DOP>(__VA_ARGS__); break;     \
        case FX_FQ2_MUL: fn<FX_FQ2_MUL>(__VA_ARGS__); break;   \
        case FX_FQ2_SQR: fn<FX_FQ2_SQR>(__VA_ARGS__); break;   \
        case FX_FQ2_INV: fn<FX_FQ2_INV>(__VA_ARGS__); break;   \
        case FX_FQ2_DOP: fn<FX_FQ2_DOP>(__VA_ARGS__); break;   \
        case FX_FQ_SQRT: fn<FX_FQ_SQRT>(__VA_ARGS__); break;   \
        case FX_FQ2_SQRT: fn<FX_FQ2_SQRT>(__VA_ARGS__); break; \
        case FX_FQ_RAW: fn<FX_FQ_RAW>(__VA_ARGS__); break;     \
        default: fn<FX_FR_RAW>(__VA_ARGS__); break;            \
    }

extern "C" {

int snarkvm_hip_selftest_field_ext(int op, const void* in, void* out, size_t n) {
    if (op < 0 || op >= FX_OPS || (n && (!in || !out))) return 1;
    FX_DISPATCH(field_ext_host, (const uint32_t*)in, (uint32_t*)out, n)
    return 0;
}
RustError snarkvm_hip_devtest_field_ext(int op, const void* in, void* out, size_t n) {
    API_BEGIN
    if (op < 0 || op >= FX_OPS) throw hip_failure{hipErrorInvalidValue, "devtest_field_ext: op must be 0..9", __LINE__};
    if (n) {
        if (!in || !out) throw hip_failure{hipErrorInvalidValue, "devtest_field_ext: null argument", __LINE__};
        const size_t in_bytes = n * FX_IN_WORDS[op] * 4, out_bytes = n * FX_OUT_WORDS[op] * 4;
        c.poly[0].ensure(in_bytes);
        c.poly[1].ensure(out_bytes);
        HIP_TRY(hipMemcpyAsync(c.poly[0].p, in, in_bytes, hipMemcpyHostToDevice, c.stream));
        FX_DISPATCH(field_ext_launch, c, c.poly[0].as<uint32_t>(), c.poly[1].as<uint32_t>(), n)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, c.poly[1].p, out_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}

}  // extern "C"
