// api_msmtest.hip - test hook for the scalar-read phase of the variable-base MSM (snarkvm_hip_devtest_msm_digits): the stand-alone digit kernels
// launched on their own, the digit matrix copied back.  The plan and the digit parameters are built the way msm_run.hip.h::msm_layout builds
// them, the launch shapes are those of msm_stage_digits, the instance table of the fused form is laid out like msm_enqueue_job's.  A translation
// unit of its own (as api_fieldtest.hip): the units that own the MSM entry points compile exactly as before.  The wide-window fused read
// (radix_hist1_wide_kernel, radix_scatter1_fused_kernel) leaves no digits in memory and has no hook; it is tested through whole MSMs.
#include "msm_batch.hip.h"

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

extern "C" {

RustError snarkvm_hip_devtest_msm_digits(const void* scalars, size_t n, int window_bits, int tables, int table_bits, int montgomery, int multi,
                                         void* digits, size_t digits_bytes, uint32_t* info) {
    API_BEGIN
    if (!scalars || !digits || !info || n == 0 || n >= ((size_t)1 << 24))
        throw hip_failure{hipErrorInvalidValue, "devtest_msm_digits: null argument, or n outside 1 .. 2^24 - 1", __LINE__};
    if (window_bits < 0 || window_bits > MSM_C_MAX) throw hip_failure{hipErrorInvalidValue, "devtest_msm_digits: window_bits outside 0 .. 23", __LINE__};
    // table_bits as a handle stores it: 256 / tables for the legacy tables, which check_tables knows by table_bits = 0
    const bool legacy = (tables == 1 || tables == 2 || tables == 4 || tables == 8 || tables == 16) && table_bits == 256 / tables;
    check_tables(tables, legacy ? 0 : table_bits, "devtest_msm_digits");
    const size_t n1 = multi ? n - n / 2 : 0, cols = multi ? msm_padded(n) + msm_padded(n1) : n;
    // msm_layout: a fused batch asks the planner for table_bits-wide windows
    const msm_plan_t pl = msm_make_plan(cols, multi ? table_bits : window_bits, tables, table_bits);
    const bool wide = pl.c > 16;
    if (pl.c < 2 || pl.c > MSM_C_MAX || pl.c * pl.Wd > MSM_BIAS_BITS) throw hip_failure{hipErrorInvalidValue, "devtest_msm_digits: the plan does not fit the 11-word recoding buffer", __LINE__};
    if (multi && (wide || pl.W != 1 || pl.c < 12)) throw hip_failure{hipErrorInvalidValue, "devtest_msm_digits: geometry not eligible for a fused multi-instance run", __LINE__};
    const size_t elem = wide ? sizeof(uint32_t) : sizeof(uint16_t), bytes = (size_t)pl.Wd * cols * elem;
    info[0] = (uint32_t)pl.c, info[1] = (uint32_t)pl.Wd, info[2] = (uint32_t)elem, info[3] = (uint32_t)cols;
    info[4] = multi ? (uint32_t)msm_padded(n) : 0u, info[5] = (uint32_t)n1;
    if (digits_bytes != bytes) throw hip_failure{hipErrorInvalidValue, "devtest_msm_digits: digits_bytes is not digit rows * columns * bytes per digit", __LINE__};
    msm_digit_params_t dp;
    memcpy(dp.bias, pl.bias, sizeof dp.bias);
    dp.c = pl.c;
    dp.W = pl.Wd;
    dp.n = cols;
    dp.montgomery = montgomery ? 1 : 0;
    hipStream_t st = c.stream;
    c.scalars.ensure(n * 32);
    c.digits.ensure(bytes);
    HIP_TRY(hipMemcpyAsync(c.scalars.p, scalars, n * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c.digits.p, 0xff, bytes, st));  // a digit the kernel does not write comes back as all ones, never as a plausible value
    size_t blocks = (cols + 255) / 256;
    msm_inst_t tab[3];
    if (multi) {
        const uint4* d_sc = c.scalars.as<uint4>();
        tab[0] = msm_inst_t{d_sc, (uint32_t)n, (uint32_t)n, 0, 0, 0, (uint32_t)(msm_padded(n) / SORT_TILE)};
        tab[1] = msm_inst_t{d_sc + 2 * (n / 2), (uint32_t)n1, (uint32_t)n1, 0, 0, (uint32_t)msm_padded(n), (uint32_t)(msm_padded(n1) / SORT_TILE)};
        tab[2] = msm_inst_t{nullptr, 0, 0, 0, 0, (uint32_t)cols, 0};  // sentinel
        c.poly[4].ensure(sizeof tab);
        HIP_TRY(hipMemcpyAsync(c.poly[4].p, tab, sizeof tab, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(msm_digits_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const msm_inst_t*)c.poly[4].as<msm_inst_t>(), 2u, c.digits.as<uint16_t>(), dp);
    } else {
        if (blocks > 256 * 16) blocks = 256 * 16;
        if (wide)
            hipLaunchKernelGGL((msm_digits_kernel<uint32_t>), dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)c.scalars.as<uint4>(), c.digits.as<uint32_t>(), dp);
        else
            hipLaunchKernelGGL((msm_digits_kernel<uint16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (const uint4*)c.scalars.as<uint4>(), c.digits.as<uint16_t>(), dp);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(digits, c.digits.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    API_END
}

}  // extern "C"
