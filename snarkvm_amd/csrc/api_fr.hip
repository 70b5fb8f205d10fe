// api_fr.hip - the transforms of the C ABI: NTT / polymul (the reference's snarkvm_ntt, snarkvm_polymul) on host and device operands, the
// pointwise product and the form conversion, the setup-time group operations built on them, and the NTT's host test hooks.  The other Fr
// entry points: api_poly.hip (vector passes, divisions, combinations, reductions) and api_varuna.hip (prover rounds, circuit index).
#include "msm_run.hip.h"  // convert_bases (g1_fixed_base_msm)
#include "group.hip.h"
#include "fr_call.hip.h"

// this unit launches the NTT passes
static void tu_set_kernel_attributes() {
    HIP_TRY(hipFuncSetAttribute((const void*)ntt_pass_kernel_v2<false, ntt_arith_u>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_TRY(hipFuncSetAttribute((const void*)ntt_pass_kernel_v2<true, ntt_arith_u>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_TRY(hipFuncSetAttribute((const void*)ntt_pass_kernel_v2<true, ntt_arith_u, ntt_load_bounded>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIP_TRY(hipFuncSetAttribute((const void*)ntt_pass_kernel_v2<false, ntt_arith_u, ntt_load_product>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
}

extern "C" {

// ---- NTT -------------------------------------------------------------------------------------
static void check_ntt_args(uint32_t lg, int order, int dir, int type) {
    if (lg > (uint32_t)NTT_LG_MAX) throw hip_failure{hipErrorMemoryAllocation, "ntt: lg_domain_size > 28 is not supported by this backend", __LINE__};
    if (order < 0 || order > 3 || dir < 0 || dir > 1 || type < 0 || type > 1) throw hip_failure{hipErrorInvalidValue, "ntt: bad enum value", __LINE__};
}
RustError snarkvm_ntt(void* inout, uint32_t lg, enum NTTInputOutputOrder order, enum NTTDirection dir, enum NTTType type) {
    API_BEGIN
    check_ntt_args(lg, (int)order, (int)dir, (int)type);
    if (!inout) throw hip_failure{hipErrorInvalidValue, "ntt: null buffer", __LINE__};
    const size_t bytes = sizeof(fr_mem_t) << lg;
    c.ntt_data.ensure(bytes);
    c.ntt_scratch.ensure(bytes);
    c.phase_begin("ntt_h2d");
    HIP_TRY(hipMemcpyAsync(c.ntt_data.p, inout, bytes, hipMemcpyHostToDevice, c.stream));
    c.phase_end();
    c.phase_begin("ntt_kernels");
    ntt_run(c.ntt_ctx(), c.ntt_data.as<fr_mem_t>(), c.ntt_scratch.as<fr_mem_t>(), (int)lg, (int)order, (int)dir, (int)type);
    c.phase_end();
    HIP_TRY(hipGetLastError());
    c.phase_begin("ntt_d2h");
    HIP_TRY(hipMemcpyAsync(inout, c.ntt_data.p, bytes, hipMemcpyDeviceToHost, c.stream));
    c.phase_end();
    HIP_TRY(hipStreamSynchronize(c.stream));
    API_END
}
RustError snarkvm_hip_ntt_device(void* d_inout, uint32_t lg, int order, int dir, int type) {
    API_BEGIN_DEV(device_for(d_inout, 1))
    check_ntt_args(lg, order, dir, type);
    c.ntt_scratch.ensure(sizeof(fr_mem_t) << lg);
    c.phase_begin("ntt_kernels");
    ntt_run(c.ntt_ctx(), (fr_mem_t*)d_inout, c.ntt_scratch.as<fr_mem_t>(), (int)lg, order, dir, type);
    c.phase_end();
    HIP_TRY(hipGetLastError());
    c.sync_or_defer();
    API_END
}
// `count` independent in-place transforms of 2^lg elements each over device vectors (the iNTTs of a prover round: second.rs:104-113
// transforms z_a, z_b, z_c at |R|; fourth.rs:174-231 nine vectors at |K|): every transform is enqueued on ONE lane's stream and the
// call synchronises once - a synchronous call per vector pays the ~0.1-0.2 ms of stream-synchronisation latency of this stack
// per transform (2.36 ms around the 2.16 ms of kernels at 2^24, 52 us around ~15 us at 2^16).  The same vector may appear more
// than once (stream order = list order).  directions / types: per vector, or NULL for all forward / all standard.
RustError snarkvm_hip_ntt_device_batch(void* const* d_inouts, size_t count, uint32_t lg, int order, const int* dirs, const int* types) {
    if (count == 0) return ok();
    if (!d_inouts || !d_inouts[0]) return fail((int)hipErrorInvalidValue, "snarkvm_hip: ntt_device_batch: null argument");
    API_BEGIN_DEV(device_for(d_inouts[0], 1))
    for (size_t k = 0; k < count; k++) {
        check_ntt_args(lg, order, dirs ? dirs[k] : 0, types ? types[k] : 0);
        if (!d_inouts[k]) throw hip_failure{hipErrorInvalidValue, "ntt_device_batch: null vector", __LINE__};
        // every vector must live on the lane's GPU: the kernels of this call run there
        const int dk = device_for(d_inouts[k], 1);
        if (g_rt.devs[dk]->physical != c.dev->physical) throw hip_failure{hipErrorInvalidValue, "ntt_device_batch: the vectors live on different devices", __LINE__};
    }
    c.phase_begin("ntt_kernels");
    // Runs of consecutive list entries with the same (direction, type) and no vector twice travel as ONE launch per pass
    // (blockIdx.y = vector; tuning ntt_batch=0: one launch sequence per vector).  List order is preserved between runs, so a
    // vector listed twice is still transformed twice, in order.
    const bool can_batch = tuning().ntt_batch && order == NTT_NN && lg > 8;
    // a run's scratch (run length x 2^lg elements) stays within that of NTT_BATCH_MAX vectors of 2^26: 24 vectors at 2^27, 12 at 2^28
    const size_t run_max = lg <= (uint32_t)NTT_TW_LG ? (size_t)NTT_BATCH_MAX : ((size_t)NTT_BATCH_MAX << NTT_TW_LG) >> lg;
    std::vector<std::pair<size_t, size_t>> runs;
    size_t max_run = 1;
    for (size_t k = 0; k < count;) {
        const int dir = dirs ? dirs[k] : 0, type = types ? types[k] : 0;
        size_t e = k + 1;
        if (can_batch) {
            while (e < count && e - k < run_max && (dirs ? dirs[e] : 0) == dir && (types ? types[e] : 0) == type) {
                bool dup = false;
                for (size_t q = k; q < e && !dup; q++) dup = d_inouts[q] == d_inouts[e];
                if (dup) break;
                e++;
            }
        }
        runs.emplace_back(k, e);
        max_run = e - k > max_run ? e - k : max_run;
        k = e;
    }
    c.ntt_scratch.ensure((sizeof(fr_mem_t) << lg) * max_run);
    for (const auto& r : runs) {
        const size_t k = r.first, nv = r.second - r.first;
        const int dir = dirs ? dirs[k] : 0, type = types ? types[k] : 0;
        if (nv > 1)
            ntt_run_nn(c.ntt_ctx(), nullptr, c.ntt_scratch.as<fr_mem_t>(), (int)lg, dir, type, (fr_mem_t* const*)(d_inouts + k), (unsigned)nv);
        else
            ntt_run(c.ntt_ctx(), (fr_mem_t*)d_inouts[k], c.ntt_scratch.as<fr_mem_t>(), (int)lg, order, dir, type);
    }
    c.phase_end();
    HIP_TRY(hipGetLastError());
    c.sync_or_defer();
    API_END
}

// ---- polymul -----------------------------------------------------------------------------------
// PolyMultiplier::multiply on the device (multiplier.rs:70-134 through snarkvm.cu:188-247 / polynomial.cuh:104-266).  Like the
// reference's `Polynomial::Mul`, the upload of operand k + 1 (on the lane's second stream, into the other of two operand
// buffers) overlaps the transform and the pointwise product of operand k; events order the two streams:
//   ev[b]     "operand buffer b has been uploaded"      (alt -> main)
//   ev[2 + b] "operand buffer b has been consumed"      (main -> alt)
RustError snarkvm_polymul(void* out, size_t pcount, const void* polynomials, const void* plens, size_t ecount, const void* evaluations,
                          const void* elens, uint32_t lg) {
    // corner cases of snarkvm.cu:196-210 first (no device needed for the copy)
    const fr_mem_t* const* polys = (const fr_mem_t* const*)polynomials;
    const fr_mem_t* const* evals = (const fr_mem_t* const*)evaluations;
    const size_t* pl = (const size_t*)plens;
    const size_t* el = (const size_t*)elens;
    if (pcount + ecount == 0) return ok();
    if (pcount + ecount == 1 && pcount == 1) {
        // `out` holds 2^lg elements: a longer polynomial would be copied past its end
        if (lg < 64 && pl[0] > ((size_t)1 << lg)) return fail((int)hipErrorInvalidValue, "snarkvm_hip: polymul: polynomial longer than the domain");
        memcpy(out, polys[0], sizeof(fr_mem_t) * pl[0]);
        return ok();
    }
    API_BEGIN
    check_ntt_args(lg, 0, 0, 0);
    const size_t n = (size_t)1 << lg;
    const size_t bytes = sizeof(fr_mem_t) * n;
    for (size_t k = 0; k < pcount; k++)
        if (pl[k] > n) throw hip_failure{hipErrorInvalidValue, "polymul: polynomial longer than the domain", __LINE__};
    for (size_t k = 0; k < ecount; k++)
        if (el[k] != n) throw hip_failure{hipErrorInvalidValue, "polymul: evaluation vector length != domain size", __LINE__};
    c.ntt_data.ensure(bytes);
    c.ntt_alt.ensure(bytes);
    c.ntt_scratch.ensure(bytes);
    c.ntt_acc.ensure(bytes);
    hipStream_t st = c.stream;
    fr_mem_t* buf[2] = {c.ntt_data.as<fr_mem_t>(), c.ntt_alt.as<fr_mem_t>()};
    fr_mem_t* acc = c.ntt_acc.as<fr_mem_t>();
    fr_mem_t* scratch = c.ntt_scratch.as<fr_mem_t>();
    const ntt_ctx_t cx = c.ntt_ctx();
    if (pcount + ecount == 1) {  // a single evaluation vector: zero-pad + inverse NTT (snarkvm.cu:203-208)
        HIP_TRY(hipMemsetAsync(acc, 0, bytes, st));
        HIP_TRY(hipMemcpyAsync(acc, evals[0], sizeof(fr_mem_t) * el[0], hipMemcpyHostToDevice, st));
        ntt_run(cx, acc, scratch, (int)lg, NTT_NN, NTT_INVERSE, NTT_STANDARD);
        HIP_TRY(hipMemcpyAsync(out, acc, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        const size_t total = pcount + ecount;
        // operand 0 goes straight into the accumulator on the main stream; operands k >= 1 alternate between the two buffers
        auto upload = [&](size_t k, fr_mem_t* dst, hipStream_t s) {
            if (k < pcount) {
                HIP_TRY(hipMemcpyAsync(dst, polys[k], sizeof(fr_mem_t) * pl[k], hipMemcpyHostToDevice, s));
                if (pl[k] < n) HIP_TRY(hipMemsetAsync(dst + pl[k], 0, sizeof(fr_mem_t) * (n - pl[k]), s));
            } else {
                HIP_TRY(hipMemcpyAsync(dst, evals[k - pcount], bytes, hipMemcpyHostToDevice, s));
            }
        };
        upload(0, acc, st);
        if (pcount > 0) ntt_run(cx, acc, scratch, (int)lg, NTT_NN, NTT_FORWARD, NTT_STANDARD);
        for (size_t k = 1; k < total; k++) {
            const int b = (int)(k & 1);
            // the kernels of operand k - 1 are already queued on the main stream: this (host-blocking, pageable) copy runs beside them
            if (k >= 3) HIP_TRY(hipStreamWaitEvent(c.alt, c.ev[2 + b], 0));  // buffer b was last consumed by operand k - 2
            upload(k, buf[b], c.alt);
            HIP_TRY(hipEventRecord(c.ev[b], c.alt));
            HIP_TRY(hipStreamWaitEvent(st, c.ev[b], 0));
            if (k < pcount) ntt_run(cx, buf[b], scratch, (int)lg, NTT_NN, NTT_FORWARD, NTT_STANDARD);
            hipLaunchKernelGGL(fr_pointwise_mul_kernel, dim3(blocks), dim3(256), 0, st, acc, acc, buf[b], n, 1);
            HIP_TRY(hipEventRecord(c.ev[2 + b], st));
        }
        ntt_run(cx, acc, scratch, (int)lg, NTT_NN, NTT_INVERSE, NTT_STANDARD);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, acc, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipStreamSynchronize(c.alt));
    }
    API_END
}

// The same product over operands that live in device memory and stay there (header: snarkvm_hip_polymul_device).  Nothing is staged:
// the forward transforms read the coefficient operands where they are (bounded load: zero beyond plens[k]), the inverse transform's
// first pass reads the product of the evaluation-form factors (product load), and the last pass writes d_out.
//   C (ntt_data, 2^lg) + X (ntt_scratch, r slots of 2^lg): the ring of ntt_forward_bounded for r coefficient operands per chunk;
//   acc (ntt_acc, 2^lg): the product so far, when the operands come in several chunks or leave more than NTT_PROD_MAX factors.
RustError snarkvm_hip_polymul_device(void* d_out, size_t pcount, const void* const* d_polys, const size_t* plens, size_t ecount, const void* const* d_evals,
                                     const size_t* elens, uint32_t lg) {
    if (pcount + ecount == 0) return ok();
    API_BEGIN_DEV(device_for(d_out, 1))
    check_ntt_args(lg, 0, 0, 0);
    if (!d_out || (pcount && (!d_polys || !plens)) || (ecount && (!d_evals || !elens))) throw hip_failure{hipErrorInvalidValue, "polymul_device: null argument", __LINE__};
    const size_t n = (size_t)1 << lg;
    const size_t bytes = sizeof(fr_mem_t) * n;
    bool zero = false;
    for (size_t k = 0; k < pcount + ecount; k++) {
        const bool poly = k < pcount;
        const void* ptr = poly ? d_polys[k] : d_evals[k - pcount];
        const size_t len = poly ? plens[k] : elens[k - pcount];
        if (!ptr) throw hip_failure{hipErrorInvalidValue, "polymul_device: null operand", __LINE__};
        if (poly && len > n) throw hip_failure{hipErrorInvalidValue, "polymul_device: polynomial longer than the domain", __LINE__};
        if (!poly && len != n) throw hip_failure{hipErrorInvalidValue, "polymul_device: evaluation vector length != domain size", __LINE__};
        if (g_rt.devs[device_for(ptr, 1)]->physical != c.dev->physical)
            throw hip_failure{hipErrorInvalidValue, "polymul_device: an operand lives on another device than d_out", __LINE__};
        // d_out may BE an operand (same start): every read of it is queued before the first write of d_out.  Any other overlap is refused.
        if (ptr != d_out && fr_spans_overlap(d_out, n, ptr, len)) throw hip_failure{hipErrorInvalidValue, "polymul_device: d_out overlaps an operand", __LINE__};
        zero = zero || len == 0;
    }
    hipStream_t st = c.stream;
    fr_mem_t* out = (fr_mem_t*)d_out;
    c.phase_begin("polymul_kernels");
    if (zero) {  // a zero polynomial among the factors
        HIP_TRY(hipMemsetAsync(out, 0, bytes, st));
    } else if (pcount == 1 && ecount == 0) {  // a copy (snarkvm.cu:196-202), and the tail the host symbol leaves to its caller
        if (d_polys[0] != d_out) HIP_TRY(hipMemcpyAsync(out, d_polys[0], sizeof(fr_mem_t) * plens[0], hipMemcpyDeviceToDevice, st));
        if (plens[0] < n) HIP_TRY(hipMemsetAsync(out + plens[0], 0, sizeof(fr_mem_t) * (n - plens[0]), st));
    } else {
        // coefficient operands per chunk: one batched launch per pass, within the scratch bound of snarkvm_hip_ntt_device_batch
        const size_t r_max = lg <= (uint32_t)NTT_TW_LG ? (size_t)NTT_BATCH_MAX : ((size_t)NTT_BATCH_MAX << NTT_TW_LG) >> lg;
        const size_t np = lg ? pcount : 0;  // a size-1 transform is the identity: the operands are their own evaluations
        const size_t r = np < r_max ? np : r_max;
        const size_t last_chunk = np ? (np - 1) % r_max + 1 : 0;
        const bool chunked = np > r_max;
        const bool need_acc = chunked || (chunked ? 1 : 0) + last_chunk + (pcount - np) + ecount > (size_t)NTT_PROD_MAX;
        if (np) c.ntt_data.ensure(bytes);
        c.ntt_scratch.ensure(bytes * (r ? r : 1));
        if (need_acc) c.ntt_acc.ensure(bytes);
        fr_mem_t *ring0 = c.ntt_data.as<fr_mem_t>(), *scratch = c.ntt_scratch.as<fr_mem_t>(), *acc = c.ntt_acc.as<fr_mem_t>();
        const ntt_ctx_t cx = c.ntt_ctx();
        const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        std::vector<const fr_mem_t*> fac;  // evaluation-form factors still to be multiplied
        // groups of NTT_PROD_MAX factors -> acc, which takes their place, until at most `keep` factors are left
        auto fold = [&](size_t keep) {
            while (fac.size() > keep) {
                const size_t m = fac.size() < (size_t)NTT_PROD_MAX ? fac.size() : (size_t)NTT_PROD_MAX;
                hipLaunchKernelGGL(fr_product_kernel, dim3(blocks), dim3(256), 0, st, acc, ntt_product_args(fac.data(), (int)m), n);
                fac.erase(fac.begin(), fac.begin() + m);
                fac.insert(fac.begin(), acc);
            }
        };
        fr_mem_t* work = scratch;  // a vector no factor lives in: the slot the last forward transform has left behind
        for (size_t k0 = 0; k0 < np; k0 += r_max) {
            const size_t nv = np - k0 < r_max ? np - k0 : r_max;
            fr_mem_t* dst[NTT_BATCH_MAX];
            for (size_t y = 0; y < nv; y++) dst[y] = y ? scratch + ((y - 1) << lg) : ring0;
            ntt_forward_bounded(cx, (const fr_mem_t* const*)d_polys + k0, plens + k0, dst, (unsigned)nv, scratch, (int)lg);
            fac.insert(fac.end(), dst, dst + nv);
            work = scratch + ((nv - 1) << lg);
            if (k0 + nv < np) fold(1);  // the ring is about to be reused (a chunk that is not the last one holds r_max >= 12 transforms)
        }
        for (size_t k = np; k < pcount; k++) fac.push_back((const fr_mem_t*)d_polys[k]);
        for (size_t k = 0; k < ecount; k++) fac.push_back((const fr_mem_t*)d_evals[k]);
        fold((size_t)NTT_PROD_MAX);
        const ntt_product_t pa = ntt_product_args(fac.data(), (int)fac.size());
        if (lg == 0)
            hipLaunchKernelGGL(fr_product_kernel, dim3(1), dim3(64), 0, st, out, pa, n);
        else
            ntt_inverse_product(cx, pa, work, out, (int)lg);
    }
    c.phase_end();
    HIP_TRY(hipGetLastError());
    c.sync_or_defer();
    API_END
}

// ---- Fr vector helpers ---------------------------------------------------------------------------
RustError snarkvm_hip_fr_mul_device(void* d_out, const void* d_a, const void* d_b, size_t n) {
    API_BEGIN_DEV(device_for(d_out, n ? 1 : 0))
    if (n) {
        const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(fr_pointwise_mul_kernel, dim3(blocks), dim3(256), 0, c.stream, (fr_mem_t*)d_out, (const fr_mem_t*)d_a, (const fr_mem_t*)d_b, n, 1);
        HIP_TRY(hipGetLastError());
        c.sync_or_defer();
    }
    API_END
}
RustError snarkvm_hip_fr_convert_device(void* d_out, const void* d_in, size_t n, int to_bigint) {
    API_BEGIN_DEV(device_for(d_out, n ? 1 : 0))
    if (n) {
        const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
        hipLaunchKernelGGL(fr_to_bigint_kernel, dim3(blocks), dim3(256), 0, c.stream, (fr_mem_t*)d_out, (const fr_mem_t*)d_in, n, to_bigint);
        HIP_TRY(hipGetLastError());
        c.sync_or_defer();
    }
    API_END
}

// ---- setup-time group operations (group.hip.h) -------------------------------------------------------
RustError snarkvm_hip_g1_fixed_base_msm(void* out_projective, const void* g_affine, const void* scalars, size_t n) {
    API_BEGIN
    if (n) {
        if (!out_projective || !g_affine || !scalars) throw hip_failure{hipErrorInvalidValue, "g1_fixed_base_msm: null argument", __LINE__};
        hipStream_t st = c.stream;
        // the base in the engine's native form, through the regular conversion kernel
        c.bases_tmp.ensure(256 + sizeof(g1_aff_mem_t));
        HIP_TRY(hipMemcpyAsync(c.bases_tmp.p, g_affine, 104, hipMemcpyHostToDevice, st));
        g1_aff_mem_t* d_g = (g1_aff_mem_t*)(c.bases_tmp.as<uint8_t>() + 256);
        convert_bases<fq_t>(c, c.bases_tmp.as<uint8_t>(), 104, 1, d_g);
        g1_aff_mem_t g_native;
        HIP_TRY(hipMemcpyAsync(&g_native, d_g, sizeof g_native, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const size_t entries = (size_t)FIXED_OUTER << FIXED_WINDOW;
        c.poly[0].ensure(entries * sizeof(g1_aff_mem_t));
        c.poly[1].ensure(n * 32);
        c.poly[2].ensure(n * 144);
        hipLaunchKernelGGL(g1_fixed_table_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, g_native, c.poly[0].as<g1_aff_mem_t>());
        HIP_TRY(hipMemcpyAsync(c.poly[1].p, scalars, n * 32, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(g1_fixed_msm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c.poly[0].as<g1_aff_mem_t>(),
                           c.poly[1].as<fr_mem_t>(), n, c.poly[2].as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_projective, c.poly[2].p, n * 144, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    API_END
}
RustError snarkvm_hip_g1_group_ntt(void* inout_projective, uint32_t lg, int inverse) {
    API_BEGIN
    if (lg > 24) throw hip_failure{hipErrorInvalidValue, "g1_group_ntt: lg_domain_size > 24", __LINE__};
    if (!inout_projective) throw hip_failure{hipErrorInvalidValue, "g1_group_ntt: null argument", __LINE__};
    const size_t n = (size_t)1 << lg;
    hipStream_t st = c.stream;
    c.poly[0].ensure(n * 144);
    c.poly[1].ensure(n * sizeof(g1_xyzz_mem_t));
    c.poly[2].ensure((n / 2 + 1) * sizeof(fr_mem_t));
    uint32_t* d_jac = c.poly[0].as<uint32_t>();
    g1_xyzz_mem_t* d_pts = c.poly[1].as<g1_xyzz_mem_t>();
    fr_mem_t* d_tw = c.poly[2].as<fr_mem_t>();
    HIP_TRY(hipMemcpyAsync(d_jac, inout_projective, n * 144, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(g1_jac_to_xyzz_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const uint32_t*)d_jac, d_pts, n);
    if (lg > 0) {
        // twiddles root^k (k < n/2) as canonical integers: ones -> distribute_powers -> to_bigint, all on the device
        fr_t omega = fr_domain_generator(lg);
        if (inverse) omega = omega.inverse();
        fr_mem_t one_mem, root_mem;
        fr_t::one().to_mem_mont().store(&one_mem);
        omega.to_mem_mont().store(&root_mem);
        const size_t h = n / 2;
        hipLaunchKernelGGL(fr_fill_kernel, dim3(fr_grid(h)), dim3(256), 0, st, d_tw, h, one_mem);
        fr_distribute_powers_run(c, d_tw, h, root_mem, one_mem);
        hipLaunchKernelGGL(fr_to_bigint_kernel, dim3(fr_grid(h)), dim3(256), 0, st, d_tw, (const fr_mem_t*)d_tw, h, 1);
        // four lanes per butterfly from 32 points on (group.hip.h: every lane of every wave must own a butterfly); tuning group_quad=0: one lane per butterfly
        const bool quad = n >= 32 && tuning().group_quad;
        for (size_t half = n / 2; half >= 1; half >>= 1) {
            if (quad)
                hipLaunchKernelGGL(g1_ntt_stage_quad_kernel, dim3((unsigned)(n * 2 / 64)), dim3(64), 0, st, d_pts, n, half, (const fr_mem_t*)d_tw, n / (2 * half));
            else
                hipLaunchKernelGGL(g1_ntt_stage_kernel, dim3((unsigned)((n / 2 + 63) / 64)), dim3(64), 0, st, d_pts, n, half, (const fr_mem_t*)d_tw, n / (2 * half));
        }
        hipLaunchKernelGGL(g1_bitrev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pts, n, (int)lg);
        if (inverse) {  // * size_inv (domain.rs:190)
            fr_mem_t k_int;
            fr_t::from_u32((uint32_t)n).inverse().mont_to_int().store(&k_int);
            if (quad)
                hipLaunchKernelGGL(g1_scale_quad_kernel, dim3((unsigned)(n * 4 / 64)), dim3(64), 0, st, d_pts, n, k_int);
            else
                hipLaunchKernelGGL(g1_scale_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_pts, n, k_int);
        }
    }
    hipLaunchKernelGGL(g1_xyzz_to_jac_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const g1_xyzz_mem_t*)d_pts, d_jac, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(inout_projective, d_jac, n * 144, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    API_END
}

// ---- test hooks: the NTT's plan, twiddle / coset-power composition and index maps, on the host --------------------------------------
// Every function below calls the same __host__ __device__ code as ntt_pass_kernel_v2 and the driver (ntt.hip.h).
// the pass radices of the 2^lg plan -> out[0 .. 3]; returns the number of passes, -1 when lg is rejected
int snarkvm_hip_selftest_ntt_plan(uint32_t lg, int32_t* out) {
    const ntt_plan_t pl = ntt_make_plan(lg > 1024 ? -1 : (int)lg);
    for (int i = 0; i < NTT_MAX_PASSES; i++) out[i] = pl.a[i];
    return pl.npass ? pl.npass : -1;
}

// the device's tables, built on the host by the set-up code of the kernels
static const ntt_tables_t& ntt_host_tables() {
    static std::vector<fr_mem_t> mem;
    static ntt_tables_t tb{};
    static std::once_flag once;
    std::call_once(once, [] {
        mem.resize(8 * NTT_TW_SIZE + 2 * NTT_LOCAL + 4 * NTT_TOP + 32 + 8);
        size_t off = 0;
        auto take = [&](size_t n) {
            fr_mem_t* r = mem.data() + off;
            off += n;
            return r;
        };
        for (int d = 0; d < 2; d++) {
            tb.pow_lo[d] = take(NTT_TW_SIZE);
            tb.pow_hi[d] = take(NTT_TW_SIZE);
            tb.g_lo[d] = take(NTT_TW_SIZE);
            tb.g_hi[d] = take(NTT_TW_SIZE);
            tb.local[d] = take(NTT_LOCAL);
            tb.pow_top[d] = take(NTT_TOP);
            tb.g_top[d] = take(NTT_TOP);
        }
        tb.size_inv = take(32);
        tb.consts = take(8);
        ntt_setup_consts_on(tb);
        for (int i = 0; i < NTT_TW_SIZE; i++) ntt_fill_tables_at(tb, i);
    });
    return tb;
}
static bool ntt_plan_from(uint32_t lg, const int32_t* plan, int npass, ntt_plan_t& pl) {
    if (lg > (uint32_t)NTT_LG_MAX) return false;
    if (!plan) {
        pl = ntt_make_plan((int)lg);
        return pl.npass > 0;
    }
    if (npass < 1 || npass > NTT_MAX_PASSES) return false;
    int sum = 0;
    for (int i = 0; i < NTT_MAX_PASSES; i++) {
        pl.a[i] = i < npass ? plan[i] : 0;
        if (i < npass && (pl.a[i] < 1 || pl.a[i] > NTT_MAX_RADIX_LG) && !(npass == 1 && pl.a[i] == 0)) return false;
        sum += pl.a[i];
    }
    pl.npass = npass;
    return sum == (int)lg;
}

// kind 0: out[i] = the closing twiddle of pass `pass` of the 2^lg transform for inner * k = x[i], i.e. W28^(x[i] << tw_shift)
//         (pass = -1: W28^x[i] itself), inverse: of W28^-1;
// kind 1: out[i] = g^x[i] (inverse: g^-x[i]).  Values in memory Montgomery form.  0, or -1: an argument or exponent out of range.
int snarkvm_hip_selftest_ntt_twiddle(int kind, uint32_t lg, int pass, int inverse, const uint64_t* x, size_t n, void* out) {
    const ntt_tables_t& tb = ntt_host_tables();
    int shift = 0;
    if (kind == 0 && pass >= 0) {
        ntt_plan_t pl;
        if (!ntt_plan_from(lg, nullptr, 0, pl) || pass >= pl.npass - 1) return -1;
        shift = ntt_pass_geometry(pl, (int)lg, pass).tw_shift;
    }
    if ((kind != 0 && kind != 1) || (inverse != 0 && inverse != 1)) return -1;
    fr_mem_t* o = (fr_mem_t*)out;
    for (size_t i = 0; i < n; i++) {
        if (x[i] >= ((uint64_t)1 << (NTT_LG_MAX - shift))) return -1;
        const uint32_t e = (uint32_t)(x[i] << shift);
        const fr_t w = kind == 0 ? ntt_twiddle(tb, inverse, e) : ntt_coset_pow(tb, inverse, e);
        w.to_mem_mont().store(&o[i]);
    }
    return 0;
}

// Index maps of the 2^lg plan (plan = NULL: the driver's; else npass forced radices), indices only.  Every non-last pass must read and
// write each position once and put its output digit at the position the next passes read it from; the last pass must write every
// output index once, and the value it writes at index f must be the transform's coefficient f: the digits the earlier passes left in
// its input position (leading digit first) followed by the last pass' own digit.  Returns the number of violations (saturated), -1: bad
// arguments.
int snarkvm_hip_selftest_ntt_index(uint32_t lg, const int32_t* plan, int npass) {
    ntt_plan_t pl;
    if (!ntt_plan_from(lg, plan, npass, pl)) return -1;
    const size_t n = (size_t)1 << lg;
    size_t bad = 0;
    std::vector<uint8_t> seen_in(n), seen_out(n);
    int consumed = 0;
    for (int k = 0; k < pl.npass; k++) {
        ntt_pass_t p = ntt_pass_geometry(pl, (int)lg, k);
        std::fill(seen_in.begin(), seen_in.end(), 0);
        std::fill(seen_out.begin(), seen_out.end(), 0);
        const int R = 1 << p.a;
        if (!p.last) {
            p.lgT = ntt_tile_lg(p.a, p.s, (int)lg);
            const size_t tiles = n >> (p.a + p.lgT);
            const int digit_at = (int)lg - consumed - p.a;  // where the next passes read this pass' digit
            for (size_t t = 0; t < tiles; t++) {
                const ntt_inner_tile_t it = ntt_inner_tile(p, t);
                for (int col = 0; col < (1 << p.lgT); col++)
                    for (int row = 0; row < R; row++) {
                        const size_t in = it.in_base + ((size_t)row << p.s) + col;
                        const uint32_t d = bitrev32((uint32_t)row, p.a);
                        const size_t o = it.in_base + ((size_t)d << p.s) + col;
                        if (in >= n || o >= n || seen_in[in]++ || seen_out[o]++) {
                            bad++;
                            continue;
                        }
                        const size_t mask = (size_t)(R - 1) << digit_at;
                        if (((o & mask) >> digit_at) != d || (o & ~mask) != (in & ~mask)) bad++;
                    }
            }
        } else {
            p.lgT = ntt_tile_lg(p.a, p.a1, (int)lg);
            const size_t tiles = n >> (p.a + p.lgT);
            const size_t col_stride = (size_t)1 << (lg - p.a1);
            for (size_t t = 0; t < tiles; t++) {
                const ntt_last_tile_t lt = ntt_last_tile(p, t);
                for (int col = 0; col < (1 << p.lgT); col++)
                    for (int row = 0; row < R; row++) {
                        const size_t in = lt.in_base + row + col * col_stride;
                        const size_t o = ntt_last_out_index(p, t, row, col);
                        if (in >= n || o >= n || seen_in[in]++ || seen_out[o]++) {
                            bad++;
                            continue;
                        }
                        // the coefficient this slot holds: the earlier digits in memory (leading first) + the last pass' digit
                        size_t f = 0;
                        int at = 0, top = (int)lg;
                        for (int i = 0; i + 1 < pl.npass; i++) {
                            top -= pl.a[i];
                            f |= ((in >> top) & (((size_t)1 << pl.a[i]) - 1)) << at;
                            at += pl.a[i];
                        }
                        if ((in & (((size_t)1 << top) - 1)) != (size_t)row) bad++;  // the row is the last pass' input digit
                        f |= (size_t)bitrev32((uint32_t)row, p.a) << at;
                        if (f != o) bad++;
                    }
            }
        }
        consumed += p.a;
    }
    return bad > 0x7fffffff ? 0x7fffffff : (int)bad;
}

// The whole NN transform of 2^lg (<= 2^16) elements on the host in exact arithmetic, pass by pass as ntt_run_nn schedules it (plan = NULL:
// the driver's plan; else npass forced radices): every pass a plain DFT of its radix over the kernels' tile addressing, the kernels'
// closing twiddles, coset powers and output index map.  inout: memory Montgomery form.  0, or -1: bad arguments.
int snarkvm_hip_selftest_ntt_host(void* inout, uint32_t lg, const int32_t* plan, int npass, int dir, int type) {
    ntt_plan_t pl;
    if (lg > 16 || !ntt_plan_from(lg, plan, npass, pl) || dir < 0 || dir > 1 || type < 0 || type > 1) return -1;
    if (lg == 0) return 0;
    const ntt_tables_t& tb = ntt_host_tables();
    const size_t n = (size_t)1 << lg;
    std::vector<fr_t> cur(n), nxt(n);
    fr_mem_t* io = (fr_mem_t*)inout;
    for (size_t i = 0; i < n; i++) cur[i] = fr_t::load(&io[i]).from_mem_mont();
    for (int k = 0; k < pl.npass; k++) {
        ntt_pass_t p = ntt_pass_geometry(pl, (int)lg, k);
        const int R = 1 << p.a;
        std::vector<fr_t> x(R);
        // powers of this pass' own root w_(2^a) = W28^(2^(28 - a))
        std::vector<fr_t> wr(R);
        for (int e = 0; e < R; e++) wr[e] = ntt_twiddle(tb, dir, (uint32_t)e << (NTT_LG_MAX - p.a));
        auto dft = [&](int d) {
            fr_t acc = fr_t::zero();
            for (int j = 0; j < R; j++) acc = acc + x[j] * wr[(j * d) & (R - 1)];
            return acc;
        };
        if (!p.last) {
            p.lgT = ntt_tile_lg(p.a, p.s, (int)lg);
            for (size_t t = 0; t < (n >> (p.a + p.lgT)); t++) {
                const ntt_inner_tile_t it = ntt_inner_tile(p, t);
                for (int col = 0; col < (1 << p.lgT); col++) {
                    for (int j = 0; j < R; j++) {
                        const size_t g = it.in_base + ((size_t)j << p.s) + col;
                        x[j] = cur[g];
                        if (k == 0 && dir == NTT_FORWARD && type == NTT_COSET) x[j] = x[j] * ntt_coset_pow(tb, 0, (uint32_t)g);
                    }
                    for (int row = 0; row < R; row++) {
                        const uint32_t d = bitrev32((uint32_t)row, p.a);
                        const uint32_t expo = (uint32_t)(((it.inner0 + col) * (size_t)d) << p.tw_shift);
                        nxt[it.in_base + ((size_t)d << p.s) + col] = dft((int)d) * ntt_twiddle(tb, dir, expo);
                    }
                }
            }
        } else {
            p.lgT = ntt_tile_lg(p.a, p.a1, (int)lg);
            const size_t col_stride = (size_t)1 << (lg - p.a1);
            for (size_t t = 0; t < (n >> (p.a + p.lgT)); t++) {
                const ntt_last_tile_t lt = ntt_last_tile(p, t);
                for (int col = 0; col < (1 << p.lgT); col++) {
                    for (int j = 0; j < R; j++) {
                        const size_t g = lt.in_base + j + col * col_stride;
                        x[j] = cur[g];
                        if (pl.npass == 1 && dir == NTT_FORWARD && type == NTT_COSET) x[j] = x[j] * ntt_coset_pow(tb, 0, (uint32_t)g);
                    }
                    for (int row = 0; row < R; row++) {
                        const size_t g = ntt_last_out_index(p, t, row, col);
                        fr_t y = dft((int)bitrev32((uint32_t)row, p.a));
                        if (dir == NTT_INVERSE) y = y * fr_t::load(&tb.size_inv[lg]);
                        if (dir == NTT_INVERSE && type == NTT_COSET) y = y * ntt_coset_pow(tb, 1, (uint32_t)g);
                        nxt[g] = y;
                    }
                }
            }
        }
        cur.swap(nxt);
    }
    for (size_t i = 0; i < n; i++) cur[i].to_mem_mont().store(&io[i]);
    return 0;
}

}  // extern "C"

