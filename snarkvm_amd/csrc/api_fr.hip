// api_fr.hip - the Fr-side entry points of the C ABI: NTT / polymul (the reference's snarkvm_ntt, snarkvm_polymul), the
// prover-round polynomial kernels and the setup-time group operations that are built on them.  A separate translation unit so
// that build.py can compile it next to api.hip (G1 MSM) and api_g2.hip.
#include "msm_run.hip.h"  // convert_bases (g1_fixed_base_msm)
#include "group.hip.h"
#include "poly.hip.h"

#include <algorithm>

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
        const uint8_t *o = (const uint8_t*)d_out, *q = (const uint8_t*)ptr;
        if (q != o && len && q < o + bytes && o < q + sizeof(fr_mem_t) * len) throw hip_failure{hipErrorInvalidValue, "polymul_device: d_out overlaps an operand", __LINE__};
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

// ---- prover-round polynomial kernels (poly.hip.h) ---------------------------------------------------
static fr_mem_t fr_mem_from_host(const void* p) {
    fr_mem_t m;
    memcpy(&m, p, sizeof m);
    return m;
}
static unsigned fr_grid(size_t n, unsigned block = 256) {
    const size_t b = (n + block - 1) / block;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
// operand `p` (n elements) as a device pointer: itself, or a staged copy in ctx.poly[slot]
static fr_mem_t* fr_stage_in(lane_t& c, int slot, const void* p, size_t n, int on_device) {
    if (on_device || !p) return (fr_mem_t*)p;
    c.poly[slot].ensure(sizeof(fr_mem_t) * (n ? n : 1));
    if (n) HIP_TRY(hipMemcpyAsync(c.poly[slot].p, p, sizeof(fr_mem_t) * n, hipMemcpyHostToDevice, c.stream));
    return c.poly[slot].as<fr_mem_t>();
}
static fr_mem_t* fr_stage_out(lane_t& c, int slot, void* p, size_t n, int on_device) {
    if (on_device || !p) return (fr_mem_t*)p;
    c.poly[slot].ensure(sizeof(fr_mem_t) * (n ? n : 1));
    return c.poly[slot].as<fr_mem_t>();
}
static void fr_finish_out(lane_t& c, fr_mem_t* d, void* p, size_t n, int on_device) {
    if (!on_device && p && n) HIP_TRY(hipMemcpyAsync(p, d, sizeof(fr_mem_t) * n, hipMemcpyDeviceToHost, c.stream));
}
// end of a vector call: device-resident operands may leave the wait to the calling thread's scope (runtime.hip.h), host operands never
static void fr_call_done(lane_t& c, int on_device) {
    if (on_device)
        c.sync_or_defer();
    else
        HIP_TRY(hipStreamSynchronize(c.stream));
}

static void check_strided(size_t n, size_t count, size_t stride, int on_device, const char* who) {
    (void)who;
    if (count == 0 || (count > 1 && (!on_device || stride < n)) || count > 65535)
        throw hip_failure{hipErrorInvalidValue, "strided batch of an Fr vector pass: needs device operands, 1 <= count <= 65535 and stride >= the vector length", __LINE__};
}
static RustError fr_vec_op_impl(int op, void* out, const void* a, const void* b, const void* c3, const void* scalar, size_t n, int on_device, size_t count,
                                size_t stride) {
    API_BEGIN_DEV(device_for(a, (on_device && n) ? 1 : 0))
    if (op < 0 || op > FR_OP_RSUB_SCALAR) throw hip_failure{hipErrorInvalidValue, "fr_vec_op: unknown op", __LINE__};
    check_strided(n, count, stride, on_device, "fr_vec_op");
    const bool need_b = op == FR_OP_ADD || op == FR_OP_SUB || op == FR_OP_MUL || op == FR_OP_MUL_SUB || op == FR_OP_AXPY;
    const bool need_c = op == FR_OP_MUL_SUB;
    const bool need_s = op == FR_OP_SCALE || op == FR_OP_SUB_SCALAR || op == FR_OP_AXPY || op == FR_OP_RSUB_SCALAR;
    if (n && (!out || !a || (need_b && !b) || (need_c && !c3) || (need_s && !scalar)))
        throw hip_failure{hipErrorInvalidValue, "fr_vec_op: missing operand", __LINE__};
    if (n) {
        fr_mem_t s{};
        if (need_s) s = fr_mem_from_host(scalar);
        const fr_mem_t* da = fr_stage_in(c, 0, a, n, on_device);
        const fr_mem_t* db = need_b ? fr_stage_in(c, 1, b, n, on_device) : nullptr;
        const fr_mem_t* dc = need_c ? fr_stage_in(c, 2, c3, n, on_device) : nullptr;
        fr_mem_t* dout = fr_stage_out(c, 3, out, n, on_device);
        hipLaunchKernelGGL(fr_vec_op_kernel, dim3(fr_grid(n), (unsigned)count), dim3(256), 0, c.stream, op, dout, da, db, dc, s, n, stride);
        HIP_TRY(hipGetLastError());
        fr_finish_out(c, dout, out, n, on_device);
        fr_call_done(c, on_device);
    }
    API_END
}
RustError snarkvm_hip_fr_vec_op(int op, void* out, const void* a, const void* b, const void* c3, const void* scalar, size_t n, int on_device) {
    return fr_vec_op_impl(op, out, a, b, c3, scalar, n, on_device, 1, 0);
}
RustError snarkvm_hip_fr_vec_op_strided(int op, void* out, const void* a, const void* b, const void* c3, const void* scalar, size_t n, size_t count, size_t stride) {
    return fr_vec_op_impl(op, out, a, b, c3, scalar, n, 1, count, stride);
}

// out[i - shift] = h_i = sum_{k >= i} in[k] m^(k - i) (and *first = h_0 when shift == 1); `out` may be null (only h_0 wanted).
// Scratch for the chunk values of every level lives in the lane's poly[4].
static void fr_suffix_horner(lane_t& c, const fr_mem_t* d_in, size_t n, const fr_mem_t& m, fr_mem_t* d_out, int shift, fr_mem_t* d_first, size_t count = 1,
                             size_t in_stride = 0, size_t out_stride = 0) {
    // `count` vectors in one launch sequence (blockIdx.y): inputs / outputs `in_stride` / `out_stride` elements apart, the chunk values
    // of vector y in its own slice of the scratch area, d_first[y] = h_0 of vector y
    hipStream_t st = c.stream;
    if (d_out && n >= 2048 && n <= ((size_t)1 << 20) && tuning().horner2) {
        // quotient wanted, a proof-sized polynomial: the three-launch form with a scan inside every workgroup (poly.hip.h); C coefficients per thread keep
        // <= 256 workgroups.  (Beyond 2^20 coefficients a thread would fold 32+ of them serially on a quarter of the chip's lanes - round 3 measured that
        // shape at 2^24: 1.69 vs 1.04 ms - and the chunk recursion below, 2^19 threads at its first level, is the better form.)
        uint32_t C = 8;
        while (((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B > 256) C *= 2;
        const size_t nblocks = ((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B;
        const size_t hs_stride = nblocks * HORNER2_B, bv_stride = nblocks;
        c.poly[4].ensure(sizeof(fr_mem_t) * (HORNER2_TAB + count * (hs_stride + bv_stride)));
        fr_mem_t* tab = c.poly[4].as<fr_mem_t>();
        fr_mem_t* hs = tab + HORNER2_TAB;
        fr_mem_t* bv = hs + count * hs_stride;
        hipLaunchKernelGGL(fr_horner2_tables_kernel, dim3(1), dim3(HORNER2_B), 0, st, m, tab, C);
        hipLaunchKernelGGL(fr_horner2_up_kernel, dim3((unsigned)nblocks, (unsigned)count), dim3(HORNER2_B), 0, st, d_in, n, m, (const fr_mem_t*)tab, hs, bv, C, in_stride,
                           hs_stride, bv_stride);
        hipLaunchKernelGGL(fr_horner2_down_kernel, dim3((unsigned)nblocks, (unsigned)count), dim3(HORNER2_B), 0, st, d_in, n, m, (const fr_mem_t*)tab, (const fr_mem_t*)hs,
                           (const fr_mem_t*)bv, C, d_out, shift, d_first, in_stride, hs_stride, bv_stride, out_stride);
        HIP_TRY(hipGetLastError());
        return;
    }
    int levels = 1;
    size_t total = 0;
    for (size_t t = n; t > 1;) {
        t = (t + POLY_CHUNK - 1) / POLY_CHUNK;
        total += t;
        levels++;
    }
    c.poly[4].ensure(sizeof(fr_mem_t) * (total * count + levels + 2));
    fr_mem_t* mult = c.poly[4].as<fr_mem_t>();
    fr_mem_t* cvbase = mult + levels + 1;
    const unsigned ny = (unsigned)count;
    hipLaunchKernelGGL(fr_horner_multipliers_kernel, dim3(1), dim3(1), 0, st, m, mult, levels);
    // up-sweep: level k holds the chunk values of level k - 1 (level 0 = the input)
    std::vector<const fr_mem_t*> in_at{d_in};
    std::vector<size_t> n_at{n}, stride_at{in_stride};
    fr_mem_t* next = cvbase;
    while (n_at.back() > 1) {
        const size_t cur = n_at.back();
        const size_t T = (cur + POLY_CHUNK - 1) / POLY_CHUNK;
        const int k = (int)n_at.size() - 1;
        hipLaunchKernelGGL(fr_horner_up_kernel, dim3((unsigned)((T + 255) / 256), ny), dim3(256), 0, st, in_at.back(), cur, mult + k, next, T, stride_at.back(), total);
        in_at.push_back(next);
        n_at.push_back(T);
        stride_at.push_back(total);
        next += T;
    }
    // the single value of the top level is h_0 of every level below; down-sweep turns each level's chunk values into
    // its suffix sums in place, the input level writes to `out`
    const int top = (int)n_at.size() - 1;
    for (int k = top; k >= 0; k--) {
        const size_t cur = n_at[k];
        const size_t T = (cur + POLY_CHUNK - 1) / POLY_CHUNK;
        const fr_mem_t* carry = (k < top) ? in_at[k + 1] : nullptr;
        if (k > 0) {
            if (k == top) continue;  // one element: it already is its own suffix sum
            hipLaunchKernelGGL(fr_horner_down_kernel, dim3((unsigned)((T + 255) / 256), ny), dim3(256), 0, st, in_at[k], cur, mult + k, carry, T,
                               (fr_mem_t*)in_at[k], 0, (fr_mem_t*)nullptr, total, total, total);
        } else if (d_out) {
            hipLaunchKernelGGL(fr_horner_down_kernel, dim3((unsigned)((T + 255) / 256), ny), dim3(256), 0, st, d_in, cur, mult, carry, T, d_out, shift,
                               d_first, in_stride, total, out_stride);
        } else if (d_first) {
            // only h_0: the value of the top level, or of the lone input element
            for (size_t y = 0; y < count; y++)
                HIP_TRY(hipMemcpyAsync(d_first + y, (top > 0 ? in_at[top] : d_in) + y * (top > 0 ? total : in_stride), sizeof(fr_mem_t), hipMemcpyDeviceToDevice, st));
        }
    }
    HIP_TRY(hipGetLastError());
}

static RustError fr_divide_by_linear_impl(void* quotient, void* remainder, const void* poly, size_t n, const void* point, int on_device, size_t count,
                                          size_t stride) {
    API_BEGIN_DEV(device_for(poly, (on_device && n) ? 1 : 0))
    if (!point || (n && !poly)) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_linear: missing operand", __LINE__};
    check_strided(n, count, stride, on_device, "fr_divide_by_linear");
    if (on_device && quotient && n > 1) {  // header: different workgroups own adjacent coefficient ranges - an in-place division would race
        const size_t span = sizeof(fr_mem_t) * ((count - 1) * stride + n);
        const uint8_t *q = (const uint8_t*)quotient, *p = (const uint8_t*)poly;
        if (q < p + span && p < q + span) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_linear: quotient overlaps poly (device operands must not alias)", __LINE__};
    }
    if (n == 0) {
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t) * count);
    } else {
        const fr_mem_t z = fr_mem_from_host(point);
        const fr_mem_t* din = fr_stage_in(c, 0, poly, n, on_device);
        fr_mem_t* dq = (quotient && n > 1) ? fr_stage_out(c, 1, quotient, n - 1, on_device) : nullptr;
        c.poly[2].ensure(sizeof(fr_mem_t) * count);
        fr_mem_t* drem = c.poly[2].as<fr_mem_t>();
        fr_suffix_horner(c, din, n, z, dq, 1, drem, count, stride, stride);
        if (dq) fr_finish_out(c, dq, quotient, n - 1, on_device);
        // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the value is there on return
        if (remainder) c.host_result(remainder, drem, sizeof(fr_mem_t) * count, on_device != 0);
        fr_call_done(c, on_device);
    }
    API_END
}
RustError snarkvm_hip_fr_divide_by_linear(void* quotient, void* remainder, const void* poly, size_t n, const void* point, int on_device) {
    return fr_divide_by_linear_impl(quotient, remainder, poly, n, point, on_device, 1, 0);
}
RustError snarkvm_hip_fr_divide_by_linear_strided(void* quotients, void* remainders, const void* polys, size_t n, const void* point, size_t count, size_t stride) {
    return fr_divide_by_linear_impl(quotients, remainders, polys, n, point, 1, count, stride);
}

static void fr_batch_inverse_run(lane_t& c, fr_mem_t* d_v, size_t n, const fr_mem_t& coeff) {
    // >= 32 elements per thread amortise the per-thread Fermat inversion; cap the thread count for huge vectors
    size_t T = (n + 31) / 32;
    if (T > (size_t)1 << 17) T = (size_t)1 << 17;
    c.poly[4].ensure(sizeof(fr_mem_t) * n);
    hipLaunchKernelGGL(fr_batch_inverse_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, c.stream, d_v, n, coeff, c.poly[4].as<fr_mem_t>(), T);
    HIP_TRY(hipGetLastError());
}
RustError snarkvm_hip_fr_batch_inversion_and_mul(void* inout, size_t n, const void* coeff, int on_device) {
    API_BEGIN_DEV(device_for(inout, (on_device && n) ? 1 : 0))
    if (n) {
        if (!inout || !coeff) throw hip_failure{hipErrorInvalidValue, "fr_batch_inversion_and_mul: missing operand", __LINE__};
        fr_mem_t* dv = fr_stage_in(c, 0, inout, n, on_device);
        fr_batch_inverse_run(c, dv, n, fr_mem_from_host(coeff));
        fr_finish_out(c, dv, inout, n, on_device);
        fr_call_done(c, on_device);
    }
    API_END
}

static void fr_distribute_powers_run(lane_t& c, fr_mem_t* d_v, size_t n, const fr_mem_t& g, const fr_mem_t& cmul) {
    size_t T = (n + 31) / 32;
    if (T > (size_t)1 << 17) T = (size_t)1 << 17;
    hipLaunchKernelGGL(fr_distribute_powers_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, c.stream, d_v, n, g, cmul, T);
    HIP_TRY(hipGetLastError());
}
RustError snarkvm_hip_fr_distribute_powers(void* inout, size_t n, const void* g, const void* cmul, int on_device) {
    API_BEGIN_DEV(device_for(inout, (on_device && n) ? 1 : 0))
    if (n) {
        if (!inout || !g || !cmul) throw hip_failure{hipErrorInvalidValue, "fr_distribute_powers: missing operand", __LINE__};
        fr_mem_t* dv = fr_stage_in(c, 0, inout, n, on_device);
        fr_distribute_powers_run(c, dv, n, fr_mem_from_host(g), fr_mem_from_host(cmul));
        fr_finish_out(c, dv, inout, n, on_device);
        fr_call_done(c, on_device);
    }
    API_END
}

// TWO_ADIC_ROOT_OF_UNITY (fr.rs:115-120), memory form - the host copy of ntt.hip.h's device table
static const uint32_t FR_TWO_ADIC_ROOT_MEM_HOST[8] = {0xda3ad648u, 0xaf80da4du, 0xfc381dacu, 0x5e223adbu,
                                                      0xb2f92525u, 0x03ba0666u, 0x3befb0ceu, 0x0f906c5bu};
RustError snarkvm_hip_fr_lagrange_coefficients(void* out, uint32_t lg, const void* tau, int on_device) {
    API_BEGIN_DEV(device_for(out, (on_device && out) ? 1 : 0))
    if (lg > 30) throw hip_failure{hipErrorInvalidValue, "fr_lagrange_coefficients: lg_domain_size > 30", __LINE__};
    if (!out || !tau) throw hip_failure{hipErrorInvalidValue, "fr_lagrange_coefficients: missing operand", __LINE__};
    const size_t n = (size_t)1 << lg;
    // scalar set-up with the same arithmetic compiled for the host (domain.rs:118-147, 258-264)
    fr_t omega = fr_t::unpack(FR_TWO_ADIC_ROOT_MEM_HOST).from_mem_mont();
    for (uint32_t i = lg; i < 47; i++) omega = omega.sqr();
    const fr_mem_t tau_mem = fr_mem_from_host(tau);
    const fr_t tau_i = fr_t::load(&tau_mem).from_mem_mont();
    const fr_t t_size = tau_i.pow_u64((uint64_t)n);
    fr_mem_t one_mem, omega_mem;
    fr_t::one().to_mem_mont().store(&one_mem);
    omega.to_mem_mont().store(&omega_mem);
    fr_mem_t* du = fr_stage_out(c, 0, out, n, on_device);
    hipStream_t st = c.stream;
    hipLaunchKernelGGL(fr_fill_kernel, dim3(fr_grid(n)), dim3(256), 0, st, du, n, one_mem);
    fr_distribute_powers_run(c, du, n, omega_mem, one_mem);  // u_i = omega^i
    if (t_size == fr_t::one()) {
        hipLaunchKernelGGL(fr_onehot_kernel, dim3(fr_grid(n)), dim3(256), 0, st, du, n, tau_mem, one_mem);
    } else {
        fr_mem_t l_mem;
        ((t_size - fr_t::one()) * fr_t::from_u32((uint32_t)n).inverse()).to_mem_mont().store(&l_mem);
        hipLaunchKernelGGL(fr_vec_op_kernel, dim3(fr_grid(n)), dim3(256), 0, st, (int)FR_OP_RSUB_SCALAR, du, (const fr_mem_t*)du, (const fr_mem_t*)nullptr,
                           (const fr_mem_t*)nullptr, tau_mem, n, (size_t)0);  // tau - omega^i
        fr_batch_inverse_run(c, du, n, one_mem);
        fr_distribute_powers_run(c, du, n, omega_mem, l_mem);  // * l * omega^i
    }
    HIP_TRY(hipGetLastError());
    fr_finish_out(c, du, out, n, on_device);
    fr_call_done(c, on_device);
    API_END
}

static RustError fr_divide_by_vanishing_impl(void* quotient, void* remainder, const void* poly, size_t len, size_t domain_size, int on_device, size_t count,
                                             size_t stride) {
    API_BEGIN_DEV(device_for(poly, (on_device && len) ? 1 : 0))
    if (domain_size == 0) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_vanishing: empty domain", __LINE__};
    check_strided(len, count, stride, on_device, "fr_divide_by_vanishing");
    if (len) {
        if (!poly || !remainder || (len > domain_size && !quotient)) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_vanishing: missing operand", __LINE__};
        const size_t qlen = len > domain_size ? len - domain_size : 0;
        const size_t rlen = len < domain_size ? len : domain_size;
        const fr_mem_t* din = fr_stage_in(c, 0, poly, len, on_device);
        fr_mem_t* dq = qlen ? fr_stage_out(c, 1, quotient, qlen, on_device) : nullptr;
        fr_mem_t* dr = fr_stage_out(c, 2, remainder, rlen, on_device);
        const size_t threads = qlen > rlen ? qlen : rlen;
        hipLaunchKernelGGL(fr_fold_vanishing_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)count), dim3(256), 0, c.stream, din, len, domain_size, dq, dr,
                           stride);
        HIP_TRY(hipGetLastError());
        if (qlen) fr_finish_out(c, dq, quotient, qlen, on_device);
        fr_finish_out(c, dr, remainder, rlen, on_device);
        fr_call_done(c, on_device);
    }
    API_END
}
RustError snarkvm_hip_fr_divide_by_vanishing(void* quotient, void* remainder, const void* poly, size_t len, size_t domain_size, int on_device) {
    return fr_divide_by_vanishing_impl(quotient, remainder, poly, len, domain_size, on_device, 1, 0);
}
RustError snarkvm_hip_fr_divide_by_vanishing_strided(void* quotients, void* remainders, const void* polys, size_t len, size_t domain_size, size_t count, size_t stride) {
    return fr_divide_by_vanishing_impl(quotients, remainders, polys, len, domain_size, 1, count, stride);
}
RustError snarkvm_hip_fr_mul_by_vanishing(void* out, const void* poly, size_t len, size_t domain_size, int on_device) {
    API_BEGIN_DEV(device_for(out, (on_device && out) ? 1 : 0))
    const size_t olen = len + domain_size;
    if (olen) {
        if (!out || (len && !poly)) throw hip_failure{hipErrorInvalidValue, "fr_mul_by_vanishing: missing operand", __LINE__};
        const fr_mem_t* din = fr_stage_in(c, 0, poly, len, on_device);
        fr_mem_t* dout = fr_stage_out(c, 1, out, olen, on_device);
        hipLaunchKernelGGL(fr_mul_vanishing_kernel, dim3((unsigned)((olen + 255) / 256)), dim3(256), 0, c.stream, din, len, domain_size, dout);
        HIP_TRY(hipGetLastError());
        fr_finish_out(c, dout, out, olen, on_device);
        fr_call_done(c, on_device);
    }
    API_END
}

// ---- linear combination of polynomials (poly.hip.h: fr_lincomb_kernel) --------------------------------------------------
// What the device call and its host replay share: validation, operand order and the split into launches.  src[k]: the caller's index of
// table entry k, -1 for `out` taken back in as a term with coefficient one (every launch after the first).
struct fr_lincomb_launch_t {
    fr_lincomb_t t;
    int64_t src[FR_LINCOMB_CHUNK];
};
// nullptr, or why the call is refused (hipErrorInvalidValue).  Nothing has been touched either way.
static const char* fr_lincomb_plan(const void* out, size_t n_out, size_t count, const void* const* polys, const size_t* lens, const void* coeffs,
                                   std::vector<fr_lincomb_launch_t>& plan) {
    if (!out || (count && (!polys || !lens || !coeffs))) return "missing argument";
    struct entry_t {
        size_t k, len;
        bool aliased;
    };
    std::vector<entry_t> live;
    size_t aliased = 0;
    const uint8_t* o = (const uint8_t*)out;
    for (size_t k = 0; k < count; k++) {
        const size_t len = lens[k];
        if (len > n_out) return "an operand is longer than n_out";
        if (!len) continue;
        const uint8_t* q = (const uint8_t*)polys[k];
        if (!q) return "null operand of non-zero length";
        // out may BE an operand (same start): a thread reads index i of every operand before it writes out[i].  Any other overlap is refused.
        if (q != o && q < o + sizeof(fr_mem_t) * n_out && o < q + sizeof(fr_mem_t) * len) return "out overlaps an operand";
        live.push_back({k, len, q == o});
        aliased += q == o;
    }
    const auto longer = [](const entry_t& a, const entry_t& b) { return a.len > b.len; };
    std::stable_sort(live.begin(), live.end(), longer);
    if (aliased && live.size() > (size_t)FR_LINCOMB_CHUNK) {
        // the first launch overwrites out: every operand that IS out goes into it, beside the longest of the others
        if (aliased > (size_t)FR_LINCOMB_CHUNK) return "out is an operand more often than one launch holds operands";
        std::stable_partition(live.begin(), live.end(), [](const entry_t& e) { return e.aliased; });
        std::stable_sort(live.begin(), live.begin() + FR_LINCOMB_CHUNK, longer);
    }
    size_t at = 0;
    do {
        fr_lincomb_launch_t L{};
        int m = 0;
        if (at) {  // the sum so far
            L.t.p[0] = (const fr_mem_t*)out, L.t.len[0] = n_out, L.src[0] = -1;
            for (int l = 0; l < 9; l++) L.t.c[0][l] = FrP::ONE[l];
            m = 1;
        }
        for (; m < FR_LINCOMB_CHUNK && at < live.size(); m++, at++) {
            const entry_t& e = live[at];
            const fr_mem_t c_mem = fr_mem_from_host((const uint8_t*)coeffs + sizeof(fr_mem_t) * e.k);
            const fr_t c = fr_t::load(&c_mem).from_mem_mont();
            L.t.p[m] = (const fr_mem_t*)polys[e.k], L.t.len[m] = e.len, L.src[m] = (int64_t)e.k;
            for (int l = 0; l < 9; l++) L.t.c[m][l] = c.v[l];
        }
        L.t.count = m;
        plan.push_back(L);
    } while (at < live.size());
    return nullptr;
}
RustError snarkvm_hip_fr_lincomb(void* out, size_t n_out, size_t count, const void* const* polys, const size_t* lens, const void* coeffs, int on_device) {
    if (n_out == 0) return ok();
    std::vector<fr_lincomb_launch_t> plan;
    if (const char* why = fr_lincomb_plan(out, n_out, count, polys, lens, coeffs, plan)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_lincomb: ") + why);
    API_BEGIN_DEV(device_for(out, on_device ? 1 : 0))
    fr_mem_t* dout = (fr_mem_t*)out;
    if (on_device) {
        for (size_t k = 0; k < count; k++)
            if (lens[k] && g_rt.devs[device_for(polys[k], 1)]->physical != c.dev->physical)
                throw hip_failure{hipErrorInvalidValue, "fr_lincomb: an operand lives on another device than out", __LINE__};
    } else {
        // host operands: one lane buffer holds out and, behind it, every operand; one upload each, one download
        size_t total = n_out;
        for (size_t k = 0; k < count; k++) total += lens[k];
        c.poly[0].ensure(sizeof(fr_mem_t) * total);
        dout = c.poly[0].as<fr_mem_t>();
        std::vector<const fr_mem_t*> staged(count, nullptr);
        fr_mem_t* next = dout + n_out;
        for (size_t k = 0; k < count; k++) {
            if (!lens[k]) continue;
            HIP_TRY(hipMemcpyAsync(next, polys[k], sizeof(fr_mem_t) * lens[k], hipMemcpyHostToDevice, c.stream));
            staged[k] = next;
            next += lens[k];
        }
        for (fr_lincomb_launch_t& L : plan)
            for (int m = 0; m < L.t.count; m++) L.t.p[m] = L.src[m] < 0 ? dout : staged[(size_t)L.src[m]];
    }
    for (const fr_lincomb_launch_t& L : plan) hipLaunchKernelGGL(fr_lincomb_kernel, dim3(fr_grid(n_out)), dim3(256), 0, c.stream, dout, n_out, L.t);
    HIP_TRY(hipGetLastError());
    fr_finish_out(c, dout, out, n_out, on_device);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernel's place: the same plan, every launch a loop over i through the kernel's own
// per-element routine.  0, or -1 when the plan refuses the arguments.
int snarkvm_hip_selftest_fr_lincomb(void* out, size_t n_out, size_t count, const void* const* polys, const size_t* lens, const void* coeffs) {
    if (n_out == 0) return 0;
    std::vector<fr_lincomb_launch_t> plan;
    if (fr_lincomb_plan(out, n_out, count, polys, lens, coeffs, plan)) return -1;
    fr_mem_t* o = (fr_mem_t*)out;
    for (const fr_lincomb_launch_t& L : plan)
        for (size_t i = 0; i < n_out; i++) fr_lincomb_at(L.t, i).store(&o[i]);
    return 0;
}

// ---- opening fold: a combination, its quotient by X - point and its value (poly.hip.h: fr_open_up_kernel ... fr_open2_down_kernel) -------
// What the device call and its host replay share: validation, operand order, the split into launches and the choice of the route.
static void fr_same_device(lane_t& c, const void* p, const char* what);
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  An empty plan: the
// combination is zero.  The LAST launch of the plan is the fused sweep, the ones before it are plain fr_lincomb_kernel launches.  With a
// quotient every launch after the first takes the quotient buffer - the sum so far - back in as its first term (src -1, coefficient one);
// without one every launch is an up sweep that stands alone, and the values of the launches are added.
static const char* fr_open_plan(const void* quotient, size_t n, size_t count, const void* const* polys, const size_t* lens, const void* coeffs, const void* point,
                                std::vector<fr_lincomb_launch_t>& plan) {
    if (!point) return "missing point";
    if (count && (!polys || !lens)) return "missing operand list";
    if (count && !coeffs) return "missing coeffs";
    struct entry_t {
        size_t k, len;
    };
    std::vector<entry_t> live;
    const uint8_t* o = (const uint8_t*)quotient;
    for (size_t k = 0; k < count; k++) {
        const size_t len = lens[k];
        if (len > n) return "an operand is longer than n";
        if (!len) continue;
        const uint8_t* q = (const uint8_t*)polys[k];
        if (!q) return "null operand of non-zero length";
        // the quotient buffer is the pass's only workspace: no operand may touch it, not even start where it starts
        if (o && q < o + sizeof(fr_mem_t) * n && o < q + sizeof(fr_mem_t) * len) return "quotient overlaps an operand";
        live.push_back({k, len});
    }
    if (live.empty()) return nullptr;
    std::stable_sort(live.begin(), live.end(), [](const entry_t& a, const entry_t& b) { return a.len > b.len; });
    size_t at = 0;
    // one table: the sum so far first (every launch into a quotient buffer but the first), then the members from `at` up to `end`
    const auto table = [&](size_t end) {
        fr_lincomb_launch_t L{};
        int m = 0;
        if (at && quotient) {
            L.t.p[0] = (const fr_mem_t*)quotient, L.t.len[0] = n, L.src[0] = -1;
            for (int l = 0; l < 9; l++) L.t.c[0][l] = FrP::ONE[l];
            m = 1;
        }
        for (; m < FR_LINCOMB_CHUNK && at < end; m++, at++) {
            const entry_t& e = live[at];
            const fr_mem_t c_mem = fr_mem_from_host((const uint8_t*)coeffs + sizeof(fr_mem_t) * e.k);
            const fr_t c = fr_t::load(&c_mem).from_mem_mont();
            L.t.p[m] = (const fr_mem_t*)polys[e.k], L.t.len[m] = e.len, L.src[m] = (int64_t)e.k;
            for (int l = 0; l < 9; l++) L.t.c[m][l] = c.v[l];
        }
        L.t.count = m;
        plan.push_back(L);
    };
    // with a quotient the fused sweep takes FR_OPEN_FUSE terms at most (poly.hip.h: one), the sum of the other members among them: those go
    // through plain accumulating launches first
    const size_t lead = quotient && live.size() > (size_t)FR_OPEN_FUSE ? live.size() - (FR_OPEN_FUSE - 1) : 0;
    while (at < lead) table(lead);
    do table(live.size());  // the fused launch (it may hold the sum alone); without a quotient one table after the other
    while (at < live.size());
    return nullptr;
}
// route 1: the three-launch scan (C coefficients per thread, `blocks` workgroups of HORNER2_B); route 0: the chunk recursion (C = POLY_CHUNK,
// `blocks` workgroups of 256 at its level 0).  The choice of fr_suffix_horner, which the quotient of a plain division goes through.
struct fr_open_geometry_t {
    int route;
    uint32_t C;
    size_t blocks;
};
static fr_open_geometry_t fr_open_geometry(size_t n, bool want_quotient) {
    if (want_quotient && n >= 2048 && n <= ((size_t)1 << 20) && tuning().horner2) {
        uint32_t C = 8;
        while (((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B > 256) C *= 2;
        return {1, C, ((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B};
    }
    const size_t T = (n + POLY_CHUNK - 1) / POLY_CHUNK;
    return {0, (uint32_t)POLY_CHUNK, (T + 255) / 256};
}
// the sizes of the levels of the chunk recursion: n, then the chunk values of the level below until one is left (always at least two levels:
// level 0 is the fused one, and its chunk values exist even for a single coefficient)
static std::vector<size_t> fr_open_levels(size_t n, size_t chunk) {
    std::vector<size_t> sizes{n};
    do sizes.push_back((sizes.back() + chunk - 1) / chunk);
    while (sizes.back() > 1);
    return sizes;
}
// enqueues the pass on the lane's stream; -> where the value h_0 will be (device memory, the lane's poly[4])
static const fr_mem_t* fr_open_run(lane_t& c, fr_mem_t* dq, size_t n, const fr_mem_t& z, const std::vector<fr_lincomb_launch_t>& plan) {
    hipStream_t st = c.stream;
    const fr_open_geometry_t g = fr_open_geometry(n, dq != nullptr);
    // a list longer than one table, quotient wanted: the leading tables are plain accumulating passes into the quotient buffer
    if (dq)
        for (size_t j = 0; j + 1 < plan.size(); j++) hipLaunchKernelGGL(fr_lincomb_kernel, dim3(fr_grid(n)), dim3(256), 0, st, dq, n, plan[j].t);
    if (g.route == 1) {
        const size_t nblocks = g.blocks;
        c.poly[4].ensure(sizeof(fr_mem_t) * (HORNER2_TAB + nblocks * HORNER2_B + nblocks + 1));
        fr_mem_t* tab = c.poly[4].as<fr_mem_t>();
        fr_mem_t* hs = tab + HORNER2_TAB;
        fr_mem_t* bv = hs + nblocks * HORNER2_B;
        fr_mem_t* res = bv + nblocks;
        hipLaunchKernelGGL(fr_horner2_tables_kernel, dim3(1), dim3(HORNER2_B), 0, st, z, tab, g.C);
        hipLaunchKernelGGL(fr_open2_up_kernel, dim3((unsigned)nblocks), dim3(HORNER2_B), 0, st, dq, n, z, (const fr_mem_t*)tab, hs, bv, g.C, plan.back().t);
        hipLaunchKernelGGL(fr_open2_down_kernel, dim3((unsigned)nblocks), dim3(HORNER2_B), 0, st, dq, n, z, (const fr_mem_t*)tab, (const fr_mem_t*)hs, (const fr_mem_t*)bv,
                           g.C, res);
        HIP_TRY(hipGetLastError());
        return res;
    }
    const std::vector<size_t> sizes = fr_open_levels(n, POLY_CHUNK);
    const int top = (int)sizes.size() - 1;
    std::vector<size_t> off(sizes.size(), 0);  // level k >= 1 at cv + off[k]
    size_t total = 0;
    for (int k = 1; k <= top; k++) off[k] = total, total += sizes[k];
    const size_t nl = plan.size();
    // mult[top + 1] | res | tops[nl] | cv[total]
    c.poly[4].ensure(sizeof(fr_mem_t) * ((size_t)top + 1 + 1 + nl + total));
    fr_mem_t* mult = c.poly[4].as<fr_mem_t>();
    fr_mem_t* res = mult + top + 1;
    fr_mem_t* tops = res + 1;
    fr_mem_t* cv = tops + nl;
    hipLaunchKernelGGL(fr_horner_multipliers_kernel, dim3(1), dim3(1), 0, st, z, mult, top + 1);
    // level k's chunk values; the single value of the top level goes to `top_at`
    const auto level = [&](int k, fr_mem_t* top_at) { return k == top ? top_at : cv + off[k]; };
    const auto up_from = [&](const fr_lincomb_t& t, fr_mem_t* q, fr_mem_t* top_at) {
        hipLaunchKernelGGL(fr_open_up_kernel, dim3((unsigned)((sizes[1] + 255) / 256)), dim3(256), 0, st, q, n, (const fr_mem_t*)mult, level(1, top_at), sizes[1], t);
        for (int k = 1; k < top; k++)
            hipLaunchKernelGGL(fr_horner_up_kernel, dim3((unsigned)((sizes[k + 1] + 255) / 256), 1u), dim3(256), 0, st, (const fr_mem_t*)level(k, top_at), sizes[k],
                               (const fr_mem_t*)(mult + k), level(k + 1, top_at), sizes[k + 1], (size_t)0, (size_t)0);
    };
    if (!dq) {
        // the value alone: by linearity one up sweep per table, the top values added in list order
        for (size_t j = 0; j < nl; j++) up_from(plan[j].t, nullptr, tops + j);
        if (nl > 1) hipLaunchKernelGGL(fr_open_sum_kernel, dim3(1), dim3(1), 0, st, (const fr_mem_t*)tops, (uint32_t)nl, res);
        HIP_TRY(hipGetLastError());
        return nl > 1 ? res : tops;
    }
    up_from(plan.back().t, dq, tops);
    // down: every level's chunk values become its suffix sums in place, level 0 turns the parked combination into the quotient
    for (int k = top - 1; k >= 1; k--)
        hipLaunchKernelGGL(fr_horner_down_kernel, dim3((unsigned)((sizes[k + 1] + 255) / 256), 1u), dim3(256), 0, st, (const fr_mem_t*)level(k, tops), sizes[k],
                           (const fr_mem_t*)(mult + k), (const fr_mem_t*)level(k + 1, tops), sizes[k + 1], level(k, tops), 0, (fr_mem_t*)nullptr, (size_t)0, (size_t)0,
                           (size_t)0);
    hipLaunchKernelGGL(fr_open_down_kernel, dim3((unsigned)((sizes[1] + 255) / 256)), dim3(256), 0, st, dq, n, (const fr_mem_t*)mult, (const fr_mem_t*)level(1, tops),
                       sizes[1], res);
    HIP_TRY(hipGetLastError());
    return res;
}
RustError snarkvm_hip_fr_open_fold(void* quotient, void* remainder, size_t n, size_t count, const void* const* polys, const size_t* lens, const void* coeffs,
                                   const void* point, int on_device) {
    if (n == 0) {
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t));
        return ok();
    }
    std::vector<fr_lincomb_launch_t> plan;
    if (const char* why = fr_open_plan(quotient, n, count, polys, lens, coeffs, point, plan)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_open_fold: ") + why);
    if (plan.empty() && !(on_device && quotient)) {  // the zero combination, nothing to write on a device
        if (quotient) memset(quotient, 0, sizeof(fr_mem_t) * n);
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t));
        return ok();
    }
    const void* anchor = quotient ? quotient : (const void*)plan[0].t.p[0];
    API_BEGIN_DEV(device_for(anchor, on_device ? 1 : 0))
    fr_mem_t* dq = (fr_mem_t*)quotient;
    if (on_device) {
        for (size_t k = 0; k < count; k++)
            if (lens[k]) fr_same_device(c, polys[k], "fr_open_fold: an operand lives on another device than the quotient (or the first operand)");
    } else {
        // host operands: one lane buffer holds the quotient and, behind it, every operand; one upload each, one download
        size_t total = quotient ? n : 0;
        for (size_t k = 0; k < count; k++) total += lens[k];
        c.poly[0].ensure(sizeof(fr_mem_t) * total);
        fr_mem_t* next = c.poly[0].as<fr_mem_t>();
        if (quotient) dq = next, next += n;
        std::vector<const fr_mem_t*> staged(count, nullptr);
        for (size_t k = 0; k < count; k++) {
            if (!lens[k]) continue;
            HIP_TRY(hipMemcpyAsync(next, polys[k], sizeof(fr_mem_t) * lens[k], hipMemcpyHostToDevice, c.stream));
            staged[k] = next;
            next += lens[k];
        }
        for (fr_lincomb_launch_t& L : plan)
            for (int m = 0; m < L.t.count; m++) L.t.p[m] = L.src[m] < 0 ? dq : staged[(size_t)L.src[m]];
    }
    if (plan.empty()) {  // device quotient of the zero combination
        HIP_TRY(hipMemsetAsync(dq, 0, sizeof(fr_mem_t) * n, c.stream));
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t));
    } else {
        const fr_mem_t* dres = fr_open_run(c, dq, n, fr_mem_from_host(point), plan);
        if (dq) fr_finish_out(c, dq, quotient, n, on_device);
        // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the value is there on return
        if (remainder) c.host_result(remainder, dres, sizeof(fr_mem_t), on_device != 0);
    }
    fr_call_done(c, on_device);
    API_END
}
// what the call launches for n coefficients when a quotient is wanted: out5 = {route (1: scan, 0: chunk recursion), coefficients per thread C,
// workgroups of the fused launches, operands per table (FR_LINCOMB_CHUNK), terms of the fused sweep at most (FR_OPEN_FUSE)}.  Without a
// quotient the route is always 0.
int snarkvm_hip_selftest_fr_open_fold_geometry(size_t n, uint32_t* out5) {
    if (!out5) return -1;
    const fr_open_geometry_t g = fr_open_geometry(n ? n : 1, true);
    out5[0] = (uint32_t)g.route, out5[1] = g.C, out5[2] = (uint32_t)g.blocks, out5[3] = FR_LINCOMB_CHUNK, out5[4] = FR_OPEN_FUSE;
    return 0;
}
// The same call on host memory with the CPU in the kernels' place, over a GIVEN geometry: the same plan, every launch a loop over its threads
// through the kernels' own per-thread routines, a workgroup's LDS exchanges as loops over its threads.
//   route 1 (needs a quotient): workgroups of HORNER2_B threads, C >= 1 coefficients per thread, ceil(n / (HORNER2_B C)) <= blocks <= 257
//   route 0: chunks of C >= 2 coefficients at every level, blocks = the workgroups of 256 threads of level 0 = ceil(ceil(n / C) / 256)
// 0, or -1 when the arguments or the geometry are refused.
int snarkvm_hip_selftest_fr_open_fold(void* quotient, void* remainder, size_t n, size_t count, const void* const* polys, const size_t* lens, const void* coeffs,
                                      const void* point, int route, uint32_t C, uint32_t blocks) {
    if (n == 0) {
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t));
        return 0;
    }
    std::vector<fr_lincomb_launch_t> plan;
    if (fr_open_plan(quotient, n, count, polys, lens, coeffs, point, plan)) return -1;
    if (route == 1) {
        if (!quotient || C < 1 || blocks > 257 || (size_t)blocks * HORNER2_B * C < n || (n - 1) / C > 0xFFFFFFFFull) return -1;
    } else if (route == 0) {
        if (C < 2 || (size_t)blocks != ((n + C - 1) / C + 255) / 256) return -1;
    } else {
        return -1;
    }
    fr_mem_t* q = (fr_mem_t*)quotient;
    fr_mem_t res;
    fr_t::zero().store(&res);
    if (plan.empty()) {
        if (q) memset(q, 0, sizeof(fr_mem_t) * n);
        if (remainder) memcpy(remainder, &res, sizeof res);
        return 0;
    }
    if (q)
        for (size_t j = 0; j + 1 < plan.size(); j++)
            for (size_t i = 0; i < n; i++) fr_lincomb_at(plan[j].t, i).store(&q[i]);
    const fr_mem_t z = fr_mem_from_host(point);
    const fr_t m = fr_t::load(&z).from_mem_mont();
    if (route == 1) {
        const uint32_t B = HORNER2_B;
        // fr_horner2_tables_kernel: step[j] = m^(C 2^j), pw[j] = m^(C j), pwB[j] = m^(256 C j)
        const fr_t mC = m.pow_u64(C), mB = mC.pow_u64(B);
        std::vector<fr_t> step(8), pw(B + 1), pwB(B);
        for (uint32_t t = 0; t < B; t++) pw[t] = mC.pow_u64(t), pwB[t] = mB.pow_u64(t);
        pw[B] = mB;
        for (uint32_t j = 0; j < 8; j++) step[j] = mC.pow_u64(1u << j);
        // up: hs and bv pass through memory, as on the device
        std::vector<fr_mem_t> hs((size_t)blocks * B), bv(blocks);
        for (uint32_t b = 0; b < blocks; b++) {
            std::vector<fr_t> h(B);
            for (uint32_t t = 0; t < B; t++) {
                const size_t lo0 = ((size_t)b * B + t) * C, lo = lo0 < n ? lo0 : n, hi = lo + C < n ? lo + C : n;
                h[t] = fr_open_up_chunk(plan.back().t, q, m, lo, hi);
            }
            for (int j = 0; j < 8; j++) {
                const std::vector<fr_t> sh = h;  // what the workgroup put into LDS before the barrier
                for (uint32_t t = 0; t + (1u << j) < B; t++) h[t] = fr_open_scan_step(sh[t], step[j], sh[t + (1u << j)]);
            }
            for (uint32_t t = 0; t < B; t++) h[t].store(&hs[(size_t)b * B + t]);
            h[0].store(&bv[b]);
        }
        for (uint32_t b = 0; b < blocks; b++) {
            std::vector<fr_t> term(B, fr_t::zero());
            for (uint32_t t = 0; t < B; t++)
                if (b + 1 + t < blocks) term[t] = fr_open_carry_term(pwB[t], fr_t::load(&bv[b + 1 + t]));
            for (uint32_t off = B / 2; off >= 1; off >>= 1) {
                const std::vector<fr_t> sh = term;
                for (uint32_t t = 0; t < off; t++) term[t] = sh[t] + sh[t + off];
            }
            const fr_t carry = term[0];
            for (uint32_t t = 0; t < B; t++) {
                const size_t lo = ((size_t)b * B + t) * C;
                if (lo >= n) continue;
                const size_t hi = lo + C < n ? lo + C : n;
                fr_t h = fr_open_thread_carry(pw[B - 1 - t], carry);
                if (t + 1 < B) h = h + fr_t::load(&hs[(size_t)b * B + t + 1]);
                h = fr_open_down_chunk(q, m, h, lo, hi);
                if (lo == 0) h.store(&res);
            }
        }
    } else {
        const std::vector<size_t> sizes = fr_open_levels(n, C);
        const int top = (int)sizes.size() - 1;
        std::vector<fr_t> mult(top + 1);  // fr_horner_multipliers_kernel: mult[k] = m^(C^k), through memory form
        {
            fr_t p = m;
            for (int k = 0; k <= top; k++) {
                fr_mem_t mm;
                p.to_mem_mont().store(&mm);
                mult[k] = fr_t::load(&mm).from_mem_mont();
                p = p.pow_u64(C);
            }
        }
        const auto chunk_hi = [&](size_t t, size_t cur) { return (t + 1) * (size_t)C < cur ? (t + 1) * (size_t)C : cur; };
        // level k >= 1 of one up sweep; -> the levels' values, cv[top] the single top value
        const auto up_from = [&](const fr_lincomb_t& tb, fr_mem_t* qq) {
            std::vector<std::vector<fr_mem_t>> cv(top + 1);
            cv[1].resize(sizes[1]);
            for (size_t t = 0; t < sizes[1]; t++) fr_open_up_chunk(tb, qq, mult[0], t * C, chunk_hi(t, n)).store(&cv[1][t]);
            for (int k = 1; k < top; k++) {
                cv[k + 1].resize(sizes[k + 1]);
                for (size_t t = 0; t < sizes[k + 1]; t++) {  // fr_horner_up_kernel
                    fr_t acc = fr_t::zero();
                    for (size_t i = chunk_hi(t, sizes[k]); i-- > t * C;) acc = fr_t::load(&cv[k][i]) + mult[k] * acc;
                    acc.store(&cv[k + 1][t]);
                }
            }
            return cv;
        };
        if (!q) {
            fr_t s = fr_t::zero();
            for (size_t j = 0; j < plan.size(); j++) {
                const fr_t v = fr_t::load(&up_from(plan[j].t, nullptr)[top][0]);
                if (plan.size() == 1)
                    v.store(&res);
                else
                    s = s + v;
            }
            if (plan.size() > 1) s.store(&res);
        } else {
            std::vector<std::vector<fr_mem_t>> cv = up_from(plan.back().t, q);
            for (int k = top - 1; k >= 1; k--)
                for (size_t t = 0; t < sizes[k + 1]; t++) {  // fr_horner_down_kernel, shift 0, in place
                    fr_t acc = t + 1 < sizes[k + 1] ? fr_t::load(&cv[k + 1][t + 1]) : fr_t::zero();
                    for (size_t i = chunk_hi(t, sizes[k]); i-- > t * C;) {
                        acc = fr_t::load(&cv[k][i]) + mult[k] * acc;
                        acc.store(&cv[k][i]);
                    }
                }
            for (size_t t = 0; t < sizes[1]; t++) {
                const fr_t h_hi = t + 1 < sizes[1] ? fr_t::load(&cv[1][t + 1]) : fr_t::zero();
                const fr_t h = fr_open_down_chunk(q, mult[0], h_hi, t * C, chunk_hi(t, n));
                if (t == 0) h.store(&res);
            }
        }
    }
    if (remainder) memcpy(remainder, &res, sizeof res);
    return 0;
}

// ---- selector fold: Varuna round 3 (poly.hip.h: fr_selector_fold_kernel) ---------------------------------------------------
// What the device call and its host replay share: validation, the member tables and the split into launches.  src[m]: the caller's index
// of table entry m (its pointers are bound later: to the caller's memory, or to the staged copies).
static void fr_same_device(lane_t& c, const void* p, const char* what);
static constexpr size_t FR_SELECTOR_LEN_MAX =(size_t)1 << 29, FR_SELECTOR_TARGET_MAX = (size_t)1 << 28;
struct fr_selector_launch_t {
    fr_selector_t t;
    size_t src[FR_SELECTOR_CHUNK];
};
struct fr_selector_plan_t {
    std::vector<fr_selector_launch_t> launches;
    bool want_h = false, want_xg = false, want_sums = false;
    uint32_t h_len = 0, N = 0, span = 0, threads = 0;  // span: the indices of xg the fold itself writes (the tile kernel the rest)
};
static fr_t fr_from_u64(uint64_t x) {
    const fr_t two32 = fr_t::from_u32(65536).sqr();
    return fr_t::from_u32((uint32_t)(x >> 32)) * two32 + fr_t::from_u32((uint32_t)x);
}
static size_t fr_gcd(size_t a, size_t b) {
    while (b) {
        const size_t r = a % b;
        a = b, b = r;
    }
    return a;
}
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  A plan without
// launches: nothing is wanted.
static const char* fr_selector_plan(const void* h_out, size_t h_len, const void* xg_out, size_t target_size, const void* sums, size_t count, const void* const* polys,
                                    const size_t* lens, const size_t* src_sizes, const void* multipliers, fr_selector_plan_t& plan) {
    if (count > 65535) return "more than 65535 members";
    if (count && (!polys || !lens || !src_sizes || !multipliers)) return "missing argument";
    if (h_out && h_len > FR_SELECTOR_LEN_MAX) return "h_len above 2^29";
    if (xg_out && (target_size == 0 || target_size > FR_SELECTOR_TARGET_MAX)) return "target_size is 0 or above 2^28";
    size_t need = 0, period = 1;
    for (size_t k = 0; k < count; k++) {
        const size_t n = src_sizes[k], L = lens[k];
        if (!n) return "an empty source domain";
        if (L > FR_SELECTOR_LEN_MAX) return "a member longer than 2^29";
        if (L && !polys[k]) return "null member of non-zero length";
        if (xg_out && target_size % n) return "a source domain does not divide target_size";
        if (L > n && L - n > need) need = L - n;
        if (xg_out && L) period = period / fr_gcd(period, n) * n;  // every n_k divides target_size: so does the period
    }
    if (h_out && h_len < need) return "h_len is shorter than the longest quotient";
    {  // no output may overlap an operand or another output; sorted by address, an overlap shows against the furthest end seen so far
        struct range_t {
            const uint8_t* p;
            size_t bytes;
            bool out;
        };
        std::vector<range_t> rs;
        if (h_out && h_len) rs.push_back({(const uint8_t*)h_out, sizeof(fr_mem_t) * h_len, true});
        if (xg_out) rs.push_back({(const uint8_t*)xg_out, sizeof(fr_mem_t) * target_size, true});
        if (sums && count) rs.push_back({(const uint8_t*)sums, sizeof(fr_mem_t) * count, true});
        for (size_t k = 0; k < count; k++)
            if (lens[k]) rs.push_back({(const uint8_t*)polys[k], sizeof(fr_mem_t) * lens[k], false});
        std::sort(rs.begin(), rs.end(), [](const range_t& x, const range_t& y) { return x.p < y.p; });
        const uint8_t *end_any = nullptr, *end_out = nullptr;
        for (const range_t& r : rs) {
            if (r.p < (r.out ? end_any : end_out)) return "an output overlaps an operand or another output";
            if (r.p + r.bytes > end_any) end_any = r.p + r.bytes;
            if (r.out && r.p + r.bytes > end_out) end_out = r.p + r.bytes;
        }
    }
    plan.want_h = h_out && h_len, plan.want_xg = xg_out != nullptr, plan.want_sums = sums && count;
    if (!plan.want_h && !plan.want_xg && !plan.want_sums) return nullptr;
    plan.h_len = plan.want_h ? (uint32_t)h_len : 0;
    plan.N = plan.want_xg ? (uint32_t)target_size : 0;
    plan.span = plan.want_xg ? (FR_SELECTOR_TILE ? (uint32_t)period : plan.N) : 0;
    plan.threads = plan.h_len > plan.span ? plan.h_len : plan.span;
    if (!plan.threads) plan.threads = 1;
    std::vector<size_t> live;  // an empty member contributes nothing: it stays only where its sum (zero) is to be written
    for (size_t k = 0; k < count; k++)
        if (lens[k] || plan.want_sums) live.push_back(k);
    size_t at = 0;
    do {  // no member at all: one launch that writes the zeros
        fr_selector_launch_t L{};
        int m = 0;
        L.t.accumulate = at != 0;
        for (; m < FR_SELECTOR_CHUNK && at < live.size(); m++, at++) {
            const size_t k = live[at];
            const fr_mem_t mu_mem = fr_mem_from_host((const uint8_t*)multipliers + sizeof(fr_mem_t) * k);
            const fr_t mu = fr_t::load(&mu_mem).from_mem_mont(), ns = fr_from_u64((uint64_t)src_sizes[k]);
            L.src[m] = k;
            L.t.len[m] = (uint32_t)lens[k];
            L.t.n[m] = src_sizes[k] > ((size_t)1 << 30) ? (1u << 30) : (uint32_t)src_sizes[k];
            for (int l = 0; l < 9; l++) L.t.mu[m][l] = mu.v[l], L.t.ns[m][l] = ns.v[l];
        }
        L.t.count = m;
        plan.launches.push_back(L);
    } while (at < live.size());
    return nullptr;
}
// pointers of the tables: member k at polys[k], its sum at sums + k (nullptr: no sums)
static void fr_selector_bind(fr_selector_plan_t& plan, const fr_mem_t* const* polys, fr_mem_t* sums) {
    for (fr_selector_launch_t& L : plan.launches)
        for (int m = 0; m < L.t.count; m++) L.t.p[m] = polys[L.src[m]], L.t.sum[m] = sums ? sums + L.src[m] : nullptr;
}
RustError snarkvm_hip_fr_selector_fold(void* h_out, size_t h_len, void* xg_out, size_t target_size, void* sums, size_t count, const void* const* polys,
                                       const size_t* lens, const size_t* src_sizes, const void* multipliers, int on_device) {
    fr_selector_plan_t plan;
    if (const char* why = fr_selector_plan(h_out, h_len, xg_out, target_size, sums, count, polys, lens, src_sizes, multipliers, plan))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_selector_fold: ") + why);
    if (plan.launches.empty()) return ok();
    const void* first = plan.want_h ? h_out : (plan.want_xg ? xg_out : sums);
    API_BEGIN_DEV(device_for(first, on_device ? 1 : 0))
    fr_mem_t *dh = plan.want_h ? (fr_mem_t*)h_out : nullptr, *dxg = plan.want_xg ? (fr_mem_t*)xg_out : nullptr, *dsums = plan.want_sums ? (fr_mem_t*)sums : nullptr;
    std::vector<const fr_mem_t*> members(count, nullptr);
    if (on_device) {
        const char* why = "fr_selector_fold: the outputs and members live on different devices";
        fr_same_device(c, dh, why), fr_same_device(c, dxg, why), fr_same_device(c, dsums, why);
        for (size_t k = 0; k < count; k++) {
            if (lens[k]) fr_same_device(c, polys[k], why);
            members[k] = (const fr_mem_t*)polys[k];
        }
    } else {
        // host operands: one lane buffer holds the outputs and, behind them, every member; one upload each, one download per output
        size_t total = (size_t)plan.h_len + plan.N + (plan.want_sums ? count : 0);
        for (size_t k = 0; k < count; k++) total += lens[k];
        c.poly[0].ensure(sizeof(fr_mem_t) * total);
        fr_mem_t* next = c.poly[0].as<fr_mem_t>();
        if (plan.want_h) dh = next, next += plan.h_len;
        if (plan.want_xg) dxg = next, next += plan.N;
        if (plan.want_sums) dsums = next, next += count;
        for (size_t k = 0; k < count; k++) {
            if (!lens[k]) continue;
            HIP_TRY(hipMemcpyAsync(next, polys[k], sizeof(fr_mem_t) * lens[k], hipMemcpyHostToDevice, c.stream));
            members[k] = next;
            next += lens[k];
        }
    }
    fr_selector_bind(plan, members.data(), dsums);
    for (const fr_selector_launch_t& L : plan.launches)
        hipLaunchKernelGGL(fr_selector_fold_kernel, dim3(fr_grid(plan.threads)), dim3(256), 0, c.stream, dh, plan.h_len, dxg, plan.span, plan.threads, L.t);
    if (plan.span < plan.N) hipLaunchKernelGGL(fr_tile_kernel, dim3(fr_grid(plan.N - plan.span)), dim3(256), 0, c.stream, dxg, plan.span, plan.N);
    HIP_TRY(hipGetLastError());
    if (plan.want_h) fr_finish_out(c, dh, h_out, plan.h_len, on_device);
    if (plan.want_xg) fr_finish_out(c, dxg, xg_out, plan.N, on_device);
    if (plan.want_sums) fr_finish_out(c, dsums, sums, count, on_device);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernels' place: the same plan, every launch a loop over i through the kernel's own
// per-index routine, then the tiling.  0, or -1 when the plan refuses the arguments.
int snarkvm_hip_selftest_fr_selector_fold(void* h_out, size_t h_len, void* xg_out, size_t target_size, void* sums, size_t count, const void* const* polys,
                                          const size_t* lens, const size_t* src_sizes, const void* multipliers) {
    fr_selector_plan_t plan;
    if (fr_selector_plan(h_out, h_len, xg_out, target_size, sums, count, polys, lens, src_sizes, multipliers, plan)) return -1;
    if (plan.launches.empty()) return 0;
    fr_mem_t *h = plan.want_h ? (fr_mem_t*)h_out : nullptr, *xg = plan.want_xg ? (fr_mem_t*)xg_out : nullptr;
    fr_selector_bind(plan, (const fr_mem_t* const*)polys, plan.want_sums ? (fr_mem_t*)sums : nullptr);
    for (const fr_selector_launch_t& L : plan.launches)
        for (uint32_t i = 0; i < plan.threads; i++) fr_selector_at(L.t, h, plan.h_len, xg, plan.span, i);
    for (uint32_t i = plan.span; i < plan.N; i++) fr_tile_at(xg, plan.span, i);
    return 0;
}

// ---- round 1: the evaluations of w on the variable domain (poly.hip.h: fr_witness_evals_kernel) ------------------------------------------
static constexpr size_t FR_ROUND12_N_MAX = (size_t)1 << 28;
static bool fr_ranges_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uint8_t *x = (const uint8_t*)p, *y = (const uint8_t*)q;
    return p && q && np && nq && x < y + sizeof(fr_mem_t) * nq && y < x + sizeof(fr_mem_t) * np;
}
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.
static const char* fr_witness_check(const void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size) {
    if (input_size == 0) return "input_size is 0";
    if (n % input_size) return "input_size does not divide n";
    if (n > FR_ROUND12_N_MAX) return "n above 2^28";
    if (w_len > n - input_size) return "w is longer than n - input_size";
    if (n && (!out || !x_evals)) return "null vector of non-zero length";
    if (w_len && !w) return "null witness of non-zero length";
    if ((out != x_evals && fr_ranges_overlap(out, n, x_evals, n)) || fr_ranges_overlap(out, n, w, w_len)) return "out overlaps an operand (only out == x_evals is allowed)";
    return nullptr;
}
RustError snarkvm_hip_fr_witness_evals(void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size, int on_device) {
    if (const char* why = fr_witness_check(out, n, w, w_len, x_evals, input_size)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_witness_evals: ") + why);
    if (n == 0) return ok();
    API_BEGIN_DEV(device_for(out, on_device ? 1 : 0))
    if (on_device) {
        const char* why = "fr_witness_evals: the operands live on different devices";
        fr_same_device(c, x_evals, why);
        if (w_len) fr_same_device(c, w, why);
    }
    const fr_mem_t* dw = fr_stage_in(c, 0, w_len ? w : nullptr, w_len, on_device);
    const fr_mem_t* dx = fr_stage_in(c, 1, x_evals, n, on_device);
    fr_mem_t* dout = fr_stage_out(c, 3, out, n, on_device);
    hipLaunchKernelGGL(fr_witness_evals_kernel, dim3(fr_grid(n)), dim3(256), 0, c.stream, dout, (uint32_t)n, dw, (uint32_t)w_len, dx, (uint32_t)(n / input_size));
    HIP_TRY(hipGetLastError());
    fr_finish_out(c, dout, out, n, on_device);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernel's place, through the kernel's own per-index routine.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_witness_evals(void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size) {
    if (fr_witness_check(out, n, w, w_len, x_evals, input_size)) return -1;
    for (size_t k = 0; k < n; k++) fr_witness_at((fr_mem_t*)out, (const fr_mem_t*)w, (uint32_t)w_len, (const fr_mem_t*)x_evals, (uint32_t)(n / input_size), (uint32_t)k);
    return 0;
}

// ---- round 2: the rowcheck fold (poly.hip.h: fr_rowcheck_fold_kernel) ------------------------------------------------------------------------
// What the device call and its host replay share: validation, the member tables and the split into launches.  Launch j holds the members
// first .. first + t.count - 1 of the caller's order (its pointers are bound later: to the caller's memory, or to the staged copies).
struct fr_rowcheck_launch_t {
    fr_rowcheck_t t;
    size_t first;
};
struct fr_rowcheck_plan_t {
    std::vector<fr_rowcheck_launch_t> launches;
    int mode = 0;  // FR_ROWCHECK_FOLD | FR_ROWCHECK_CHECK: what is wanted
};
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  A plan without launches:
// no kernel is needed (n == 0, or nothing is wanted).
static const char* fr_rowcheck_plan(const void* out, const uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c,
                                    const void* multipliers, fr_rowcheck_plan_t& plan) {
    if (n > FR_ROUND12_N_MAX) return "n above 2^28";
    if (count > 65535) return "more than 65535 members";
    if (count && (!a || !b || !c || (out && !multipliers))) return "missing argument";
    if (n)
        for (size_t k = 0; k < count; k++) {
            if (!a[k] || !b[k] || !c[k]) return "null member";
            if (fr_ranges_overlap(out, n, a[k], n) || fr_ranges_overlap(out, n, b[k], n) || fr_ranges_overlap(out, n, c[k], n)) return "out overlaps a member";
        }
    plan.mode = (out ? FR_ROWCHECK_FOLD : 0) | (violations && count ? FR_ROWCHECK_CHECK : 0);
    if (!n || !plan.mode) return nullptr;
    size_t at = 0;
    do {  // no member at all: one launch that writes the zeros
        fr_rowcheck_launch_t L{};
        L.first = at, L.t.accumulate = at != 0;
        int m = 0;
        for (; m < FR_ROWCHECK_CHUNK && at < count; m++, at++) {
            if (!out) continue;
            const fr_mem_t mu_mem = fr_mem_from_host((const uint8_t*)multipliers + sizeof(fr_mem_t) * at);
            const fr_t mu = fr_t::load(&mu_mem).from_mem_mont(), mu_fix = mu.from_mem_mont(), neg = mu.neg();
            for (int l = 0; l < 9; l++) L.t.mu[m][l] = mu_fix.v[l], L.t.nmu[m][l] = neg.v[l];
        }
        L.t.count = m;
        plan.launches.push_back(L);
    } while (at < count);
    return nullptr;
}
// pointers of the tables: member k's vectors at a[k], b[k], c[k]
static void fr_rowcheck_bind(fr_rowcheck_plan_t& plan, const fr_mem_t* const* a, const fr_mem_t* const* b, const fr_mem_t* const* c) {
    for (fr_rowcheck_launch_t& L : plan.launches)
        for (int m = 0; m < L.t.count; m++) L.t.a[m] = a[L.first + m], L.t.b[m] = b[L.first + m], L.t.c[m] = c[L.first + m];
}
RustError snarkvm_hip_fr_rowcheck_fold(void* out, uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c3,
                                       const void* multipliers, int on_device) {
    fr_rowcheck_plan_t plan;
    if (const char* why = fr_rowcheck_plan(out, violations, n, count, a, b, c3, multipliers, plan)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_rowcheck_fold: ") + why);
    if (plan.launches.empty()) {
        if (violations && count) memset(violations, 0, sizeof(uint64_t) * count);  // n == 0: nothing is violated
        return ok();
    }
    API_BEGIN_DEV(device_for(out ? out : a[0], on_device ? 1 : 0))
    fr_mem_t* dout = (fr_mem_t*)out;
    std::vector<const fr_mem_t*> members[3];
    const void* const* given[3] = {a, b, c3};
    for (auto& v : members) v.assign(count, nullptr);
    if (on_device) {
        const char* why = "fr_rowcheck_fold: out and the members live on different devices";
        for (int j = 0; j < 3; j++)
            for (size_t k = 0; k < count; k++) fr_same_device(c, given[j][k], why), members[j][k] = (const fr_mem_t*)given[j][k];
    } else {
        // host operands: one lane buffer holds out and, behind it, every member vector; one upload each, one download
        c.poly[0].ensure(sizeof(fr_mem_t) * n * ((out ? 1 : 0) + 3 * count));
        fr_mem_t* next = c.poly[0].as<fr_mem_t>();
        if (out) dout = next, next += n;
        for (int j = 0; j < 3; j++)
            for (size_t k = 0; k < count; k++) {
                HIP_TRY(hipMemcpyAsync(next, given[j][k], sizeof(fr_mem_t) * n, hipMemcpyHostToDevice, c.stream));
                members[j][k] = next, next += n;
            }
    }
    fr_rowcheck_bind(plan, members[0].data(), members[1].data(), members[2].data());
    unsigned long long* dviol = nullptr;
    if (plan.mode & FR_ROWCHECK_CHECK) {  // workspace: one 64-bit counter per member
        c.poly[4].ensure(sizeof(unsigned long long) * count);
        dviol = c.poly[4].as<unsigned long long>();
        HIP_TRY(hipMemsetAsync(dviol, 0, sizeof(unsigned long long) * count, c.stream));
    }
    const dim3 grid(fr_grid(n)), block(256);
    for (const fr_rowcheck_launch_t& L : plan.launches) {
        unsigned long long* v = dviol ? dviol + L.first : nullptr;
        if (plan.mode == FR_ROWCHECK_FOLD)
            hipLaunchKernelGGL(fr_rowcheck_fold_kernel<FR_ROWCHECK_FOLD>, grid, block, 0, c.stream, dout, v, (uint32_t)n, L.t);
        else if (plan.mode == FR_ROWCHECK_CHECK)
            hipLaunchKernelGGL(fr_rowcheck_fold_kernel<FR_ROWCHECK_CHECK>, grid, block, 0, c.stream, dout, v, (uint32_t)n, L.t);
        else
            hipLaunchKernelGGL(fr_rowcheck_fold_kernel<FR_ROWCHECK_FOLD | FR_ROWCHECK_CHECK>, grid, block, 0, c.stream, dout, v, (uint32_t)n, L.t);
    }
    HIP_TRY(hipGetLastError());
    if (out) fr_finish_out(c, dout, out, n, on_device);
    // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the counts are there on return
    if (dviol) c.host_result(violations, dviol, sizeof(uint64_t) * count, on_device != 0);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernel's place: the same plan, every launch a loop over i through the kernel's own
// per-index routine, the bits it returns counted per member.  0, or -1 when the plan refuses the arguments.
int snarkvm_hip_selftest_fr_rowcheck_fold(void* out, uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c3,
                                          const void* multipliers) {
    fr_rowcheck_plan_t plan;
    if (fr_rowcheck_plan(out, violations, n, count, a, b, c3, multipliers, plan)) return -1;
    const bool check = violations && count;
    if (check) memset(violations, 0, sizeof(uint64_t) * count);
    if (plan.launches.empty()) return 0;
    fr_rowcheck_bind(plan, (const fr_mem_t* const*)a, (const fr_mem_t* const*)b, (const fr_mem_t* const*)c3);
    for (const fr_rowcheck_launch_t& L : plan.launches)
        for (size_t i = 0; i < n; i++) {
            uint32_t bad;
            if (plan.mode == FR_ROWCHECK_FOLD)
                bad = fr_rowcheck_at<FR_ROWCHECK_FOLD>(L.t, (fr_mem_t*)out, (uint32_t)i);
            else if (plan.mode == FR_ROWCHECK_CHECK)
                bad = fr_rowcheck_at<FR_ROWCHECK_CHECK>(L.t, (fr_mem_t*)out, (uint32_t)i);
            else
                bad = fr_rowcheck_at<FR_ROWCHECK_FOLD | FR_ROWCHECK_CHECK>(L.t, (fr_mem_t*)out, (uint32_t)i);
            for (int m = 0; bad; m++, bad >>= 1) violations[L.first + m] += bad & 1;
        }
    return 0;
}
// the members per launch and per Montgomery reduction the library was built with
int snarkvm_hip_selftest_fr_rowcheck_geometry(uint32_t* out2) {
    if (!out2) return -1;
    out2[0] = FR_ROWCHECK_CHUNK, out2[1] = FR_ROWCHECK_G;
    return 0;
}

// ---- reductions (poly.hip.h: fr_reduce_kernel, fr_support_kernel) ---------------------------------------------------------------
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device
static const char* fr_reduce_check(int op, const void* result, const void* a, const void* b, size_t n) {
    if (op != FR_REDUCE_SUM && op != FR_REDUCE_DOT) return "unknown op";
    if (!result) return "null result";
    if (n && !a) return "null operand a";
    if (n && op == FR_REDUCE_DOT && !b) return "null operand b of an inner product";
    return nullptr;
}
// check_strided without a lane: the same refusal, before any device is needed
static bool fr_strided_refused(size_t n, size_t count, size_t stride, RustError& err) {
    try {
        check_strided(n, count, stride, 1, "fr_reduce");
    } catch (const hip_failure& f) {
        err = from_failure(f);
        return true;
    }
    return false;
}
static void fr_same_device(lane_t& c, const void* p, const char* what) {
    if (p && g_rt.devs[device_for(p, 1)]->physical != c.dev->physical) throw hip_failure{hipErrorInvalidValue, what, __LINE__};
}
static RustError fr_reduce_impl(int op, void* results, const void* a, const void* b, size_t n, int on_device, size_t count, size_t stride, int b_shared) {
    if (count == 0) return ok();
    if (const char* why = fr_reduce_check(op, results, a, b, n)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_reduce: ") + why);
    RustError refused = ok();
    if (fr_strided_refused(n, count, stride, refused)) return refused;
    if (n == 0) {
        memset(results, 0, sizeof(fr_mem_t) * count);
        return ok();
    }
    API_BEGIN_DEV(device_for(a, on_device ? 1 : 0))
    const bool dot = op == FR_REDUCE_DOT;
    if (on_device && dot) fr_same_device(c, b, "fr_reduce: b lives on another device than a");
    const fr_mem_t* da = fr_stage_in(c, 0, a, n, on_device);
    const fr_mem_t* db = !dot ? nullptr : ((b == a && !on_device) ? da : fr_stage_in(c, 1, b, n, on_device));
    const unsigned blocks = fr_reduce_blocks(n);
    // workspace: count x blocks partials, then the count results
    c.poly[4].ensure(sizeof(fr_mem_t) * count * ((size_t)blocks + 1));
    fr_mem_t* parts = c.poly[4].as<fr_mem_t>();
    fr_mem_t* dres = parts + count * (size_t)blocks;
    const dim3 grid(blocks, (unsigned)count);
    if (dot)
        hipLaunchKernelGGL(fr_reduce_kernel<FR_REDUCE_DOT>, grid, dim3(FR_REDUCE_B), 0, c.stream, da, db, n, stride, b_shared ? (size_t)0 : stride, parts);
    else
        hipLaunchKernelGGL(fr_reduce_kernel<FR_REDUCE_SUM>, grid, dim3(FR_REDUCE_B), 0, c.stream, da, db, n, stride, (size_t)0, parts);
    hipLaunchKernelGGL(fr_reduce_final_kernel, dim3(1, (unsigned)count), dim3(FR_REDUCE_B), 0, c.stream, op, (const fr_mem_t*)parts, (size_t)blocks, dres);
    HIP_TRY(hipGetLastError());
    // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the value is there on return
    c.host_result(results, dres, sizeof(fr_mem_t) * count, on_device != 0);
    fr_call_done(c, on_device);
    API_END
}
RustError snarkvm_hip_fr_reduce(int op, void* result, const void* a, const void* b, size_t n, int on_device) {
    return fr_reduce_impl(op, result, a, b, n, on_device, 1, 0, 0);
}
RustError snarkvm_hip_fr_reduce_strided(int op, void* results, const void* a, const void* b, size_t n, size_t count, size_t stride, int b_shared) {
    return fr_reduce_impl(op, results, a, b, n, 1, count, stride, b_shared);
}
static RustError fr_support_impl(uint64_t* out, const void* v, size_t n, int on_device, size_t count, size_t stride) {
    if (count == 0) return ok();
    if (!out || (n && !v)) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_support: missing argument");
    RustError refused = ok();
    if (fr_strided_refused(n, count, stride, refused)) return refused;
    if (n == 0) {
        memset(out, 0, 3 * sizeof(uint64_t) * count);
        return ok();
    }
    API_BEGIN_DEV(device_for(v, on_device ? 1 : 0))
    const fr_mem_t* dv = fr_stage_in(c, 0, v, n, on_device);
    const unsigned blocks = fr_reduce_blocks(n);
    c.poly[4].ensure(3 * sizeof(uint64_t) * count * ((size_t)blocks + 1));
    uint64_t* parts = c.poly[4].as<uint64_t>();
    uint64_t* dres = parts + 3 * count * (size_t)blocks;
    hipLaunchKernelGGL(fr_support_kernel, dim3(blocks, (unsigned)count), dim3(FR_REDUCE_B), 0, c.stream, dv, n, stride, parts);
    hipLaunchKernelGGL(fr_support_final_kernel, dim3(1, (unsigned)count), dim3(FR_REDUCE_B), 0, c.stream, (const uint64_t*)parts, (size_t)blocks, n, dres);
    HIP_TRY(hipGetLastError());
    c.host_result(out, dres, 3 * sizeof(uint64_t) * count, on_device != 0);
    fr_call_done(c, on_device);
    API_END
}
RustError snarkvm_hip_fr_support(uint64_t* out3, const void* v, size_t n, int on_device) { return fr_support_impl(out3, v, n, on_device, 1, 0); }
RustError snarkvm_hip_fr_support_strided(uint64_t* out, const void* v, size_t n, size_t count, size_t stride) { return fr_support_impl(out, v, n, 1, count, stride); }

// The two passes on host memory with the CPU in the kernels' place, over a GIVEN geometry (blocks workgroups of `threads` threads, threads = 64, 128
// or 256): every thread through the kernels' own per-thread routine, every tree level a loop over the lanes it exchanges between, the second launch
// with FR_REDUCE_B threads.  0, or -1 when the arguments are refused.
static bool fr_reduce_geometry_ok(uint32_t blocks, uint32_t threads) { return blocks >= 1 && (threads == 64 || threads == 128 || threads == 256); }
// the butterflies of fr_block_sum / fr_block_support over `vals` (one per thread): lanes l and l ^ off meet, then the waves' values
extern "C++" {
template <class T, class Combine>
static T fr_block_tree_host(std::vector<T> vals, const T& identity, Combine combine) {
    const size_t nw = vals.size() / 64;
    auto butterfly = [&](T* lanes, size_t from) {
        for (size_t off = from; off >= 1; off >>= 1) {
            T next[64];
            for (size_t l = 0; l < 64; l++) next[l] = combine(lanes[l], lanes[l ^ off]);
            std::copy(next, next + 64, lanes);
        }
    };
    for (size_t w = 0; w < nw; w++) butterfly(vals.data() + 64 * w, 32);
    if (nw == 1) return vals[0];
    T u[64];
    for (size_t l = 0; l < 64; l++) u[l] = l < nw ? vals[64 * l] : identity;
    butterfly(u, nw >> 1);
    return u[0];
}
}  // extern "C++"
int snarkvm_hip_selftest_fr_reduce(int op, void* out, const void* a, const void* b, size_t n, uint32_t blocks, uint32_t threads) {
    if (fr_reduce_check(op, out, a, b, n) || !fr_reduce_geometry_ok(blocks, threads)) return -1;
    const fr_mem_t *pa = (const fr_mem_t*)a, *pb = (const fr_mem_t*)b;
    const auto add = [](const fr_t& x, const fr_t& y) { return x + y; };
    std::vector<fr_mem_t> parts(blocks);
    for (uint32_t x = 0; x < blocks; x++) {
        std::vector<fr_t> vals(threads);
        for (uint32_t t = 0; t < threads; t++) {
            const size_t first = (size_t)x * threads + t, step = (size_t)blocks * threads;
            vals[t] = op == FR_REDUCE_DOT ? fr_reduce_thread<FR_REDUCE_DOT>(pa, pb, n, first, step) : fr_reduce_thread<FR_REDUCE_SUM>(pa, pb, n, first, step);
        }
        fr_block_tree_host(vals, fr_t::zero(), add).store(&parts[x]);
    }
    std::vector<fr_t> vals(FR_REDUCE_B);
    for (uint32_t t = 0; t < (uint32_t)FR_REDUCE_B; t++) vals[t] = fr_reduce_thread<FR_REDUCE_SUM>(parts.data(), nullptr, blocks, t, FR_REDUCE_B);
    fr_mem_t res;
    fr_reduce_finish(op, fr_block_tree_host(vals, fr_t::zero(), add)).store(&res);
    memcpy(out, &res, sizeof res);
    return 0;
}
int snarkvm_hip_selftest_fr_support(uint64_t* out3, const void* v, size_t n, uint32_t blocks, uint32_t threads) {
    if (!out3 || (n && !v) || !fr_reduce_geometry_ok(blocks, threads)) return -1;
    const fr_support_t id = fr_support_identity(n);
    std::vector<uint64_t> parts(3 * (size_t)blocks);
    for (uint32_t x = 0; x < blocks; x++) {
        std::vector<fr_support_t> vals(threads);
        for (uint32_t t = 0; t < threads; t++) vals[t] = fr_support_thread((const fr_mem_t*)v, n, (size_t)x * threads + t, (size_t)blocks * threads);
        const fr_support_t s = fr_block_tree_host(vals, id, fr_support_combine);
        parts[3 * x] = s.trimmed_len, parts[3 * x + 1] = s.leading_zeros, parts[3 * x + 2] = s.nonzero;
    }
    std::vector<fr_support_t> vals(FR_REDUCE_B);
    for (uint32_t t = 0; t < (uint32_t)FR_REDUCE_B; t++) vals[t] = fr_support_fold(parts.data(), blocks, n, t, FR_REDUCE_B);
    const fr_support_t s = fr_block_tree_host(vals, id, fr_support_combine);
    out3[0] = s.trimmed_len, out3[1] = s.leading_zeros, out3[2] = s.nonzero;
    return 0;
}
// what snarkvm_hip_fr_reduce / _fr_support launch for n elements: out4 = {workgroups, threads per workgroup, the cap on workgroups, the group size G
// of the inner product's sum_of_products}
int snarkvm_hip_selftest_fr_reduce_geometry(size_t n, uint32_t* out4) {
    if (!out4) return -1;
    out4[0] = fr_reduce_blocks(n), out4[1] = FR_REDUCE_B, out4[2] = FR_REDUCE_BLOCKS_MAX, out4[3] = FR_REDUCE_G;
    return 0;
}

// ---- sparse matrix times vector over a registered matrix (poly.hip.h: fr_spmv_seg_kernel, fr_spmv_fix_kernel) ----------------------
static constexpr size_t FR_SPMV_DIM_MAX = (size_t)1 << NTT_LG_MAX;  // rows, cols, n_out: the SRS maximum the transforms stop at
// nullptr, or why the CSR arrays are refused (hipErrorInvalidValue).  Needs no device and touches nothing: after it no index the kernels will
// ever see can point outside x (cols elements), vals or col_idx.
static const char* fr_spmv_matrix_check(size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals) {
    if (rows > FR_SPMV_DIM_MAX || cols > FR_SPMV_DIM_MAX) return "more than 2^28 rows or columns";
    if (!row_ptr) return "null row_ptr";
    if (row_ptr[0] != 0) return "row_ptr[0] != 0";
    for (size_t r = 0; r < rows; r++)
        if (row_ptr[r + 1] < row_ptr[r]) return "row_ptr decreases";
    const uint64_t nnz = row_ptr[rows];
    if (nnz > 0xFFFFFFFFull) return "more than 2^32 - 1 entries";
    if (nnz && (!col_idx || !vals)) return "null col_idx or vals of a matrix with entries";
    for (uint64_t k = 0; k < nnz; k++)
        if (col_idx[k] >= cols) return "a column index is not below cols";
    return nullptr;
}
// the work layout of a checked matrix for segments of at most `seg` entries -> number of partial-sum slots
static size_t fr_spmv_layout(size_t rows, const uint64_t* row_ptr, uint32_t seg, std::vector<fr_spmv_seg_t>& segs, std::vector<fr_spmv_fix_t>& fix) {
    size_t nparts = 0;
    for (size_t r = 0; r < rows; r++) {
        const uint64_t first = row_ptr[r], len = row_ptr[r + 1] - first;
        const uint64_t pieces = (len + seg - 1) / seg;
        if (pieces != 1) fix.push_back({(uint32_t)r, (uint32_t)nparts, (uint32_t)pieces, 0});
        for (uint64_t p = 0; p < pieces; p++) {
            const uint64_t at = p * seg;
            segs.push_back({(uint32_t)r, (uint32_t)(first + at), (uint32_t)(len - at < seg ? len - at : seg), pieces == 1 ? FR_SPMV_SOLE : (uint32_t)(nparts + p)});
        }
        if (pieces > 1) nparts += pieces;
    }
    return nparts;
}
}  // extern "C"
// one replica per logical device, like registered bases: ONE block holding vals | segment table | fix-up table | col_idx
struct snarkvm_hip_fr_matrix {
    size_t rows = 0, cols = 0, nnz = 0, nseg = 0, nfix = 0, nparts = 0;
    uint32_t seg = 0, width = 0;
    std::vector<uint8_t*> d;  // [logical device]
    size_t off_segs = 0, off_fix = 0, off_col = 0, bytes = 0;
    const fr_mem_t* vals(int dev) const { return (const fr_mem_t*)d[dev]; }
    const fr_spmv_seg_t* segs(int dev) const { return (const fr_spmv_seg_t*)(d[dev] + off_segs); }
    const fr_spmv_fix_t* fix(int dev) const { return (const fr_spmv_fix_t*)(d[dev] + off_fix); }
    const uint32_t* col(int dev) const { return (const uint32_t*)(d[dev] + off_col); }
    void free_all() {
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (size_t i = 0; i < d.size(); i++)
            if (d[i]) {
                (void)hipSetDevice(g_rt.devs[i]->physical);
                (void)hipFree(d[i]);  // waits for every stream of the device: nothing queued - an open scope's product included - can still use the block
                d[i] = nullptr;
            }
        (void)hipSetDevice(prev);
    }
};
template <int W>
static void fr_spmv_launch(lane_t& c, const snarkvm_hip_fr_matrix& h, int dev, const fr_mem_t* dx, size_t stride_x, fr_mem_t* dy, size_t stride_y, size_t n_out,
                           size_t count, fr_mem_t* parts) {
    const size_t per_block = FR_SPMV_B / W;
    if (h.nseg)
        hipLaunchKernelGGL(fr_spmv_seg_kernel<W>, dim3((unsigned)((h.nseg + per_block - 1) / per_block), (unsigned)count), dim3(FR_SPMV_B), 0, c.stream, h.segs(dev), h.nseg,
                           h.vals(dev), h.col(dev), dx, stride_x, dy, stride_y, parts, h.nparts);
    const size_t groups = h.nfix + (n_out - h.rows);
    if (groups)
        hipLaunchKernelGGL(fr_spmv_fix_kernel<W>, dim3((unsigned)((groups + per_block - 1) / per_block), (unsigned)count), dim3(FR_SPMV_B), 0, c.stream, h.fix(dev), h.nfix,
                           (const fr_mem_t*)parts, h.nparts, dy, stride_y, h.rows, n_out);
}
extern "C" {
RustError snarkvm_hip_fr_matrix_register(snarkvm_hip_fr_matrix_t** handle, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_matrix_register: null handle");
    *handle = nullptr;
    if (const char* why = fr_spmv_matrix_check(rows, cols, row_ptr, col_idx, vals)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_matrix_register: ") + why);
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_matrix> h(new snarkvm_hip_fr_matrix());
    std::vector<fr_spmv_seg_t> segs;
    std::vector<fr_spmv_fix_t> fix;
    h->rows = rows, h->cols = cols, h->nnz = (size_t)row_ptr[rows], h->seg = FR_SPMV_SEG;
    h->nparts = fr_spmv_layout(rows, row_ptr, h->seg, segs, fix);
    h->nseg = segs.size(), h->nfix = fix.size();
    h->width = fr_spmv_width(h->nnz, h->nseg);
    h->off_segs = sizeof(fr_mem_t) * h->nnz;
    h->off_fix = h->off_segs + sizeof(fr_spmv_seg_t) * h->nseg;
    h->off_col = h->off_fix + sizeof(fr_spmv_fix_t) * h->nfix;
    h->bytes = h->off_col + sizeof(uint32_t) * h->nnz;
    const int nd = g_rt.ndev();
    h->d.assign(nd, nullptr);
    try {
        std::vector<int> all;
        for (int d = 0; d < nd; d++) all.push_back(d);
        for_each_device(all, [&](int dev) {  // every device uploads its own replica
            lane_guard lg(dev);
            lane_t& c = lg.c();
            HIP_TRY(hipMalloc((void**)&h->d[dev], h->bytes ? h->bytes : 32));
            uint8_t* d = h->d[dev];
            if (h->nnz) HIP_TRY(hipMemcpyAsync(d, vals, sizeof(fr_mem_t) * h->nnz, hipMemcpyHostToDevice, c.stream));
            if (h->nseg) HIP_TRY(hipMemcpyAsync(d + h->off_segs, segs.data(), sizeof(fr_spmv_seg_t) * h->nseg, hipMemcpyHostToDevice, c.stream));
            if (h->nfix) HIP_TRY(hipMemcpyAsync(d + h->off_fix, fix.data(), sizeof(fr_spmv_fix_t) * h->nfix, hipMemcpyHostToDevice, c.stream));
            if (h->nnz) HIP_TRY(hipMemcpyAsync(d + h->off_col, col_idx, sizeof(uint32_t) * h->nnz, hipMemcpyHostToDevice, c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
        });
    } catch (...) {
        h->free_all();
        throw;
    }
    *handle = h.release();
    API_CATCH
}
void snarkvm_hip_fr_matrix_free(snarkvm_hip_fr_matrix_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}
// nullptr, or why the product is refused (hipErrorInvalidValue); needs no device
static const char* fr_spmv_check(const void* y, size_t n_out, const snarkvm_hip_fr_matrix* h, const void* x, size_t count, size_t stride_x, size_t stride_y, int on_device) {
    if (!h) return "null handle";
    if (n_out < h->rows) return "n_out is less than the number of rows";
    if (n_out > FR_SPMV_DIM_MAX) return "n_out > 2^28";
    if (count > 65535) return "more than 65535 batch members";
    if (count > 1 && ((stride_x && stride_x < h->cols) || stride_y < n_out)) return "a stride is shorter than its vector";
    // count < 2^16 members of at most 2^40 elements apart: no span below can wrap, in elements or in bytes
    if (count > 1 && (stride_x > ((size_t)1 << 40) || stride_y > ((size_t)1 << 40))) return "a stride of more than 2^40 elements";
    if (!y || (!x && h->nnz)) return "null operand";
    if (on_device) {
        const size_t span_x = h->cols ? (count - 1) * stride_x + h->cols : 0, span_y = (count - 1) * stride_y + n_out;
        const uint8_t *px = (const uint8_t*)x, *py = (const uint8_t*)y;
        if (px && span_x && px < py + sizeof(fr_mem_t) * span_y && py < px + sizeof(fr_mem_t) * span_x) return "y overlaps x (rows are owned by different waves: an in-place product races)";
    }
    return nullptr;
}
RustError snarkvm_hip_fr_spmv(void* y, size_t n_out, const snarkvm_hip_fr_matrix_t* h, const void* x, size_t count, size_t stride_x, size_t stride_y, int on_device) {
    if (h && (count == 0 || (n_out == 0 && h->rows == 0))) return ok();
    if (const char* why = fr_spmv_check(y, n_out, h, x, count, stride_x, stride_y, on_device)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_spmv: ") + why);
    if (count == 1) stride_x = stride_y = 0;
    API_BEGIN_DEV(device_for(y, on_device ? 1 : 0))
    const int dev = c.dev->logical;
    if (dev >= (int)h->d.size() || !h->d[dev]) throw hip_failure{hipErrorInvalidValue, "fr_spmv: the matrix has no replica on this device", __LINE__};
    const fr_mem_t* dx = (const fr_mem_t*)x;
    fr_mem_t* dy = (fr_mem_t*)y;
    size_t sx = stride_x, sy = stride_y;
    if (on_device) {
        fr_same_device(c, x, "fr_spmv: x lives on another device than y");
    } else {
        // host operands: x as it lies (members and the gaps between them), y packed member after member and downloaded member by member
        dx = fr_stage_in(c, 0, x, h->cols ? (count - 1) * stride_x + h->cols : 0, 0);
        dy = fr_stage_out(c, 1, y, count * n_out, 0);
        sy = n_out;
    }
    c.poly[4].ensure(sizeof(fr_mem_t) * (count * h->nparts ? count * h->nparts : 1));
    fr_mem_t* parts = c.poly[4].as<fr_mem_t>();
    switch (h->width) {
        case 4: fr_spmv_launch<4>(c, *h, dev, dx, sx, dy, sy, n_out, count, parts); break;
        case 8: fr_spmv_launch<8>(c, *h, dev, dx, sx, dy, sy, n_out, count, parts); break;
        case 16: fr_spmv_launch<16>(c, *h, dev, dx, sx, dy, sy, n_out, count, parts); break;
        default: fr_spmv_launch<64>(c, *h, dev, dx, sx, dy, sy, n_out, count, parts); break;
    }
    HIP_TRY(hipGetLastError());
    if (!on_device)
        for (size_t m = 0; m < count; m++) HIP_TRY(hipMemcpyAsync((fr_mem_t*)y + m * stride_y, dy + m * n_out, sizeof(fr_mem_t) * n_out, hipMemcpyDeviceToHost, c.stream));
    fr_call_done(c, on_device);
    API_END
}
// The product on host memory with the CPU in the kernels' place, for a GIVEN segment size and lane-group width: the same validation and layout,
// every lane of every segment through fr_spmv_lane, the butterfly level by level over the lanes it exchanges between, the partials, the fix-up
// launch with its own lanes and butterfly, the zero tail.  0, or -1 when refused.
static fr_t fr_spmv_tree_host(std::vector<fr_t>& lanes) {
    const size_t w = lanes.size();
    for (size_t off = w / 2; off >= 1; off >>= 1) {
        std::vector<fr_t> next(w);
        for (size_t l = 0; l < w; l++) next[l] = lanes[l] + lanes[l ^ off];
        lanes.swap(next);
    }
    return lanes[0];
}
int snarkvm_hip_selftest_fr_spmv(void* y, size_t n_out, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, const void* x,
                                 uint32_t seg, uint32_t width) {
    if (fr_spmv_matrix_check(rows, cols, row_ptr, col_idx, vals)) return -1;
    if (seg < 1 || (width != 4 && width != 8 && width != 16 && width != 64)) return -1;
    if (n_out < rows || n_out > FR_SPMV_DIM_MAX || (n_out && !y) || (row_ptr[rows] && !x)) return -1;
    std::vector<fr_spmv_seg_t> segs;
    std::vector<fr_spmv_fix_t> fix;
    const size_t nparts = fr_spmv_layout(rows, row_ptr, seg, segs, fix);
    std::vector<fr_mem_t> parts(nparts ? nparts : 1);
    fr_mem_t* py = (fr_mem_t*)y;
    std::vector<fr_t> lanes(width);
    for (const fr_spmv_seg_t& s : segs) {
        lanes.resize(width);
        for (uint32_t l = 0; l < width; l++) lanes[l] = fr_spmv_lane((const fr_mem_t*)vals + s.first, col_idx + s.first, (const fr_mem_t*)x, s.count, l, width);
        const fr_t v = fr_spmv_tree_host(lanes);
        if (s.part == FR_SPMV_SOLE)
            fr_spmv_finish(v).store(&py[s.row]);
        else
            v.store(&parts[s.part]);
    }
    for (const fr_spmv_fix_t& f : fix) {
        lanes.resize(width);
        for (uint32_t l = 0; l < width; l++) lanes[l] = fr_reduce_thread<FR_REDUCE_SUM>(parts.data() + f.first, nullptr, f.count, l, width);
        fr_spmv_finish(fr_spmv_tree_host(lanes)).store(&py[f.row]);
    }
    for (size_t r = rows; r < n_out; r++) fr_t::zero().store(&py[r]);
    return 0;
}
// what registration lays out for a matrix of `rows` rows and nnz entries spread evenly (the first nnz % rows rows one entry longer): out4 = {segment
// size S, lane-group width, threads per workgroup, segments}
int snarkvm_hip_selftest_fr_spmv_geometry(size_t rows, size_t nnz, uint32_t* out4) {
    if (!out4 || nnz > 0xFFFFFFFFull || rows > FR_SPMV_DIM_MAX || (nnz && !rows)) return -1;
    const size_t S = FR_SPMV_SEG, lo = rows ? nnz / rows : 0, longer = rows ? nnz % rows : 0;
    const size_t nseg = longer * ((lo + 1 + S - 1) / S) + (rows - longer) * ((lo + S - 1) / S);
    out4[0] = (uint32_t)S, out4[1] = fr_spmv_width(nnz, nseg), out4[2] = FR_SPMV_B, out4[3] = (uint32_t)nseg;
    return 0;
}

// ---- Varuna round 4: matrix-sumcheck evaluations over a registered arithmetization (poly.hip.h: fr_sumcheck_evals_kernel) -----------
static constexpr size_t FR_ARITH_K_MAX = (size_t)1 << NTT_LG_MAX;
}  // extern "C"
// one replica per logical device, like a registered matrix: ONE block holding row | col | row_col_val, k elements each
struct snarkvm_hip_fr_arith {
    size_t k = 0;
    std::vector<fr_mem_t*> d;  // [logical device]
    void free_all() {
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (size_t i = 0; i < d.size(); i++)
            if (d[i]) {
                (void)hipSetDevice(g_rt.devs[i]->physical);
                (void)hipFree(d[i]);  // waits for every stream of the device: nothing queued - an open scope's evaluation included - can still use the block
                d[i] = nullptr;
            }
        (void)hipSetDevice(prev);
    }
};
extern "C" {
RustError snarkvm_hip_fr_arith_register(snarkvm_hip_fr_arith_t** handle, size_t k, const void* row, const void* col, const void* row_col_val) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: null handle");
    *handle = nullptr;
    if (k > FR_ARITH_K_MAX) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: more than 2^28 elements");
    if (k && (!row || !col || !row_col_val)) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: null array of a non-empty arithmetization");
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_arith> h(new snarkvm_hip_fr_arith());
    h->k = k;
    const int nd = g_rt.ndev();
    h->d.assign(nd, nullptr);
    try {
        std::vector<int> all;
        for (int d = 0; d < nd; d++) all.push_back(d);
        for_each_device(all, [&](int dev) {  // every device uploads its own replica
            lane_guard lg(dev);
            lane_t& c = lg.c();
            const size_t bytes = sizeof(fr_mem_t) * k;
            HIP_TRY(hipMalloc((void**)&h->d[dev], k ? 3 * bytes : 32));
            if (k) {
                HIP_TRY(hipMemcpyAsync(h->d[dev], row, bytes, hipMemcpyHostToDevice, c.stream));
                HIP_TRY(hipMemcpyAsync(h->d[dev] + k, col, bytes, hipMemcpyHostToDevice, c.stream));
                HIP_TRY(hipMemcpyAsync(h->d[dev] + 2 * k, row_col_val, bytes, hipMemcpyHostToDevice, c.stream));
                HIP_TRY(hipStreamSynchronize(c.stream));
            }
        });
    } catch (...) {
        h->free_all();
        throw;
    }
    *handle = h.release();
    API_CATCH
}
void snarkvm_hip_fr_arith_free(snarkvm_hip_fr_arith_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}
// one wanted output of a call: member, which of a / b / f, the caller's pointer, elements
struct fr_sumcheck_out_t {
    size_t m;
    int which;
    uint8_t* p;
    size_t k;
};
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  outs: every non-NULL output of a member with k > 0.
static const char* fr_sumcheck_check(const snarkvm_hip_fr_arith_t* const* ariths, size_t count, void* const* a, void* const* b, void* const* f, const void* alpha,
                                     const void* beta, const void* scales, std::vector<fr_sumcheck_out_t>& outs) {
    if (count > (size_t)FR_SUMCHECK_MEMBERS) return "more than 16 members";
    if (!ariths) return "null list of handles";
    for (size_t m = 0; m < count; m++)
        if (!ariths[m]) return "null handle in the list";
    if (!alpha || !beta || !scales) return "null alpha, beta or scales";
    void* const* lists[3] = {a, b, f};
    for (size_t m = 0; m < count; m++)
        for (int w = 0; w < 3; w++)
            if (ariths[m]->k && lists[w] && lists[w][m]) outs.push_back({m, w, (uint8_t*)lists[w][m], ariths[m]->k});
    // sorted by address: any overlap shows between neighbours
    std::vector<fr_sumcheck_out_t> by_addr(outs);
    std::sort(by_addr.begin(), by_addr.end(), [](const fr_sumcheck_out_t& x, const fr_sumcheck_out_t& y) { return x.p < y.p; });
    for (size_t i = 1; i < by_addr.size(); i++)
        if (by_addr[i].p < by_addr[i - 1].p + sizeof(fr_mem_t) * by_addr[i - 1].k) return "two outputs overlap";
    return nullptr;
}
RustError snarkvm_hip_fr_matrix_sumcheck_evals(const snarkvm_hip_fr_arith_t* const* ariths, size_t count, void* const* a_evals, void* const* b_evals, void* const* f_evals,
                                               const void* alpha, const void* beta, const void* scales, int on_device) {
    if (count == 0) return ok();
    std::vector<fr_sumcheck_out_t> outs;
    if (const char* why = fr_sumcheck_check(ariths, count, a_evals, b_evals, f_evals, alpha, beta, scales, outs))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_matrix_sumcheck_evals: ") + why);
    if (outs.empty()) return ok();  // every k_m == 0, or nothing wanted
    API_BEGIN_DEV(device_for(outs[0].p, on_device ? 1 : 0))
    const int dev = c.dev->logical;
    if (on_device)
        for (const fr_sumcheck_out_t& o : outs) fr_same_device(c, o.p, "fr_matrix_sumcheck_evals: the outputs live on different devices");
    fr_sumcheck_t tab{};
    size_t threads = 0;
    for (const fr_sumcheck_out_t& o : outs) {
        const snarkvm_hip_fr_arith& h = *ariths[o.m];
        if (dev >= (int)h.d.size() || !h.d[dev]) throw hip_failure{hipErrorInvalidValue, "fr_matrix_sumcheck_evals: a handle has no replica on this device", __LINE__};
        fr_sumcheck_member_t& mb = tab.m[o.m];
        mb.row = h.d[dev], mb.col = h.d[dev] + h.k, mb.rcv = h.d[dev] + 2 * h.k;
        mb.k = h.k, mb.T = fr_sumcheck_threads(h.k);
        if (mb.T > threads) threads = mb.T;
    }
    fr_mem_t* staged = nullptr;
    if (!on_device) {  // host outputs: one lane buffer holds them one behind the other; one download each
        size_t total = 0;
        for (const fr_sumcheck_out_t& o : outs) total += o.k;
        c.poly[0].ensure(sizeof(fr_mem_t) * total);
        staged = c.poly[0].as<fr_mem_t>();
    }
    {
        fr_mem_t* next = staged;
        for (const fr_sumcheck_out_t& o : outs) {
            fr_mem_t* d = on_device ? (fr_mem_t*)o.p : next;
            fr_sumcheck_member_t& mb = tab.m[o.m];
            (o.which == 0 ? mb.a : (o.which == 1 ? mb.b : mb.f)) = d;
            if (!on_device) next += o.k;
        }
    }
    const uint8_t* sc = (const uint8_t*)scales;
    const fr_mem_t sc3[3] = {fr_mem_from_host(sc), fr_mem_from_host(sc + sizeof(fr_mem_t)), fr_mem_from_host(sc + 2 * sizeof(fr_mem_t))};
    tab.cs = fr_sumcheck_consts(fr_mem_from_host(alpha), fr_mem_from_host(beta), sc3);
    hipLaunchKernelGGL(fr_sumcheck_evals_kernel, dim3((unsigned)((threads + FR_SUMCHECK_B - 1) / FR_SUMCHECK_B), (unsigned)count), dim3(FR_SUMCHECK_B), 0, c.stream, tab);
    HIP_TRY(hipGetLastError());
    if (!on_device) {
        fr_mem_t* next = staged;
        for (const fr_sumcheck_out_t& o : outs) {
            HIP_TRY(hipMemcpyAsync(o.p, next, sizeof(fr_mem_t) * o.k, hipMemcpyDeviceToHost, c.stream));
            next += o.k;
        }
    }
    fr_call_done(c, on_device);
    API_END
}
// One member on host memory with the CPU in the kernel's place over blocks x threads threads: the same constants, every thread through
// fr_sumcheck_thread.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_sumcheck(void* a, void* b, void* f, const void* row, const void* col, const void* rcv, size_t k, const void* alpha, const void* beta,
                                     const void* scales, uint32_t blocks, uint32_t threads) {
    if (k > FR_ARITH_K_MAX || (k && (!row || !col || !rcv)) || !alpha || !beta || !scales || blocks < 1 || threads < 1) return -1;
    const uint8_t* sc = (const uint8_t*)scales;
    const fr_mem_t sc3[3] = {fr_mem_from_host(sc), fr_mem_from_host(sc + sizeof(fr_mem_t)), fr_mem_from_host(sc + 2 * sizeof(fr_mem_t))};
    const fr_sumcheck_consts_t cs = fr_sumcheck_consts(fr_mem_from_host(alpha), fr_mem_from_host(beta), sc3);
    fr_sumcheck_member_t mb{(const fr_mem_t*)row, (const fr_mem_t*)col, (const fr_mem_t*)rcv, (fr_mem_t*)a, (fr_mem_t*)b, (fr_mem_t*)f, k, (size_t)blocks * threads};
    for (size_t t = 0; t < mb.T && t < k; t++) fr_sumcheck_thread(mb, cs, t);
    return 0;
}
// what snarkvm_hip_fr_matrix_sumcheck_evals launches for a member of k elements: out4 = {threads, threads per workgroup, workgroups, elements per thread}
int snarkvm_hip_selftest_fr_sumcheck_geometry(size_t k, uint32_t* out4) {
    if (!out4 || k > FR_ARITH_K_MAX) return -1;
    const size_t T = fr_sumcheck_threads(k);
    out4[0] = (uint32_t)T, out4[1] = FR_SUMCHECK_B, out4[2] = (uint32_t)((T + FR_SUMCHECK_B - 1) / FR_SUMCHECK_B), out4[3] = (uint32_t)fr_sumcheck_share(k);
    return 0;
}

// ---- the circuit index: the arithmetization of a CSR matrix on K (poly.hip.h: fr_arithmetize_kernel) ---------------------------------
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device and touches nothing.  host_csr: the CSR arrays can be read here -
// after it no index the kernel will ever see points outside row_ptr, col_idx, vals or a table.  Device CSR: the contents are the caller's contract.
static const char* fr_arith_check(void* const* outs, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, uint32_t lg_constraint,
                                  uint32_t lg_variable, uint32_t lg_input, bool host_csr) {
    if (lg_constraint > (uint32_t)NTT_LG_MAX || lg_variable > (uint32_t)NTT_LG_MAX || lg_input > (uint32_t)NTT_LG_MAX) return "a domain of more than 2^28 elements";
    if (lg_input >= lg_variable) return "other.size() must be smaller than self.size() (lg_input >= lg_variable)";
    if (k > FR_ARITH_K_MAX) return "more than 2^28 elements";
    if (rows > ((size_t)1 << lg_constraint)) return "more rows than the constraint domain has elements";
    if (!row_ptr) return "null row_ptr";
    size_t span_vals = 1;  // device CSR: nnz cannot be read here - the first element of vals is checked, the rest is the caller's contract
    if (host_csr) {
        if (row_ptr[0] != 0) return "row_ptr[0] != 0";
        for (size_t r = 0; r < rows; r++)
            if (row_ptr[r + 1] < row_ptr[r]) return "row_ptr decreases";
        const uint64_t nnz = row_ptr[rows];
        if (nnz > 0xFFFFFFFFull) return "more than 2^32 - 1 entries";
        if (nnz && (!col_idx || !vals)) return "null col_idx or vals of a matrix with entries";
        if (k < nnz) return "k is less than the number of entries";
        for (uint64_t e = 0; e < nnz; e++)
            if (col_idx[e] >> lg_variable) return "a column index is not below the variable domain size";
        span_vals = (size_t)nnz;
    }
    for (int i = 0; i < 4; i++) {
        if (fr_ranges_overlap(outs[i], k, vals, span_vals)) return "an output overlaps vals";
        for (int j = i + 1; j < 4; j++)
            if (fr_ranges_overlap(outs[i], k, outs[j], k)) return "two outputs overlap";
    }
    return nullptr;
}
static fr_mem_t fr_domain_generator_mem(uint32_t lg) {  // group_gen of the 2^lg domain (fft_field.rs:75-85), memory form
    fr_t omega = fr_t::unpack(FR_TWO_ADIC_ROOT_MEM_HOST).from_mem_mont();
    for (uint32_t i = lg; i < 47; i++) omega = omega.sqr();
    fr_mem_t m;
    omega.to_mem_mont().store(&m);
    return m;
}
// everything of a kernel argument but the pointers
static fr_arith_t fr_arith_args(size_t k, size_t rows, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, uint32_t s_r, uint32_t s_c) {
    fr_arith_t a{};
    fr_t::one().to_mem_mont().store(&a.one);
    const fr_t fix2 = fr_t::one().from_mem_mont().from_mem_mont();
    for (int l = 0; l < 9; l++) a.fix2[l] = fix2.v[l];
    a.k = (uint32_t)k, a.rows = (uint32_t)rows;
    a.s_r = s_r, a.mask_r = (1u << lg_constraint) - 1, a.s_c = s_c, a.mask_c = (1u << lg_variable) - 1;
    a.input_size = 1u << lg_input, a.period = 1u << (lg_variable - lg_input);
    return a;
}
// the tables and the pass, enqueued on the lane's stream; every pointer is device memory of the lane's device.  Tables: c.poly[4].
static void fr_arith_run(lane_t& c, fr_mem_t* const* outs, size_t k, size_t rows, const uint64_t* d_row_ptr, const uint32_t* d_col, const fr_mem_t* d_vals,
                         uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input) {
    const uint32_t s_r = fr_arith_split(lg_constraint), s_c = FR_ARITH_FULL_TABLE ? lg_variable : fr_arith_split(lg_variable);
    const size_t n_r = ((size_t)1 << s_r) + ((size_t)1 << (lg_constraint - s_r)), n_c = ((size_t)1 << s_c) + ((size_t)1 << (lg_variable - s_c));
    c.poly[4].ensure(sizeof(fr_mem_t) * (n_r + n_c));
    fr_mem_t* t = c.poly[4].as<fr_mem_t>();
    fr_arith_t a = fr_arith_args(k, rows, lg_constraint, lg_variable, lg_input, s_r, s_c);
    a.row = outs[0], a.col = outs[1], a.row_col = outs[2], a.rcv = outs[3];
    a.row_ptr = d_row_ptr, a.col_idx = d_col, a.vals = d_vals;
    a.r_lo = t, a.r_hi = t + ((size_t)1 << s_r), a.c_lo = t + n_r, a.c_hi = t + n_r + ((size_t)1 << s_c);
    hipLaunchKernelGGL(fr_arith_tables_kernel, dim3((unsigned)((n_r + 255) / 256)), dim3(256), 0, c.stream, t, t + ((size_t)1 << s_r), fr_domain_generator_mem(lg_constraint), s_r,
                       (uint32_t)n_r);
#if FR_ARITH_FULL_TABLE  // measurement variant: w_C^x for every x of the variable domain, as fr_lagrange_coefficients forms them
    hipLaunchKernelGGL(fr_fill_kernel, dim3(fr_grid((size_t)1 << lg_variable)), dim3(256), 0, c.stream, t + n_r, (size_t)1 << lg_variable, a.one);
    fr_distribute_powers_run(c, t + n_r, (size_t)1 << lg_variable, fr_domain_generator_mem(lg_variable), a.one);
#else
    hipLaunchKernelGGL(fr_arith_tables_kernel, dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0, c.stream, t + n_r, t + n_r + ((size_t)1 << s_c),
                       fr_domain_generator_mem(lg_variable), s_c, (uint32_t)n_c);
#endif
    hipLaunchKernelGGL(fr_arithmetize_kernel, dim3(fr_grid(k)), dim3(256), 0, c.stream, a);
    HIP_TRY(hipGetLastError());
}
// the host CSR arrays as device pointers in c.poly[0 .. 2]
static void fr_arith_stage_csr(lane_t& c, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, const uint64_t*& d_row_ptr, const uint32_t*& d_col,
                               const fr_mem_t*& d_vals) {
    const size_t nnz = (size_t)row_ptr[rows];
    c.poly[0].ensure(sizeof(uint64_t) * (rows + 1) + (FR_ARITH_ROW_INDEX ? sizeof(uint32_t) * nnz : 0));
    c.poly[1].ensure(sizeof(uint32_t) * (nnz ? nnz : 1));
    HIP_TRY(hipMemcpyAsync(c.poly[0].p, row_ptr, sizeof(uint64_t) * (rows + 1), hipMemcpyHostToDevice, c.stream));
#if FR_ARITH_ROW_INDEX  // measurement variant: the row of every entry, expanded here and laid behind row_ptr (the copy is synchronous: pageable memory)
    {
        std::vector<uint32_t> row_of(nnz);
        for (size_t r = 0; r < rows; r++)
            for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) row_of[e] = (uint32_t)r;
        if (nnz) HIP_TRY(hipMemcpy(c.poly[0].as<uint64_t>() + rows + 1, row_of.data(), sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    }
#endif
    if (nnz) HIP_TRY(hipMemcpyAsync(c.poly[1].p, col_idx, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, c.stream));
    d_row_ptr = c.poly[0].as<uint64_t>(), d_col = c.poly[1].as<uint32_t>();
    d_vals = fr_stage_in(c, 2, nnz ? vals : nullptr, nnz, 0);
}
RustError snarkvm_hip_fr_arithmetize(void* row, void* col, void* row_col, void* row_col_val, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                                     const void* vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, int on_device) {
    void* const outs[4] = {row, col, row_col, row_col_val};
    if (const char* why = fr_arith_check(outs, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, !on_device))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_arithmetize: ") + why);
    void* first = row ? row : (col ? col : (row_col ? row_col : row_col_val));
    if (k == 0 || !first) return ok();
    API_BEGIN_DEV(device_for(first, on_device ? 1 : 0))
    fr_mem_t* d_outs[4] = {(fr_mem_t*)row, (fr_mem_t*)col, (fr_mem_t*)row_col, (fr_mem_t*)row_col_val};
    const uint64_t* d_row_ptr = row_ptr;
    const uint32_t* d_col = col_idx;
    const fr_mem_t* d_vals = (const fr_mem_t*)vals;
    if (on_device) {
        const char* why = "fr_arithmetize: the operands live on different devices";
        for (int i = 0; i < 4; i++) fr_same_device(c, outs[i], why);
        fr_same_device(c, row_ptr, why);
        fr_same_device(c, col_idx, why);
        fr_same_device(c, vals, why);
    } else {  // host operands: the CSR arrays in three lane buffers, the wanted outputs one behind the other in a fourth; one download each
        fr_arith_stage_csr(c, rows, row_ptr, col_idx, vals, d_row_ptr, d_col, d_vals);
        size_t wanted = 0;
        for (int i = 0; i < 4; i++) wanted += outs[i] ? 1 : 0;
        c.poly[3].ensure(sizeof(fr_mem_t) * wanted * k);
        fr_mem_t* next = c.poly[3].as<fr_mem_t>();
        for (int i = 0; i < 4; i++)
            if (outs[i]) d_outs[i] = next, next += k;
    }
    fr_arith_run(c, d_outs, k, rows, d_row_ptr, d_col, d_vals, lg_constraint, lg_variable, lg_input);
    if (!on_device)
        for (int i = 0; i < 4; i++)
            if (outs[i]) HIP_TRY(hipMemcpyAsync(outs[i], d_outs[i], sizeof(fr_mem_t) * k, hipMemcpyDeviceToHost, c.stream));
    fr_call_done(c, on_device);
    API_END
}
RustError snarkvm_hip_fr_arith_register_csr(snarkvm_hip_fr_arith_t** handle, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals,
                                            uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register_csr: null handle");
    *handle = nullptr;
    void* const none[4] = {nullptr, nullptr, nullptr, nullptr};
    if (const char* why = fr_arith_check(none, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, true))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_arith_register_csr: ") + why);
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_arith> h(new snarkvm_hip_fr_arith());
    h->k = k;
    const int nd = g_rt.ndev();
    h->d.assign(nd, nullptr);
    try {
        std::vector<int> all;
        for (int d = 0; d < nd; d++) all.push_back(d);
        for_each_device(all, [&](int dev) {  // every device computes its own replica from the CSR arrays
            lane_guard lg(dev);
            lane_t& c = lg.c();
            HIP_TRY(hipMalloc((void**)&h->d[dev], k ? 3 * sizeof(fr_mem_t) * k : 32));
            if (k) {
                const uint64_t* d_row_ptr;
                const uint32_t* d_col;
                const fr_mem_t* d_vals;
                fr_arith_stage_csr(c, rows, row_ptr, col_idx, vals, d_row_ptr, d_col, d_vals);
                fr_mem_t* const outs[4] = {h->d[dev], h->d[dev] + k, nullptr, h->d[dev] + 2 * k};
                fr_arith_run(c, outs, k, rows, d_row_ptr, d_col, d_vals, lg_constraint, lg_variable, lg_input);
                HIP_TRY(hipStreamSynchronize(c.stream));
            }
        });
    } catch (...) {
        h->free_all();
        throw;
    }
    *handle = h.release();
    API_CATCH
}
// snarkvm_hip_fr_arithmetize on host memory with the CPU in the kernel's place, for a GIVEN table split (split_bits low bits per domain, cut to the
// domain's lg) and `threads` threads: the same validation, the tables through fr_arith_table_at, thread t over e = t, t + threads, ... through
// fr_arith_at.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_arithmetize(void* row, void* col, void* row_col, void* row_col_val, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                                        const void* vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, uint32_t split_bits, uint32_t threads) {
    void* const outs[4] = {row, col, row_col, row_col_val};
    if (FR_ARITH_FULL_TABLE || FR_ARITH_ROW_INDEX) return -1;  // a measurement variant has no twin
    if (threads < 1 || fr_arith_check(outs, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, true)) return -1;
    const uint32_t s_r = split_bits < lg_constraint ? split_bits : lg_constraint, s_c = split_bits < lg_variable ? split_bits : lg_variable;
    const size_t n_r = ((size_t)1 << s_r) + ((size_t)1 << (lg_constraint - s_r)), n_c = ((size_t)1 << s_c) + ((size_t)1 << (lg_variable - s_c));
    std::vector<fr_mem_t> tab(n_r + n_c);
    const fr_mem_t w_r = fr_domain_generator_mem(lg_constraint), w_c = fr_domain_generator_mem(lg_variable);
    for (size_t t = 0; t < n_r; t++) fr_arith_table_at(tab.data(), tab.data() + ((size_t)1 << s_r), fr_t::load(&w_r).from_mem_mont(), s_r, (uint32_t)t);
    for (size_t t = 0; t < n_c; t++) fr_arith_table_at(tab.data() + n_r, tab.data() + n_r + ((size_t)1 << s_c), fr_t::load(&w_c).from_mem_mont(), s_c, (uint32_t)t);
    fr_arith_t a = fr_arith_args(k, rows, lg_constraint, lg_variable, lg_input, s_r, s_c);
    a.row = (fr_mem_t*)row, a.col = (fr_mem_t*)col, a.row_col = (fr_mem_t*)row_col, a.rcv = (fr_mem_t*)row_col_val;
    a.row_ptr = row_ptr, a.col_idx = col_idx, a.vals = (const fr_mem_t*)vals;
    a.r_lo = tab.data(), a.r_hi = tab.data() + ((size_t)1 << s_r), a.c_lo = tab.data() + n_r, a.c_hi = tab.data() + n_r + ((size_t)1 << s_c);
    const uint32_t nnz = (uint32_t)row_ptr[rows];
    for (size_t t = 0; t < threads && t < k; t++)
        for (size_t e = t; e < k; e += threads) fr_arith_at(a, nnz, (uint32_t)e);
    return 0;
}
// what snarkvm_hip_fr_arithmetize launches for k elements, and the table split of a domain of 2^lg elements: out4 = {workgroups, threads per
// workgroup, the cap on workgroups, split bits s}
int snarkvm_hip_selftest_fr_arithmetize_geometry(size_t k, uint32_t lg, uint32_t* out4) {
    if (!out4 || k > FR_ARITH_K_MAX || lg > (uint32_t)NTT_LG_MAX) return -1;
    out4[0] = fr_grid(k), out4[1] = 256, out4[2] = 8192, out4[3] = fr_arith_split(lg);
    return 0;
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
        fr_t omega = fr_t::unpack(FR_TWO_ADIC_ROOT_MEM_HOST).from_mem_mont();
        for (uint32_t i = lg; i < 47; i++) omega = omega.sqr();  // group_gen of the 2^lg domain (fft_field.rs:75-85)
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

