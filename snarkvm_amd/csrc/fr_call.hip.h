// fr_call.hip.h - the host-side frame of an Fr entry point, shared by api_fr.hip (transforms, group operations), api_poly.hip (vector passes,
// divisions, combinations, reductions) and api_varuna.hip (the prover rounds and the circuit index): operand staging, the refusals every call
// makes (strides, devices, overlaps), the packing of host operands into one workspace slot and the per-device replicas of a registered handle.
// One definition of each; [[maybe_unused]] because no unit uses all of them.
#pragma once
#include "runtime.hip.h"
#include "poly.hip.h"

#include <algorithm>

[[maybe_unused]] static fr_mem_t fr_mem_from_host(const void* p) {
    fr_mem_t m;
    memcpy(&m, p, sizeof m);
    return m;
}
[[maybe_unused]] static unsigned fr_grid(size_t n, unsigned block = 256) {
    const size_t b = (n + block - 1) / block;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
// operand `p` (n elements) as a device pointer: itself, or a staged copy in ctx.poly[slot]
[[maybe_unused]] static fr_mem_t* fr_stage_in(lane_t& c, int slot, const void* p, size_t n, int on_device) {
    if (on_device || !p) return (fr_mem_t*)p;
    c.poly[slot].ensure(sizeof(fr_mem_t) * (n ? n : 1));
    if (n) HIP_TRY(hipMemcpyAsync(c.poly[slot].p, p, sizeof(fr_mem_t) * n, hipMemcpyHostToDevice, c.stream));
    return c.poly[slot].as<fr_mem_t>();
}
[[maybe_unused]] static fr_mem_t* fr_stage_out(lane_t& c, int slot, void* p, size_t n, int on_device) {
    if (on_device || !p) return (fr_mem_t*)p;
    c.poly[slot].ensure(sizeof(fr_mem_t) * (n ? n : 1));
    return c.poly[slot].as<fr_mem_t>();
}
[[maybe_unused]] static void fr_finish_out(lane_t& c, fr_mem_t* d, void* p, size_t n, int on_device) {
    if (!on_device && p && n) HIP_TRY(hipMemcpyAsync(p, d, sizeof(fr_mem_t) * n, hipMemcpyDeviceToHost, c.stream));
}
// end of a vector call: device-resident operands may leave the wait to the calling thread's scope (runtime.hip.h), host operands never
[[maybe_unused]] static void fr_call_done(lane_t& c, int on_device) {
    if (on_device)
        c.sync_or_defer();
    else
        HIP_TRY(hipStreamSynchronize(c.stream));
}

[[maybe_unused]] static void check_strided(size_t n, size_t count, size_t stride, int on_device) {
    if (count == 0 || (count > 1 && (!on_device || stride < n)) || count > 65535)
        throw hip_failure{hipErrorInvalidValue, "strided batch of an Fr vector pass: needs device operands, 1 <= count <= 65535 and stride >= the vector length", __LINE__};
}
// check_strided without a lane: the same refusal, before any device is needed
[[maybe_unused]] static bool fr_strided_refused(size_t n, size_t count, size_t stride, RustError& err) {
    try {
        check_strided(n, count, stride, 1);
    } catch (const hip_failure& f) {
        err = from_failure(f);
        return true;
    }
    return false;
}
[[maybe_unused]] static void fr_same_device(lane_t& c, const void* p, const char* what) {
    if (p && g_rt.devs[device_for(p, 1)]->physical != c.dev->physical) throw hip_failure{hipErrorInvalidValue, what, __LINE__};
}
[[maybe_unused]] static fr_t fr_from_u64(uint64_t x) {
    const fr_t two32 = fr_t::from_u32(65536).sqr();
    return fr_t::from_u32((uint32_t)(x >> 32)) * two32 + fr_t::from_u32((uint32_t)x);
}
[[maybe_unused]] static size_t fr_gcd(size_t a, size_t b) {
    while (b) {
        const size_t r = a % b;
        a = b, b = r;
    }
    return a;
}

// TWO_ADIC_ROOT_OF_UNITY (fr.rs:115-120), memory form - the host copy of ntt.hip.h's device table
static const uint32_t FR_TWO_ADIC_ROOT_MEM_HOST[8] = {0xda3ad648u, 0xaf80da4du, 0xfc381dacu, 0x5e223adbu,
                                                      0xb2f92525u, 0x03ba0666u, 0x3befb0ceu, 0x0f906c5bu};
[[maybe_unused]] static fr_t fr_domain_generator(uint32_t lg) {  // group_gen of the 2^lg domain (fft_field.rs:75-85)
    fr_t omega = fr_t::unpack(FR_TWO_ADIC_ROOT_MEM_HOST).from_mem_mont();
    for (uint32_t i = lg; i < 47; i++) omega = omega.sqr();
    return omega;
}
// v[i] *= cmul g^i, enqueued on the lane's stream
[[maybe_unused]] static void fr_distribute_powers_run(lane_t& c, fr_mem_t* d_v, size_t n, const fr_mem_t& g, const fr_mem_t& cmul) {
    size_t T = (n + 31) / 32;
    if (T > (size_t)1 << 17) T = (size_t)1 << 17;
    hipLaunchKernelGGL(fr_distribute_powers_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, c.stream, d_v, n, g, cmul, T);
    HIP_TRY(hipGetLastError());
}

// ---- overlaps ----------------------------------------------------------------------------------------------------------------
// do the spans of np elements at p and nq elements at q share memory?  A null or empty span overlaps nothing.  What a call allows beyond
// that (an output that IS an operand) is the call's own exception, made before it asks.
[[maybe_unused]] static bool fr_spans_overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uint8_t *x = (const uint8_t*)p, *y = (const uint8_t*)q;
    return p && q && np && nq && x < y + sizeof(fr_mem_t) * nq && y < x + sizeof(fr_mem_t) * np;
}
// Many ranges at once: does an output overlap an operand or another output?  Sorted by address, an overlap shows against the furthest end seen
// so far.  Empty ranges are the caller's to leave out.
struct fr_range_t {
    const uint8_t* p;
    size_t bytes;
    bool out;
};
[[maybe_unused]] static bool fr_output_overlaps(std::vector<fr_range_t> rs) {
    std::sort(rs.begin(), rs.end(), [](const fr_range_t& x, const fr_range_t& y) { return x.p < y.p; });
    const uint8_t *end_any = nullptr, *end_out = nullptr;
    for (const fr_range_t& r : rs) {
        if (r.p < (r.out ? end_any : end_out)) return true;
        if (r.p + r.bytes > end_any) end_any = r.p + r.bytes;
        if (r.out && r.p + r.bytes > end_out) end_out = r.p + r.bytes;
    }
    return false;
}

// ---- the assignment gather (poly.hip.h: fr_assignment_evals_kernel) ------------------------------------------------------------
// What snarkvm_hip_fr_assignment_evals (api_varuna.hip) and its host twin (api_selftest.hip) share: nullptr, or why the call is refused
// (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  After it no index the kernel forms can leave a member's
// row (num_vars elements) or its output (n elements), and no member's span can wrap.
static constexpr size_t FR_ASSIGNMENT_N_MAX = (size_t)1 << 28;
[[maybe_unused]] static const char* fr_assignment_check(const void* out, size_t n, const void* vars, size_t num_vars, size_t input_size, size_t count, size_t stride_out,
                                                        size_t stride_vars) {
    if (input_size == 0) return "input_size is 0";
    if (n % input_size) return "input_size does not divide n";
    if (n > FR_ASSIGNMENT_N_MAX) return "n above 2^28";
    if (n && (num_vars < input_size || num_vars > n)) return "num_vars is below input_size or above n";
    if (count > 65535) return "more than 65535 members";
    if (count > 1 && (stride_out < n || stride_vars < num_vars)) return "a stride is shorter than its vector";
    // count < 2^16 members of at most 2^40 elements apart: no span below can wrap, in elements or in bytes
    if (count > 1 && (stride_out > ((size_t)1 << 40) || stride_vars > ((size_t)1 << 40))) return "a stride of more than 2^40 elements";
    if (n && count && (!out || !vars)) return "null operand of non-zero length";
    if (n && count && fr_spans_overlap(out, (count - 1) * stride_out + n, vars, (count - 1) * stride_vars + num_vars)) return "out overlaps vars";
    return nullptr;
}
// the launch of one member's n elements: fr_grid's workgroups of 256 threads, the member on blockIdx.y
static constexpr unsigned FR_ASSIGNMENT_BLOCK = 256;

// ---- host operands -----------------------------------------------------------------------------------------------------------
// host operands: one lane buffer (c.poly[slot]) holds the outputs and the operands of a call one behind the other; one upload per operand,
// one download per output.  begin() takes the total up front - ensure() may move the buffer; a pack that was never begun (device operands)
// downloads nothing.
struct fr_host_pack_t {
    lane_t& c;
    fr_mem_t* next = nullptr;
    bool begun = false;
    struct out_t {
        void* host;
        const fr_mem_t* dev;
        size_t n;
    };
    std::vector<out_t> outs;
    explicit fr_host_pack_t(lane_t& lane) : c(lane) {}
    void begin(int slot, size_t total) {
        c.poly[slot].ensure(sizeof(fr_mem_t) * total);
        next = c.poly[slot].as<fr_mem_t>();
        begun = true;
    }
    void need_begun() const {
        if (!begun) throw hip_failure{hipErrorInvalidValue, "fr_host_pack_t: out() or in() before begin()", __LINE__};
    }
    fr_mem_t* out(void* host, size_t n) {
        need_begun();
        outs.push_back({host, next, n});
        next += n;
        return next - n;
    }
    const fr_mem_t* in(const void* host, size_t n) {  // nullptr for an empty operand
        if (!n) return nullptr;
        need_begun();
        HIP_TRY(hipMemcpyAsync(next, host, sizeof(fr_mem_t) * n, hipMemcpyHostToDevice, c.stream));
        next += n;
        return next - n;
    }
    void download() {
        for (const out_t& o : outs)
            if (o.n) HIP_TRY(hipMemcpyAsync(o.host, o.dev, sizeof(fr_mem_t) * o.n, hipMemcpyDeviceToHost, c.stream));
    }
};

// ---- registered handles ------------------------------------------------------------------------------------------------------
// one replica per logical device, like registered bases: ONE block of device memory each
template <class T>
struct fr_replicas_t {
    std::vector<T*> d;  // [logical device]
    void free_all() {
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (size_t i = 0; i < d.size(); i++)
            if (d[i]) {
                (void)hipSetDevice(g_rt.devs[i]->physical);
                (void)hipFree(d[i]);  // waits for every stream of the device: nothing queued - an open scope's call included - can still use the block
                d[i] = nullptr;
            }
        (void)hipSetDevice(prev);
    }
    // every device allocates `bytes` and fills its replica - fill(lane, block) uploads or computes it and waits for the lane's stream; a
    // failure on any device frees them all
    template <class Fill>
    void fill_all(size_t bytes, Fill fill) {
        const int nd = g_rt.ndev();
        d.assign(nd, nullptr);
        try {
            std::vector<int> all;
            for (int dev = 0; dev < nd; dev++) all.push_back(dev);
            for_each_device(all, [&](int dev) {
                lane_guard lg(dev);
                lane_t& c = lg.c();
                HIP_TRY(hipMalloc((void**)&d[dev], bytes ? bytes : 32));
                fill(c, d[dev]);
            });
        } catch (...) {
            free_all();
            throw;
        }
    }
    // the replica of the lane's device; `why_not`: the caller's "has no replica on this device"
    T* on(const lane_t& c, const char* why_not) const {
        const int dev = c.dev->logical;
        if (dev >= (int)d.size() || !d[dev]) throw hip_failure{hipErrorInvalidValue, why_not, __LINE__};
        return d[dev];
    }
};
