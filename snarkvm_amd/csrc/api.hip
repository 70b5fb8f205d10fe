// api.hip - C ABI (include/snarkvm_hip.h) of the gfx950 MSM / NTT backend: runtime configuration and the G1 MSM entry points.
//
// Host runtime (runtime.hip.h) = what algorithms/cuda/cuda/snarkvm.cu:73-312 (snarkvm_t) and snarkvm_api.cu:23-84 are in the
// reference: a lazily constructed per-process runtime over every selected GPU (device arenas, streams, twiddle tables), a
// pool of (device, stream) resource tokens handed to concurrent callers, staging of the caller's host buffers, the
// point-range split of one MSM over the GPUs with a host-side combine, error reporting as RustError.
// This unit: the runtime's globals, configuration, device memory and scopes; the G1 registered-bases and registered-MSM entry points (validation over the
// front end shared with G2, msm_registered.hip.h); `snarkvm_msm` over its base cache (base_cache.hip.h); g1_sum / g1_to_affine and the synthetic bases.
// Fr entry points: api_fr.hip (NTT, polymul), api_poly.hip (polynomial passes), api_varuna.hip (prover rounds); point encoding + setup-time group operations:
// api_serde.hip; G2: api_g2.hip; test hooks: api_selftest.hip (host arithmetic), api_fieldtest.hip, api_msmtest.hip, api_tailtest.hip.
#include "msm_registered.hip.h"
#include "ffl.hip.h"
#include "g1_generator.hip.h"  // the seed of the synthetic bases

// this unit launches the scans and the G1 MSMs (msm_acc_lds: the lazy accumulate kernel's LDS request)
static void tu_set_kernel_attributes() {
    HIP_TRY(hipFuncSetAttribute((const void*)scan_one_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SCAN_ONE_MAX * 4)));
    HIP_TRY(hipFuncSetAttribute((const void*)msm_accumulate_lazy_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
}

runtime_t g_rt;
thread_local thread_scope_t g_tl_scope;
// A thread that ends inside a scope (a worker that died, a caller that forgot scope_end): its lanes return to the pool - they are a bounded resource
// (12 of a GPU's 16 may be held by scopes) and nobody else can end this scope.  The queued work is waited for; results that were still owed (MSM
// outputs, parked remainders) are NOT delivered: their buffers belong to a thread that is gone.
thread_scope_t::~thread_scope_t() {
    if (!lane) return;
    pending.clear();
    (void)hipStreamSynchronize(lane->stream);
    for (int i = 0; i < naux; i++) {
        (void)hipStreamSynchronize(aux[i]->stream);
        aux[i]->dev->give(aux[i], true);
    }
    lane->in_scope = false;
    lane->deferred.clear();
    lane->deferred_bytes = 0;
    if (!lane->tw_leases.empty()) ntt_tw_release(lane->dev, lane->tw_leases);
    lane->dev->give(lane, true);
    lane = nullptr;
}
std::atomic<uint64_t> g_co_stats[4];
static std::atomic<uint64_t> g_alloc_stats[5];  // {device allocations, device bytes, pinned allocations, pinned bytes, microseconds}
void sv_alloc_note(int slot, size_t bytes, double ms) {
    g_alloc_stats[slot].fetch_add(1, std::memory_order_relaxed);
    g_alloc_stats[slot + 1].fetch_add(bytes, std::memory_order_relaxed);
    g_alloc_stats[4].fetch_add((uint64_t)(ms * 1e3), std::memory_order_relaxed);
}

// Outgrown workspace blocks (runtime.hip.h: sv_defer_free) wait on a list of the THREAD that outgrew them and are released when that thread's call ends
// (lane_t::end_call) or its scope is flushed.  (Round 5 kept one process-wide list that every lane's end_call drained: hipFree waits for every stream
// of the device, so a short call of thread B inherited the wait for thread A's whole queued scope - the stall the deferral exists to avoid, moved to
// another caller.)  A thread that ends with blocks still parked releases them in the list's destructor.
struct tl_free_list_t {
    std::vector<void*> v;
    ~tl_free_list_t() {
        for (void* p : v) (void)hipFree(p);
    }
};
static thread_local tl_free_list_t g_tl_free;
void sv_defer_free(void* p) { g_tl_free.v.push_back(p); }
void sv_drain_frees() {
    if (g_tl_free.v.empty()) return;
    std::vector<void*> mine;
    mine.swap(g_tl_free.v);
    for (void* p : mine) (void)hipFree(p);  // hipFree takes a pointer of any device
}

extern "C" {

int snarkvm_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int snarkvm_hip_batch_lanes(size_t npoints) { return batch_lanes(npoints); }
// Select the devices this process uses (before the first compute call).  Duplicated ids make independent logical devices on
// one GPU (tests).  snarkvm_hip_set_device(d) == set_devices(&d, 1): the one-process-per-GPU deployment.
RustError snarkvm_hip_set_devices(const int32_t* ids, size_t n) {
    std::lock_guard<std::mutex> lk(g_rt.cfg_mu);
    if (n == 0 || !ids) return fail(1, "snarkvm_hip_set_devices: empty device list");
    std::vector<int> v(ids, ids + n);
    if (g_rt.configured) {
        bool same = v.size() == g_rt.devs.size();
        for (size_t i = 0; same && i < v.size(); i++) same = g_rt.devs[i]->physical == v[i];
        if (!same) return fail(1, "snarkvm_hip_set_devices: the runtime is already initialised on another device set");
        return ok();
    }
    g_rt.want = v;
    return ok();
}
RustError snarkvm_hip_set_device(int device) {
    const int32_t d = device;
    return snarkvm_hip_set_devices(&d, 1);
}
int snarkvm_hip_num_devices(void) {
    try {
        return g_rt.ndev();
    } catch (...) {
        return 0;
    }
}
void snarkvm_hip_set_profiling(int enabled) { g_rt.profiling.store(enabled != 0); }
int snarkvm_hip_get_phase_count(void) {
    std::lock_guard<std::mutex> lk(g_rt.prof_mu);
    return (int)g_rt.last_phases.size();
}
const char* snarkvm_hip_get_phase_name(int i) {
    std::lock_guard<std::mutex> lk(g_rt.prof_mu);
    return (i >= 0 && i < (int)g_rt.last_phases.size()) ? g_rt.last_phases[i].first.c_str() : "";
}
double snarkvm_hip_get_phase_ms(int i) {
    std::lock_guard<std::mutex> lk(g_rt.prof_mu);
    return (i >= 0 && i < (int)g_rt.last_phases.size()) ? g_rt.last_phases[i].second : 0.0;
}

// coalescer statistics (G1 and G2 callers): out[4] = {batches dispatched, tickets in them, largest
// batch, single-ticket batches}; reset != 0 clears them
void snarkvm_hip_coalescer_stats(uint64_t* out, int reset) {
    for (int i = 0; i < 4; i++) {
        if (out) out[i] = g_co_stats[i].load();
        if (reset) g_co_stats[i].store(0);
    }
}
void snarkvm_hip_alloc_stats(uint64_t* out, int reset) {
    for (int i = 0; i < 5; i++) {
        if (out) out[i] = g_alloc_stats[i].load();
        if (reset) g_alloc_stats[i].store(0);
    }
}
RustError snarkvm_hip_synchronize(void) {
    API_TRY
    g_rt.configure();
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (auto& d : g_rt.devs) {
        if (!d->ready) continue;
        HIP_TRY(hipSetDevice(d->physical));
        for (auto& l : d->lane) {
            HIP_TRY(hipStreamSynchronize(l.stream));
            HIP_TRY(hipStreamSynchronize(l.alt));
        }
    }
    (void)hipSetDevice(prev);
    API_CATCH
}

// ---- device memory for hosts without a HIP binding (a Rust prover) ---------------------------------------------
// Plain hipMalloc / hipFree / copies behind the C ABI, so that the device-resident entry points can be fed without torch or a HIP crate
// on the caller's side.  Copies run on a lane like every other call: inside the calling thread's scope that is the scope's own stream
// (ordered with its transforms), outside a scope any free lane of the device that owns the device pointer.
RustError snarkvm_hip_malloc(void** d_ptr, size_t bytes, int device) {
    API_TRY
    if (!d_ptr) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_malloc: null result pointer", __LINE__};
    *d_ptr = nullptr;
    g_rt.configure();
    lane_t* sl = tl_scope().lane;
    if (device < 0) device = sl ? sl->dev->logical : 0;
    if (device >= (int)g_rt.devs.size()) throw hip_failure{hipErrorInvalidDevice, "snarkvm_hip_malloc: logical device index out of range", __LINE__};
    if (bytes) {
        int prev = -1;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        const int phys = g_rt.devs[device]->physical;
        if (prev != phys) HIP_TRY(hipSetDevice(phys));
        const hipError_t e = hipMalloc(d_ptr, bytes);
        if (prev >= 0 && prev != phys) (void)hipSetDevice(prev);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *d_ptr = nullptr;
            throw hip_failure{e, "snarkvm_hip_malloc: hipMalloc", __LINE__};
        }
    }
    API_CATCH
}
RustError snarkvm_hip_free(void* d_ptr) {
    API_TRY
    if (d_ptr) HIP_TRY(hipFree(d_ptr));  // waits for every stream of the owning device: nothing queued can still use the block
    API_CATCH
}
RustError snarkvm_hip_memcpy_h2d(void* d_dst, const void* src, size_t bytes) {
    if (!bytes) return ok();
    API_BEGIN_DEV(device_for(d_dst, 1))
    if (!d_dst || !src) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_memcpy_h2d: null pointer", __LINE__};
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));  // host side: complete on return, also inside a scope (header)
    API_END
}
RustError snarkvm_hip_memcpy_d2h(void* dst, const void* d_src, size_t bytes) {
    if (!bytes) return ok();
    API_BEGIN_DEV(device_for(d_src, 1))
    if (!dst || !d_src) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_memcpy_d2h: null pointer", __LINE__};
    HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    API_END
}
RustError snarkvm_hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes) {
    if (!bytes) return ok();
    API_BEGIN_DEV(device_for(d_dst, 1))
    if (!d_dst || !d_src) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_memcpy_d2d: null pointer", __LINE__};
    const uint8_t *a = (const uint8_t*)d_dst, *b = (const uint8_t*)d_src;
    if (a < b + bytes && b < a + bytes) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_memcpy_d2d: the ranges overlap", __LINE__};
    if (g_rt.device_of(d_src) < 0) throw hip_failure{hipErrorInvalidValue, "snarkvm_hip_memcpy_d2d: source is not on a device in use", __LINE__};
    HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDefault, c.stream));
    c.sync_or_defer();
    API_END
}
RustError snarkvm_hip_memset(void* d_dst, int value, size_t bytes) {
    if (!bytes) return ok();
    API_BEGIN_DEV(device_for(d_dst, 1))
    HIP_TRY(hipMemsetAsync(d_dst, value, bytes, c.stream));
    c.sync_or_defer();
    API_END
}

// ---- deferred-synchronisation scope ---------------------------------------------------------------------
// One lane stays bound to the calling thread between _begin and _end; the thread's calls on device-resident operands
// (snarkvm_hip_ntt_device[_batch], snarkvm_hip_fr_* with on_device = 1) are enqueued on that lane's stream and return at once,
// small host results (the remainder of fr_divide_by_linear) are delivered by _end.  How a prover that keeps its polynomials in HBM
// issues a whole round - or the same round of many proofs in lock step - without a stream synchronisation per call (~40 us each
// on this stack: 45 transforms per proof).  Calls that leave the scope's lane (MSMs, host buffers) wait for the scope first.
static constexpr uint32_t SCOPE_FLAGS_ALL = SNARKVM_HIP_SCOPE_ASYNC_MSM | SNARKVM_HIP_SCOPE_STABLE_INPUTS | SNARKVM_HIP_SCOPE_MSM_IN_STREAM;
RustError snarkvm_hip_scope_begin_ex(const void* d_any, uint32_t flags) {
    API_TRY
    thread_scope_t& sc = tl_scope();
    if (sc.lane) throw hip_failure{hipErrorInvalidValue, "scope_begin: the calling thread already has an open scope", __LINE__};
    if (flags & ~SCOPE_FLAGS_ALL) throw hip_failure{hipErrorInvalidValue, "scope_begin: unknown flag", __LINE__};
    g_rt.configure();
    const int nd = (int)g_rt.devs.size();
    int dev = device_for(d_any, d_any ? 1 : 0);
    if (dev < 0) dev = (int)(g_rt.rr.fetch_add(1) % (uint32_t)nd);
    device_t* d = g_rt.devs[dev].get();
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = 0;
    lane_t* l = d->take_for_scope(true);  // waits while the GPU's scopes hold SCOPE_LANES_MAX lanes
    try {
        HIP_TRY(hipSetDevice(d->physical));
        d->init();
        tu_kernel_attributes(d->logical);
    } catch (...) {
        d->give(l, true);
        (void)hipSetDevice(prev);
        throw;
    }
    l->begin_call();
    l->in_scope = true;
    l->pin_used = 0;
    l->scope_events_used = 0;
    sc = thread_scope_t();
    sc.lane = l;
    sc.prev_device = prev;
    sc.flags = flags;
    API_CATCH
}
RustError snarkvm_hip_scope_begin(const void* d_any) { return snarkvm_hip_scope_begin_ex(d_any, 0); }
void* snarkvm_hip_scope_stream(void) {
    lane_t* l = tl_scope().lane;
    return l ? (void*)l->stream : nullptr;
}
RustError snarkvm_hip_scope_set_flags(uint32_t flags) {
    API_TRY
    thread_scope_t& sc = tl_scope();
    if (!sc.lane) throw hip_failure{hipErrorInvalidValue, "scope_set_flags: the calling thread has no open scope", __LINE__};
    if (flags & ~SCOPE_FLAGS_ALL) throw hip_failure{hipErrorInvalidValue, "scope_set_flags: unknown flag", __LINE__};
    sc.flags = flags;  // applies to the calls that follow; what is enqueued stays where it is
    API_CATCH
}
RustError snarkvm_hip_scope_collect(const void* out) {
    API_TRY
    scope_collect(out);
    API_CATCH
}
RustError snarkvm_hip_scope_end(void) {
    thread_scope_t& sc = tl_scope();
    lane_t* l = sc.lane;
    if (!l) return ok();
    RustError r = ok();
    try {
        scope_flush();
    } catch (const hip_failure& f) {
        r = from_failure(f);
    } catch (const std::exception& e) {
        r = fail(1, std::string("snarkvm_hip: scope_end: ") + e.what());
    } catch (...) {
        r = fail(1, "snarkvm_hip: scope_end failed");
    }
    l->in_scope = false;
    l->deferred.clear();
    l->deferred_bytes = 0;
    for (int i = 0; i < sc.naux; i++) {
        (void)hipStreamSynchronize(sc.aux[i]->stream);  // (already idle unless the flush failed half-way)
        sc.aux[i]->dev->give(sc.aux[i], true);
    }
    const int prev = sc.prev_device;
    sc = thread_scope_t();
    l->dev->give(l, true);
    if (prev >= 0) (void)hipSetDevice(prev);
    return r;
}

// ---- registered bases ---------------------------------------------------------------------------------
// One replica per logical device (msm_registered.hip.h::bases_build).  Host source: every device uploads and converts for itself.  Device source:
// the owner converts and precomputes, the other devices receive the finished tables by peer copies.
static void register_bases_impl(snarkvm_hip_bases_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int on_device, int tables,
                                int table_bits) {
    if (!handle) throw hip_failure{hipErrorInvalidValue, "register_bases: null handle", __LINE__};
    if (npoints && !points) throw hip_failure{hipErrorInvalidValue, "register_bases: null points", __LINE__};
    if (ffi_affine_sz < 104 || (ffi_affine_sz & 7)) throw hip_failure{hipErrorInvalidValue, "register_bases: bad stride", __LINE__};
    check_tables(tables, table_bits, "register_bases");
    scope_flush();  // device-resident points may come out of the caller's open scope; the per-device workers of the build are other threads
    if (!table_bits) table_bits = 256 / tables;
    if (on_device)
        *handle = bases_build<fq_t>(
            npoints, tables, table_bits, [&](lane_t& c, g1_aff_mem_t* table0) { convert_bases<fq_t>(c, (const uint8_t*)points, ffi_affine_sz, npoints, table0); },
            points);
    else
        *handle = bases_build<fq_t>(npoints, tables, table_bits,
                                    [&](lane_t& c, g1_aff_mem_t* table0) { bases_fill_from_host<fq_t>(c, points, npoints, ffi_affine_sz, table0); });
}
RustError snarkvm_hip_register_bases(snarkvm_hip_bases_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int on_device) {
    API_TRY
    register_bases_impl(handle, points, npoints, ffi_affine_sz, on_device, 1, 0);
    API_CATCH
}
RustError snarkvm_hip_register_bases_tables(snarkvm_hip_bases_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int on_device,
                                            int tables) {
    API_TRY
    register_bases_impl(handle, points, npoints, ffi_affine_sz, on_device, tables, 0);
    API_CATCH
}
RustError snarkvm_hip_register_bases_windowed(snarkvm_hip_bases_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int on_device,
                                              int tables, int window_bits) {
    API_TRY
    if (window_bits <= 0) throw hip_failure{hipErrorInvalidValue, "register_bases_windowed: window_bits must be positive", __LINE__};
    register_bases_impl(handle, points, npoints, ffi_affine_sz, on_device, tables, window_bits);
    API_CATCH
}
void snarkvm_hip_free_bases(snarkvm_hip_bases_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}

// ---- MSM over registered bases ----------------------------------------------------------------------------
static void check_window_bits(int window_bits, const char* who) {
    if (!msm_window_bits_ok(window_bits)) throw std::runtime_error(std::string(who) + ": window_bits must be 0 or 2..23");
}
RustError snarkvm_hip_msm_registered(void* out, const snarkvm_hip_bases_t* h, size_t offset, size_t npoints, const void* scalars,
                                     int scalars_on_device, int window_bits) {
    API_TRY
    if (!h || offset + npoints > h->n) throw hip_failure{hipErrorInvalidValue, "msm_registered: range exceeds the registered bases", __LINE__};
    check_window_bits(window_bits, "msm_registered");
    if (!out || (npoints && !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_registered: null argument", __LINE__};
    msm_req_t one;
    one.off0 = offset, one.n0 = npoints, one.scalars = scalars, one.out = out;
    msm_registered_single<fq_t>(*h, one, scalars_on_device, 0, window_bits, true);
    API_CATCH
}
RustError snarkvm_hip_msm_registered_ex(void* out, const snarkvm_hip_bases_t* h, size_t off0, size_t n0, size_t off1, size_t n1,
                                        const void* scalars, int scalars_on_device, int scalars_montgomery, int window_bits) {
    API_TRY
    if (!h || off0 + n0 > h->n || off1 + n1 > h->n) throw hip_failure{hipErrorInvalidValue, "msm_registered_ex: range exceeds the registered bases", __LINE__};
    check_window_bits(window_bits, "msm_registered_ex");
    if (!out || ((n0 + n1) && !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_registered_ex: null argument", __LINE__};
    msm_req_t one;
    one.off0 = off0, one.n0 = n0, one.off1 = n1 ? off1 : 0, one.n1 = n1, one.scalars = scalars, one.out = out;
    msm_registered_single<fq_t>(*h, one, scalars_on_device, scalars_montgomery, window_bits, true);
    API_CATCH
}

// A batch of independent MSMs (the commitments of a batch of proofs) fanned out over devices x lanes.  Host scalars:
// instance k goes to device k mod ndev; device scalars: to the device that owns them.  On each device the instances cycle
// over several lanes, so the latency-bound tail of one overlaps the accumulation of the next; the host finishes instance k
// (Horner over its bit planes) as soon as its planes have arrived, while the GPU works on the later instances.
RustError snarkvm_hip_msm_registered_batch(void* outs, const snarkvm_hip_bases_t* h, size_t count, const size_t* offsets, const size_t* npoints,
                                           const void* const* scalars, int scalars_on_device, int scalars_montgomery, int window_bits) {
    API_TRY
    if (!h) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: null handle", __LINE__};
    check_window_bits(window_bits, "msm_registered_batch");
    if (count && (!outs || !offsets || !npoints || !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: null argument", __LINE__};
    std::vector<msm_req_t> req = msm_requests<fq_t>(outs, count, offsets, npoints, nullptr, nullptr, scalars);
    msm_batch_dispatch<fq_t>(*h, req, scalars_on_device, scalars_montgomery, window_bits);
    API_CATCH
}

// The same with two base ranges per instance (KZG10::commit with hiding / SonicKZG10::commit's degree-bounded polynomials:
// instance k = bases [off0[k], + n0[k]) then [off1[k], + n1[k]), n0 + n1 consecutive scalars).
RustError snarkvm_hip_msm_registered_batch_ex(void* outs, const snarkvm_hip_bases_t* h, size_t count, const size_t* off0, const size_t* n0,
                                              const size_t* off1, const size_t* n1, const void* const* scalars, int scalars_on_device,
                                              int scalars_montgomery, int window_bits) {
    API_TRY
    if (!h) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch_ex: null handle", __LINE__};
    check_window_bits(window_bits, "msm_registered_batch_ex");
    if (count && (!outs || !off0 || !n0 || !off1 || !n1 || !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch_ex: null argument", __LINE__};
    std::vector<msm_req_t> req = msm_requests<fq_t>(outs, count, off0, n0, off1, n1, scalars);
    msm_batch_dispatch<fq_t>(*h, req, scalars_on_device, scalars_montgomery, window_bits);
    API_CATCH
}

}  // extern "C"

// the opt-in cache of host ranges seen twice.  Included HERE because it registers such a range through register_bases_impl and releases it through
// snarkvm_hip_free_bases, both defined above (the header declares them).
#include "base_cache.hip.h"

extern "C" {

// STATELESS by default, like the reference's symbol; with the base cache on (base_cache.hip.h), a host range passed a second time is registered and served
// from its tables
RustError snarkvm_msm(void* out, const void* points, size_t npoints, const void* scalars, size_t ffi_affine_sz) {
    API_TRY
    if (!out) throw hip_failure{hipErrorInvalidValue, "msm: null output", __LINE__};
    g_rt.configure();  // no device: an error, never a silent host result
    if (npoints == 0) {
        write_infinity<fq_t>(out);
    } else {
        if (!points || !scalars) throw hip_failure{hipErrorInvalidValue, "msm: null argument", __LINE__};
        base_cache_use u;
        if (base_cache_tables() && npoints > 1024 && ffi_affine_sz >= 104 && !(ffi_affine_sz & 7)) u = base_cache_lookup(points, npoints, ffi_affine_sz);
        if (u.h && u.shadow)
            msm_cached_verified(out, u, points, npoints, scalars, ffi_affine_sz);
        else if (u.h && msm_coalescible(*u.h, npoints, 0))
            msm_single_coalesced(out, u.h.get(), u.offset, npoints, 0, 0, scalars, 0, 0, 0);
        else if (u.h)
            msm_registered_host_scalars(out, u.h.get(), u.offset, npoints, 0, 0, scalars, 0, 0);
        else
            msm_host_chunked<fq_t>(out, points, npoints, scalars, ffi_affine_sz);
    }
    API_CATCH
}

RustError snarkvm_hip_g1_sum(void* out, const void* in_projective, size_t n) {
    API_BEGIN
    if (!out || (n && !in_projective)) throw hip_failure{hipErrorInvalidValue, "g1_sum: null argument", __LINE__};
    if (n == 0) {
        write_infinity<fq_t>(out);
    } else {
        c.poly[0].ensure(n * 144 + 144);
        uint32_t* d_in = c.poly[0].as<uint32_t>();
        uint32_t* d_out = d_in + 36 * n;
        HIP_TRY(hipMemcpyAsync(d_in, in_projective, n * 144, hipMemcpyHostToDevice, c.stream));
        hipLaunchKernelGGL(g1_sum_kernel, dim3(1), dim3(64), 0, c.stream, (const uint32_t*)d_in, n, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, d_out, 144, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}
RustError snarkvm_hip_g1_to_affine(void* out_affine, const void* in_projective, size_t n) {
    API_BEGIN
    if (n) {
        if (!out_affine || !in_projective) throw hip_failure{hipErrorInvalidValue, "g1_to_affine: null argument", __LINE__};
        c.poly[0].ensure(n * 144);
        c.poly[1].ensure(n * 104);
        HIP_TRY(hipMemcpyAsync(c.poly[0].p, in_projective, n * 144, hipMemcpyHostToDevice, c.stream));
        hipLaunchKernelGGL(g1_to_affine_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, c.poly[0].as<uint32_t>(), c.poly[1].as<uint32_t>(), n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_affine, c.poly[1].p, n * 104, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}

// ---- synthetic bases ---------------------------------------------------------------------------
RustError snarkvm_hip_g1_generate_bases_device(void* d_out, uint64_t start, size_t npoints) {
    API_BEGIN_DEV(device_for(d_out, npoints ? 1 : 0))
    if (npoints) {
        const g1_aff_t g = g1_generator();  // converted on the host with the same arithmetic
        g1_aff_mem_t gm;
        g.x.pack(gm.x.w);
        g.y.pack(gm.y.w);
        c.gen_pts.ensure(npoints * sizeof(g1_xyzz_mem_t));
        c.gen_prod.ensure(npoints * sizeof(fq_mem_t));
        const size_t threads = (npoints + GEN_RUN - 1) / GEN_RUN;
        hipLaunchKernelGGL(g1_generate_bases_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c.stream, gm, start, npoints,
                           (uint8_t*)d_out, (size_t)104, c.gen_pts.as<g1_xyzz_mem_t>(), c.gen_prod.as<fq_mem_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}

}  // extern "C"
