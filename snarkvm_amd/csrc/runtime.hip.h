#pragma once
// runtime.hip.h - host runtime shared by the translation units of the backend (api*.hip, compiled in parallel by snarkvm_amd/build.py):
// errors, device / pinned buffers, lanes, devices, the per-thread scope, lane_guard and the API_* frame of an exported function.  Everything
// here is header-only (static / inline / templates) except the one context object, which api.hip defines.  It includes only the kernel
// header whose types a device stores by value (ntt.hip.h: the twiddle tables); what runs ON a lane lives with its kernels - one MSM:
// msm_run.hip.h, many MSMs: msm_batch.hip.h - and every unit includes what it launches.
//
// Host runtime = what algorithms/cuda/cuda/snarkvm.cu:73-312 (snarkvm_t) and snarkvm_api.cu:23-84 are in the
// reference: a lazily constructed per-process context (device arenas, stream, twiddle tables), staging of the
// caller's host buffers, error reporting as RustError, serialisation of concurrent callers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/snarkvm_hip.h"
#include "ff.hip.h"
#include "ntt.hip.h"

using namespace sv;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static RustError ok() { return RustError{0, nullptr}; }
static RustError fail(int code, const std::string& msg) {
    char* m = (char*)malloc(msg.size() + 1);
    if (m) memcpy(m, msg.c_str(), msg.size() + 1);
    return RustError{code ? code : 1, m};
}
struct hip_failure {
    hipError_t e;
    const char* what;
    int line;
};
#define HIP_TRY(x)                                             \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) throw hip_failure{_e, #x, __LINE__}; \
    } while (0)
static RustError from_failure(const hip_failure& f) {
    char buf[512];
    snprintf(buf, sizeof buf, "snarkvm_hip: %s failed at api.hip:%d: %s", f.what, f.line, hipGetErrorString(f.e));
    return fail((int)f.e, buf);
}

static double host_now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// ------------------------------------------------------------------------------------------------
// runtime: devices, lanes (the reference's (dev, stream) resource tokens), staging buffers
// ------------------------------------------------------------------------------------------------
// Workspace growth is the one thing in the library that synchronises the whole device behind the caller's back (hipFree waits for
// every stream): counted, so that a caller - or a test - can see that a timed region allocated nothing
// (snarkvm_hip_alloc_stats: {device allocations, device bytes, pinned allocations, pinned bytes, microseconds inside them}).
void sv_alloc_note(int slot, size_t bytes, double ms);  // api.hip: the process-wide counters (this header is compiled into four units)
// A buffer that is outgrown in the middle of a call is not freed on the spot: hipFree returns only when EVERY stream of the device is
// idle (measured: 281 ms behind ~280 ms of kernels queued on another stream, tools/tables1_cliff.py), i.e. the second instance of a
// pipelined batch would only be enqueued after the first one had finished, and a caller on another lane would stall behind this one.
// The old block goes to a list of the calling thread and is released by sv_drain_frees() when that thread's call ends (lane_t::end_call, scope flush),
// or at once when an allocation fails.  Inside a long scope an outgrown block therefore stays allocated beside its replacement until the flush.  (Round 4's "tables1" bench leg had six such frees inside its timed region; whether they were what
// the driver's 93.6 ms per step came from could not be reproduced - profiles/r05_summary.md.)
void sv_defer_free(void* p);
void sv_drain_frees();
struct alloc_timer_t {
    double t0;
    int slot;
    size_t bytes;
    alloc_timer_t(int s, size_t b) : t0(host_now_ms()), slot(s), bytes(b) {}
    ~alloc_timer_t() { sv_alloc_note(slot, bytes, host_now_ms() - t0); }
};
struct dev_buf {
    void* p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes) {  // on the CURRENT device (a lane guard has selected it)
        if (bytes <= cap) return;
        size_t want = bytes + bytes / 8 + 256;
        alloc_timer_t timer(0, want);
        if (p) sv_defer_free(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, want) != hipSuccess) {  // out of memory with outgrown blocks still parked: release them and try once more
            (void)hipGetLastError();
            p = nullptr;
            sv_drain_frees();
            const hipError_t e = hipMalloc(&p, want);
            if (e != hipSuccess) {  // still out of memory: the call fails, the lane stays usable (no error left behind for its next call)
                (void)hipGetLastError();
                p = nullptr;
                throw hip_failure{e, "hipMalloc", __LINE__};
            }
        }
        cap = want;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};
struct pinned_buf {  // page-locked host staging (the reference's per-GPU pinned arena, snarkvm.cu:51,123-151)
    void* p = nullptr;
    size_t cap = 0;
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        size_t want = bytes + bytes / 8 + 4096;
        alloc_timer_t timer(2, want);
        if (p) HIP_TRY(hipHostFree(p));
        p = nullptr;
        cap = 0;
        HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

struct phase_rec {
    const char* name;
    hipEvent_t e0, e1;
    double ms;
};
struct device_t;

// One lane = one HIP stream of one device with every scratch buffer a call needs: what a `(dev, stream)` token of the
// reference's resource channel stands for (snarkvm.cu:84,146-150).  A caller owns a lane for the duration of one API call;
// concurrent callers (rayon workers: one commitment each, sonic_pc/mod.rs:203-245) get different lanes / devices.
struct lane_t {
    device_t* dev = nullptr;
    int index = 0;
    hipStream_t stream = nullptr;
    // MSM workspace
    dev_buf scalars, digits, counts, offsets, scan_tmp, sorted, boff, cnt_a, cnt_b, start_a, start_b, part_a, part_b, part_raw, planes;
    dev_buf rv1, rl1, rcounts2, roff2, rbinstart, rntiles, rtstart, rbsize;  // radix-partition sort (msm_sort.hip.h)
    dev_buf rv2, rl2, rmid_size, rmid_boff;                                   // its middle level (wide windows)
    dev_buf fold_sums;                                                        // two-axis bucket fold
    dev_buf tail_flags;                                                       // Fq2 tail: outputs whose tree met equal x coordinates (recomputed by the fix kernels)
    dev_buf sink_acc;                                                         // bucket sink of a chunked MSM (msm_bucket_sink_t)
    dev_buf fchunk;                                                           // chunk sums / offsets of the fused level-1 scan
    dev_buf bases_tmp, scalars_tmp, gen_pts, gen_prod;
    // NTT / polynomial staging
    dev_buf ntt_data, ntt_scratch, ntt_acc, ntt_alt;
    dev_buf serde_status;  // one u32 of SERDE_* bits (serde.hip.h)
    dev_buf poly[5];       // staging / scratch of the prover-round vector kernels (poly.hip.h)
    pinned_buf pin, pin2;  // host staging: MSM bit-plane sums / chunked uploads
    hipStream_t alt = nullptr;  // second stream of the lane: copies of operand k + 1 while operand k is transformed (polynomial.cuh:136-242)
    hipEvent_t ev[4] = {};
    std::vector<void*> tw_leases;  // twiddle tables this call pinned in the device's cache
    // deferred-synchronisation scope (snarkvm_hip_scope_begin): the owning thread's device-resident calls are only enqueued
    bool in_scope = false;
    struct deferred_out_t {
        void* dst;
        size_t off, bytes;
    };
    std::vector<deferred_out_t> deferred;  // host results parked in pin2 until the scope ends
    size_t deferred_bytes = 0;
    // a lane owned by a scope (its main lane or one of its MSM lanes): `pin` is handed out piecewise to the MSMs the scope has enqueued
    // (bit planes + instance tables stay where they are until the scope's flush has collected them), events that must outlive a call
    size_t pin_used = 0;
    std::vector<hipEvent_t> scope_events;
    size_t scope_events_used = 0;
    hipEvent_t scope_event() {
        if (scope_events_used == scope_events.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            scope_events.push_back(e);
        }
        return scope_events[scope_events_used++];
    }
    // profiling
    std::vector<phase_rec> phases;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;

    hipEvent_t new_event() {
        if (events_used == event_pool.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            event_pool.push_back(e);
        }
        return event_pool[events_used++];
    }
    inline ntt_ctx_t ntt_ctx(hipStream_t st = nullptr);
    inline void begin_call();
    inline void phase_begin(const char* name);
    inline void phase_end();
    inline void phase_host(const char* name, double ms);
    inline void end_call();
    // the end of a call whose results all live in device memory: wait, unless the calling thread deferred that to its scope's end
    void sync_or_defer() {
        if (!in_scope) HIP_TRY(hipStreamSynchronize(stream));
    }
    // a small host result (<= a few KB) of a call that may run inside a scope: copied now and waited for, or parked in pinned
    // memory and delivered by snarkvm_hip_scope_end
    // may_defer = false: the call itself waits for the stream (host operands), so the value must be in `dst` when it returns
    void host_result(void* dst, const void* d_src, size_t bytes, bool may_defer = true) {
        if (!in_scope || !may_defer) {
            HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, stream));
            return;
        }
        if (deferred_bytes + bytes > pin2.cap) {
            if (!deferred.empty()) flush_scope();  // staging full: deliver what is parked, then start over
            pin2.ensure(deferred_bytes + bytes > (size_t)1 << 16 ? deferred_bytes + bytes : (size_t)1 << 16);
        }
        HIP_TRY(hipMemcpyAsync(pin2.as<uint8_t>() + deferred_bytes, d_src, bytes, hipMemcpyDeviceToHost, stream));
        deferred.push_back({dst, deferred_bytes, bytes});
        deferred_bytes += (bytes + 15) & ~(size_t)15;
    }
    inline void flush_scope();
};

struct device_t {
    int logical = 0, physical = 0;
    bool ready = false;
    std::mutex init_mu;
    ntt_tables_t tb{};
    dev_buf tables_mem;
    ntt_tw_cache_t tw;
    static constexpr int LANES = 16;  // streams are created up front; a lane's buffers only when it is first used
    lane_t lane[LANES];
    // token pool
    std::mutex mu;
    std::condition_variable cv;
    uint32_t busy = 0;
    // lanes held by deferred-synchronisation scopes (for as long as the scope is open).  At most SCOPE_LANES_MAX of them: four lanes of
    // every device always belong to calls that return their lane when they return, so a thread that waits for a lane - the ninth
    // scope_begin, a call on another device from inside a scope, the per-device worker threads of a multi-GPU call - waits for
    // something that ends (round-4 review: eight scopes that each issued an MSM held all eight lanes and waited for a ninth).
    static constexpr int SCOPE_LANES_MAX = LANES - 4;
    int scope_held = 0;

    void init() {  // the calling thread has this device current
        std::lock_guard<std::mutex> lk(init_mu);
        if (ready) return;
        // A scope hands its asynchronous MSMs - the work that is NOT on the caller's critical path: the independent G2 MSM of a proof, commitments whose results
        // are only due at scope_end - to the upper half of the lanes (take_for_scope searches from the top); ordinary calls and the scopes' own lanes take from the
        // bottom.  Every lane has the same kind of stream: a low priority or a compute-unit mask for the upper half was measured and retired (HISTORY.md).
        for (int l = 0; l < LANES; l++) {
            lane[l].dev = this;
            lane[l].index = l;
            HIP_TRY(hipStreamCreateWithFlags(&lane[l].stream, hipStreamNonBlocking));
            HIP_TRY(hipStreamCreateWithFlags(&lane[l].alt, hipStreamNonBlocking));
            for (auto& e : lane[l].ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        // tables: 4 x (lo + hi) x NTT_TW_SIZE + 2 x NTT_LOCAL + 4 x NTT_TOP + size_inv[NTT_LG_MAX + 1] + 4 constants, 32 B each
        static_assert(NTT_LG_MAX + 1 <= 32, "size_inv");
        const size_t entries = 8 * NTT_TW_SIZE + 2 * NTT_LOCAL + 4 * NTT_TOP + 32 + 8;
        tables_mem.ensure(entries * sizeof(fr_mem_t));
        fr_mem_t* base = tables_mem.as<fr_mem_t>();
        size_t off = 0;
        auto take = [&](size_t n) {
            fr_mem_t* r = base + off;
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
        hipStream_t st = lane[0].stream;
        hipLaunchKernelGGL(ntt_setup_consts, dim3(1), dim3(64), 0, st, tb);
        hipLaunchKernelGGL(ntt_fill_tables, dim3(NTT_TW_SIZE / 256), dim3(256), 0, st, tb);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        ready = true;
    }
    // lowest free lanes, up to `want` (at least one: blocks until a lane is free); returns the number taken
    int take(lane_t** out, int want) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return busy != (1u << LANES) - 1; });
        int got = 0;
        for (int l = 0; l < LANES && got < want; l++)
            if (!(busy & (1u << l))) {
                busy |= 1u << l;
                out[got++] = &lane[l];
            }
        return got;
    }
    bool try_take(lane_t** out) {
        std::lock_guard<std::mutex> lk(mu);
        for (int l = 0; l < LANES; l++)
            if (!(busy & (1u << l))) {
                busy |= 1u << l;
                *out = &lane[l];
                return true;
            }
        return false;
    }
    // n lanes (<= want) without waiting; 0 when none is free
    int try_take_n(lane_t** out, int want) {
        std::lock_guard<std::mutex> lk(mu);
        int got = 0;
        for (int l = 0; l < LANES && got < want; l++)
            if (!(busy & (1u << l))) {
                busy |= 1u << l;
                out[got++] = &lane[l];
            }
        return got;
    }
    // a lane for a scope: block = the scope's main lane (waits for a free lane AND for room under the cap); else an extra MSM lane, only if
    // one is free right now
    lane_t* take_for_scope(bool block) {
        std::unique_lock<std::mutex> lk(mu);
        auto room = [&] { return busy != (1u << LANES) - 1 && scope_held < SCOPE_LANES_MAX; };
        if (block)
            cv.wait(lk, room);
        else if (!room())
            return nullptr;
        // a scope's own lane: from the bottom (normal priority); its further MSM lanes: from the top (low-priority streams, see init)
        for (int i = 0; i < LANES; i++) {
            const int l = block ? i : LANES - 1 - i;
            if (!(busy & (1u << l))) {
                busy |= 1u << l;
                scope_held++;
                return &lane[l];
            }
        }
        return nullptr;
    }
    void give(lane_t* l, bool from_scope = false) {
        {
            std::lock_guard<std::mutex> lk(mu);
            busy &= ~(1u << l->index);
            if (from_scope) scope_held--;
        }
        cv.notify_all();  // waiters wait on different conditions (a free lane / room under the scope cap)
    }
};

// The process-wide runtime: the set of devices in use (the reference's `ngpus()` loop, snarkvm.cu:123-151), chosen by
// snarkvm_hip_set_devices / SNARKVM_HIP_DEVICES (default: every visible device).  A physical device may be listed more than
// once: each entry is an independent logical device (own streams, workspaces, base replicas) - how the multi-device paths
// are exercised on a one-GPU box.
struct runtime_t {
    std::mutex cfg_mu;
    std::vector<int> want;  // physical ids requested (empty: default)
    std::vector<std::unique_ptr<device_t>> devs;
    bool configured = false;
    std::atomic<uint32_t> rr{0};
    // profiling: phases of the most recent profiled call (any lane)
    std::atomic<bool> profiling{false};
    std::mutex prof_mu;
    std::vector<std::pair<std::string, double>> last_phases;

    void configure() {
        std::lock_guard<std::mutex> lk(cfg_mu);
        if (configured) return;
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) throw hip_failure{e == hipSuccess ? hipErrorNoDevice : e, "hipGetDeviceCount (no MI355X visible)", __LINE__};
        std::vector<int> ids = want;
        if (ids.empty()) {
            if (const char* env = getenv("SNARKVM_HIP_DEVICES")) {
                for (const char* p = env; *p;) {
                    char* end = nullptr;
                    long v = strtol(p, &end, 10);
                    if (end == p) break;
                    ids.push_back((int)v);
                    p = (*end == ',') ? end + 1 : end;
                }
            }
        }
        if (ids.empty())
            for (int d = 0; d < ndev; d++) ids.push_back(d);
        for (int id : ids)
            if (id < 0 || id >= ndev) throw hip_failure{hipErrorInvalidDevice, "device index out of range (snarkvm_hip_set_devices / SNARKVM_HIP_DEVICES)", __LINE__};
        for (size_t i = 0; i < ids.size(); i++) {
            devs.emplace_back(new device_t());
            devs.back()->logical = (int)i;
            devs.back()->physical = ids[i];
        }
        configured = true;
    }
    int ndev() {
        configure();
        return (int)devs.size();
    }
    // logical device that owns a device pointer (-1: not a device pointer of a configured device)
    int device_of(const void* ptr) {
        configure();
        hipPointerAttribute_t at;
        if (!ptr || hipPointerGetAttributes(&at, ptr) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        std::vector<int> match;
        for (auto& d : devs)
            if (d->physical == at.device) match.push_back(d->logical);
        if (match.empty()) return -1;
        return match[rr.fetch_add(1) % match.size()];
    }
};
extern runtime_t g_rt;  // defined in api.hip

// Per-(translation unit, device) kernel attributes: kernels with more than 64 KB of dynamic LDS need the attribute on THEIR
// function object; the non-template kernels are static, i.e. every unit launches its own copy.  Every api*.hip unit defines
// tu_set_kernel_attributes() once: the hipFuncSetAttribute calls for the kernels IT launches (an empty body when there are none).
static void tu_set_kernel_attributes();
static void tu_kernel_attributes(int logical) {
    static std::mutex mu;
    static std::vector<char> done;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)done.size() <= logical) done.resize(logical + 1, 0);
    if (done[logical]) return;
    tu_set_kernel_attributes();
    done[logical] = 1;
}

// RAII ownership of lanes.  Selecting a lane makes its device current on the calling thread (the HIP current device is per
// host thread - rayon workers!) and restores the previous one on release.
// Deferred-synchronisation scope of the calling thread (snarkvm_hip_scope_begin / _end): one lane stays bound to the thread; its
// device-resident calls borrow that lane and return after the enqueue.  Anything that takes OTHER lanes (host-buffer MSMs, another
// device) first waits for the scope's work - what it reads may have been produced inside the scope - and then runs on the scope's own
// lane (plus whatever further lanes are free right now): a thread inside a scope never waits for a lane.
// SNARKVM_HIP_SCOPE_ASYNC_MSM: MSMs over registered bases with device-resident scalars are enqueued as well - on up to SCOPE_AUX_MAX
// further lanes of the scope, in turn, each behind an event of the scope's stream - and their host finishes (the Horner chain over the
// bit planes) run when the scope is flushed.
static constexpr int SCOPE_AUX_MAX = 7;  // one proof: six commitment rounds + the G2 MSM, every one on its own stream
struct scope_pending_t {
    hipEvent_t done;               // everything the finish reads has arrived in pinned memory
    std::function<void()> finish;  // host Horner chains -> the callers' `out` buffers
    const void* tag;               // the first `out` pointer of the call that enqueued it (snarkvm_hip_scope_collect(out))
};
struct thread_scope_t {
    lane_t* lane = nullptr;
    int prev_device = -1;
    unsigned flags = 0;
    lane_t* aux[SCOPE_AUX_MAX] = {};
    int naux = 0;
    unsigned aux_rr = 0;
    bool aux_exhausted = false;  // a try for a further lane failed: not tried again in this scope
    std::vector<scope_pending_t> pending;
    thread_scope_t() = default;
    thread_scope_t(const thread_scope_t&) = default;
    thread_scope_t& operator=(const thread_scope_t&) = default;
    ~thread_scope_t();  // a thread that ends with its scope open gives the lanes back (api.hip)
};
// ONE object per thread for the whole library: defined in api.hip.  (Rounds 3-4 kept it as a function-local static of this header,
// i.e. one copy per translation unit: a scope opened by api.hip was invisible to the transforms and vector passes of api_fr.hip and
// to the G2 calls of api_g2.hip - they took another lane and waited for it call by call, unordered against the scope's stream.)
extern thread_local thread_scope_t g_tl_scope;
static thread_scope_t& tl_scope() { return g_tl_scope; }
// wait for everything the calling thread's scope has enqueued; deliver the results it owes (MSM outputs, parked host values)
static void scope_flush() {
    thread_scope_t& sc = tl_scope();
    if (!sc.lane) return;
    std::exception_ptr err;
    // in enqueue order: the host finishes of the early MSMs run while the GPU still works on the later ones
    for (scope_pending_t& p : sc.pending) {
        try {
            HIP_TRY(hipEventSynchronize(p.done));
            p.finish();
        } catch (...) {
            if (!err) err = std::current_exception();
        }
    }
    sc.pending.clear();
    try {
        sc.lane->flush_scope();
        for (int i = 0; i < sc.naux; i++) HIP_TRY(hipStreamSynchronize(sc.aux[i]->stream));
    } catch (...) {
        if (!err) err = std::current_exception();
    }
    sc.lane->pin_used = 0;
    sc.lane->scope_events_used = 0;
    for (int i = 0; i < sc.naux; i++) sc.aux[i]->pin_used = 0, sc.aux[i]->scope_events_used = 0;
    if (err) std::rethrow_exception(err);
}
// the outputs of the MSM call that was given `tag` as its (first) output - or, tag == nullptr, of every MSM the scope has enqueued so far
// (snarkvm_hip_scope_collect): the scope stays open, its own stream is not waited for, the other pending MSMs stay pending
static void scope_collect(const void* tag) {
    thread_scope_t& sc = tl_scope();
    if (!sc.lane) return;
    std::exception_ptr err;
    if (tag) {
        // While this thread would only WAIT for `tag`'s results, it delivers what has already arrived for the others (a proof in transcript order: the independent
        // G2 MSM issued first is ready two or three rounds later - its Horner chain over Fq2, ~0.15 ms of host time, then runs under a commitment round's kernels
        // instead of behind the last round at scope_end).  Only while the wanted results are not there yet: they are never delayed by more than one such finish.
        auto ready = [](const scope_pending_t& p) {
            const hipError_t e = hipEventQuery(p.done);
            if (e == hipSuccess) return true;
            (void)hipGetLastError();  // (hipErrorNotReady is an answer, not a failure: it must not surface in a later launch check)
            return false;
        };
        auto wanted_ready = [&]() {
            for (const scope_pending_t& p : sc.pending)
                if (p.tag == tag && !ready(p)) return false;
            return true;
        };
        for (size_t i = 0; i < sc.pending.size() && !wanted_ready();) {
            if (sc.pending[i].tag != tag && ready(sc.pending[i])) {
                try {
                    sc.pending[i].finish();
                } catch (...) {
                    if (!err) err = std::current_exception();
                }
                sc.pending.erase(sc.pending.begin() + (ptrdiff_t)i);
            } else {
                i++;
            }
        }
    }
    std::vector<scope_pending_t> keep;
    for (scope_pending_t& p : sc.pending) {
        if (tag && p.tag != tag) {
            keep.push_back(std::move(p));
            continue;
        }
        try {
            HIP_TRY(hipEventSynchronize(p.done));
            p.finish();
        } catch (...) {
            if (!err) err = std::current_exception();
        }
    }
    sc.pending.swap(keep);
    if (sc.pending.empty()) {
        // nothing of an enqueued MSM is in flight any more: the staging areas and the events can be handed out again - on the MSM lanes (an MSM is
        // the only work they get) and on the scope's own lane (its events were "inputs ready" marks for those MSMs, or, without a free MSM lane, the
        // MSMs' own "done" marks; parked host values live in pin2, not in pin)
        sc.lane->pin_used = 0, sc.lane->scope_events_used = 0;
        for (int i = 0; i < sc.naux; i++) sc.aux[i]->pin_used = 0, sc.aux[i]->scope_events_used = 0;
    }
    if (err) std::rethrow_exception(err);
}
struct lane_guard {
    std::vector<lane_t*> lanes;
    int prev_device = -1;
    bool borrowed = false;        // every lane belongs to the thread's scope (nothing to give back)
    bool first_borrowed = false;  // lanes[0] is the scope's lane, the others are ours
    lane_guard() {}
    lane_guard(const lane_guard&) = delete;
    // one lane on logical device `dev`, or on the least busy device when dev < 0
    explicit lane_guard(int dev) {
        lane_t* sl = tl_scope().lane;
        if (sl && (dev < 0 || (dev < (int)g_rt.devs.size() && g_rt.devs[dev]->physical == sl->dev->physical))) {  // inside the thread's scope: its lane, its device is already current
            borrowed = true;
            lanes.push_back(sl);
            tu_kernel_attributes(sl->dev->logical);  // this unit's kernels may not have run on the device yet (the scope was opened by api.hip)
            return;
        }
        acquire(dev, 1);
    }
    void acquire(int dev, int want) {
        scope_flush();
        g_rt.configure();
        const int nd = (int)g_rt.devs.size();
        if (dev >= nd) throw hip_failure{hipErrorInvalidDevice, "logical device index out of range", __LINE__};
        if (lane_t* sl = tl_scope().lane) {
            if (dev < 0 || g_rt.devs[dev]->physical == sl->dev->physical) {
                // the scope's own lane (idle now) serves as the first lane of this call; more only if they are free right now
                lanes.push_back(sl);
                first_borrowed = true;
                tu_kernel_attributes(sl->dev->logical);
                lane_t* more[device_t::LANES];
                const int n = want > 1 ? sl->dev->try_take_n(more, want - 1) : 0;
                for (int i = 0; i < n; i++) lanes.push_back(more[i]);
                return;
            }
        }
        if (prev_device < 0 && hipGetDevice(&prev_device) != hipSuccess) prev_device = 0;
        device_t* d = nullptr;
        lane_t* got[device_t::LANES];
        int n = 0;
        if (dev >= 0) {
            d = g_rt.devs[dev].get();
        } else {
            const uint32_t s = g_rt.rr.fetch_add(1);
            for (int i = 0; i < nd && !d; i++) {  // first device (round-robin start) with a free lane
                device_t* cand = g_rt.devs[(s + i) % nd].get();
                if (want == 1) {
                    if (cand->try_take(&got[0])) {
                        d = cand;
                        n = 1;
                    }
                } else {
                    d = cand;
                }
            }
            if (!d) d = g_rt.devs[s % nd].get();
        }
        if (!n) n = d->take(got, want);
        try {  // a failure below must not leak the tokens: the destructor of a throwing constructor never runs
            HIP_TRY(hipSetDevice(d->physical));
            d->init();
            tu_kernel_attributes(d->logical);
        } catch (...) {
            for (int i = 0; i < n; i++) d->give(got[i]);
            if (prev_device >= 0) (void)hipSetDevice(prev_device);
            throw;
        }
        for (int i = 0; i < n; i++) lanes.push_back(got[i]);
    }
    lane_t& c() { return *lanes[0]; }
    ~lane_guard() {
        if (borrowed) return;
        for (size_t i = first_borrowed ? 1 : 0; i < lanes.size(); i++) lanes[i]->dev->give(lanes[i]);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
};

inline ntt_ctx_t lane_t::ntt_ctx(hipStream_t st) { return ntt_ctx_t{st ? st : stream, &dev->tb, &dev->tw, &tw_leases}; }
inline void lane_t::begin_call() {
    phases.clear();
    events_used = 0;
}
inline void lane_t::phase_begin(const char* name) {
    if (!g_rt.profiling.load(std::memory_order_relaxed)) return;
    phase_rec r{name, new_event(), new_event(), 0.0};
    HIP_TRY(hipEventRecord(r.e0, stream));
    phases.push_back(r);
}
inline void lane_t::phase_end() {
    if (!g_rt.profiling.load(std::memory_order_relaxed) || phases.empty()) return;
    HIP_TRY(hipEventRecord(phases.back().e1, stream));
}
inline void lane_t::phase_host(const char* name, double ms) {  // a phase that ran on the calling thread (no events)
    if (!g_rt.profiling.load(std::memory_order_relaxed)) return;
    phases.push_back(phase_rec{name, nullptr, nullptr, ms});
}
static void ntt_tw_release(device_t* dev, std::vector<void*>& leases) { ntt_tw_release_entries(dev->tw, leases); }
inline void lane_t::flush_scope() {  // wait for everything the scope has enqueued, deliver parked host results, return the twiddle leases
    HIP_TRY(hipStreamSynchronize(stream));
    for (const deferred_out_t& d : deferred) memcpy(d.dst, pin2.as<uint8_t>() + d.off, d.bytes);
    deferred.clear();
    deferred_bytes = 0;
    if (!tw_leases.empty()) ntt_tw_release(dev, tw_leases);
    sv_drain_frees();
}
inline void lane_t::end_call() {
    if (in_scope) return;  // nothing is waited for; leases are held until the scope ends
    sv_drain_frees();
    if (!tw_leases.empty()) {
        HIP_TRY(hipStreamSynchronize(stream));
        ntt_tw_release(dev, tw_leases);
    }
    if (phases.empty()) return;
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<std::pair<std::string, double>> out;
    for (auto& r : phases) {
        if (r.e0) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, r.e0, r.e1));
            r.ms = ms;
        }
        out.emplace_back(r.name, r.ms);
    }
    std::lock_guard<std::mutex> lk(g_rt.prof_mu);
    g_rt.last_phases.swap(out);
}

// fn(logical device) on every listed device: inline for one device, one host thread per device otherwise (the reference's
// per-GPU `pool.spawn`, snarkvm.cu:262).  The first exception is rethrown on the caller's thread.
template <class Fn>
static void for_each_device(const std::vector<int>& devices, Fn fn) {
    if (devices.size() <= 1) {
        for (int d : devices) fn(d);
        return;
    }
    std::vector<std::thread> th;
    std::vector<std::exception_ptr> errs(devices.size());
    for (size_t i = 0; i < devices.size(); i++)
        th.emplace_back([&, i] {
            try {
                fn(devices[i]);
            } catch (...) {
                errs[i] = std::current_exception();
            }
        });
    for (auto& t : th) t.join();
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);
}

// fn(i) for i < n on up to `max_threads` host threads (the calling thread is one of them).  Used for the Horner finishes of a fused
// group: 25 - 35 us each on one core, 64 of them per group.
template <class Fn>
static void host_parallel_for(size_t n, int max_threads, Fn fn) {
    size_t T = n / 4;
    if (T > (size_t)max_threads) T = (size_t)max_threads;
    if (T <= 1) {
        for (size_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<size_t> next{0};
    std::vector<std::exception_ptr> errs(T);
    auto work = [&](size_t t) {
        try {
            for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
        } catch (...) {
            errs[t] = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
    for (auto& e : errs)
        if (e) std::rethrow_exception(e);
}

// ------------------------------------------------------------------------------------------------
// exported-function scaffolding
// ------------------------------------------------------------------------------------------------
// API_BEGIN: take one lane on any device;  API_BEGIN_DEV(d): on logical device d (d < 0: any).  `c` is the lane.
#define API_BEGIN_DEV(devsel)                      \
    try {                                          \
        lane_guard _lg(devsel);                    \
        lane_t& c = _lg.c();                       \
        c.begin_call();
#define API_BEGIN API_BEGIN_DEV(-1)
// API_TRY / API_CATCH: the frame of a function that manages its lanes itself;  API_END closes API_BEGIN: the lane's call ends, same handlers
#define API_TRY try {
#define API_CATCH                                  \
    return ok();                                   \
    }                                              \
    catch (const hip_failure& f) {                 \
        return from_failure(f);                    \
    }                                              \
    catch (const std::exception& e) {              \
        return fail(1, std::string("snarkvm_hip: ") + e.what()); \
    }                                              \
    catch (...) {                                  \
        return fail(1, "snarkvm_hip: unknown error"); \
    }
#define API_END   \
    c.end_call(); \
    API_CATCH
// logical device for a call whose operands live in device memory (on_device != 0): the owner of `ptr`
static int device_for(const void* ptr, int on_device) {
    if (!on_device || !ptr) return -1;
    const int d = g_rt.device_of(ptr);
    if (d < 0) throw hip_failure{hipErrorInvalidValue, "device pointer does not belong to a device in use (snarkvm_hip_set_devices)", __LINE__};
    return d;
}
