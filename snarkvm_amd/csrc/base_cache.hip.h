#pragma once
// base_cache.hip.h - the opt-in base cache of `snarkvm_msm` (api.hip, the only unit that includes this): the host thread pool of its verification, the
// cache of registered host ranges, a verified hit, and the three snarkvm_hip_*base_cache* entry points.  Host code only, and never a translation unit of
// its own: a second unit that called msm_run<fq_t> would compile the G1 MSM kernels a second time.  Needs register_bases_impl of api.hip.
#include "msm_registered.hip.h"

// what this header needs of the unit that includes it (api.hip defines both in front of the include)
static void register_bases_impl(snarkvm_hip_bases_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int on_device, int tables, int table_bits);
extern "C" void snarkvm_hip_free_bases(snarkvm_hip_bases_t* h);

// ---- the reference's FFI MSM (host bases + host scalars) -----------------------------------------------------------------
// `snarkvm_msm` is STATELESS by default, like the reference's symbol (the callee must not retain the caller's
// pointers): bases and scalars are uploaded, converted and summed on every call and nothing is remembered after return.
//
// Opt-in base cache (SNARKVM_HIP_BASE_CACHE=1 / 2 / 4 / 8 / 16 | verified | verified:1 / 2 / 4 / 8 / 16; an EXTENSION with its own
// contract): the reference's callers pass slices of ONE long-lived vector (`powers_of_beta_g[lz .. lz + len]`,
// kzg10/mod.rs:117-119).  With the cache on, a host range that is passed a SECOND time - the same address and length - is
// registered (converted, with precomputed tables, on every device) from the memory of THAT call, and later calls whose base
// range lies inside it skip the upload, the conversion and most of the Horner chain.  Host memory is only ever read inside the
// slice the current call passed.  A registration that fails (HBM exhausted) marks the entry do-not-retry and the call takes the
// stateless path.  SNARKVM_HIP_BASE_CACHE_MB caps the device bytes per device (default 65536); least recently used ranges go first.
// Two modes:
// - sampled (the numeric values): a hit is verified against raw copies of every CACHE_STEP-th point of the requested slice (a
//   slice > 1024 points always contains at least 16 of them); a mismatch drops the entry.  The contract the caller accepts by
//   setting the variable: the vector is immutable and outlives the process's use of it (true of an SRS; not checkable from here).
// - verified: the registration also copies the 97 payload bytes (x, y, infinity; never Rust's 7 padding bytes) of every point
//   into a host shadow, and EVERY hit compares its whole slice with it on the verification pool while the cached MSM runs on the
//   device; a mismatch drops the entry and the call is computed on the stateless path, so the result always reflects the bytes
//   passed in and the caller promises nothing.  SNARKVM_HIP_BASE_CACHE_HOST_MB caps the shadow bytes (default 4096) in the
//   same LRU as the device bytes; a range whose shadow does not fit is not cached.
// Switching between the two modes drops every entry.
// Callers that can change their code should use snarkvm_hip_register_bases* + snarkvm_hip_msm_registered* instead.

// A small pool of host threads for the byte comparison of verified hits and the shadow copy of a registration.  Its size is
// SNARKVM_HIP_VERIFY_THREADS (default 4, clamped to 1..16), never the machine's core count (a process may be confined to
// fewer cores than it sees); the thread that waits for a job takes chunks of it too, so a job finishes even without the pool.
struct host_job_t {
    std::function<void(host_job_t&, size_t)> fn;  // chunk index -> work; captures nothing of the submitter's stack
    size_t nchunks = 0;
    std::atomic<size_t> next{0}, done{0};
    std::atomic<bool> flag{false};     // verification: some chunk differed (later chunks skip their work)
    std::atomic<uint64_t> bytes{0};    // verification: bytes compared
    std::mutex mu;
    std::condition_variable cv;
    void work() {
        for (size_t k; (k = next.fetch_add(1)) < nchunks;) {
            fn(*this, k);
            if (done.fetch_add(1) + 1 == nchunks) {
                std::lock_guard<std::mutex> lk(mu);
                cv.notify_all();
            }
        }
    }
    void wait() {  // take the chunks nobody has claimed yet, then wait for the ones in flight
        work();
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done.load() == nchunks; });
    }
};
class host_pool_t {
public:
    explicit host_pool_t(int threads) {
        for (int i = 0; i < threads; i++) std::thread([this] { loop(); }).detach();
    }
    void submit(const std::shared_ptr<host_job_t>& j) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(j);
        }
        cv_.notify_all();
    }

private:
    void loop() {
        for (;;) {
            std::shared_ptr<host_job_t> j;  // a worker keeps the job alive while it touches it
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !q_.empty(); });
                j = q_.front();
                if (j->next.load() >= j->nchunks) {  // every chunk claimed: the job leaves the queue
                    q_.pop_front();
                    continue;
                }
            }
            j->work();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::shared_ptr<host_job_t>> q_;
};
static int verify_threads() {
    const char* s = getenv("SNARKVM_HIP_VERIFY_THREADS");
    const int t = s ? atoi(s) : 4;
    return t < 1 ? 1 : t > 16 ? 16 : t;
}
static host_pool_t& verify_pool() {
    static host_pool_t* p = new host_pool_t(verify_threads());  // never destroyed: its detached threads outlive static destruction
    return *p;
}
static constexpr size_t PAYLOAD = 97, VERIFY_CHUNK = 4096;  // x (48) + y (48) + infinity (1); points per pool chunk
// the payload of n points at `host` (stride bytes apart) equals n consecutive 97-byte records at `shadow`
static bool payload_equal(const uint8_t* host, size_t stride, const uint8_t* shadow, size_t n) {
    uint64_t diff = 0;
    for (size_t i = 0; i < n; i++, host += stride, shadow += PAYLOAD) {
        for (int w = 0; w < 12; w++) {
            uint64_t a, b;
            memcpy(&a, host + 8 * w, 8);
            memcpy(&b, shadow + 8 * w, 8);
            diff |= a ^ b;
        }
        diff |= (uint64_t)(host[96] ^ shadow[96]);
    }
    return diff == 0;
}
struct host_shadow_t {
    std::unique_ptr<uint8_t[]> b;  // n records of PAYLOAD bytes
    size_t n = 0;
};

struct base_cache_entry {
    const uint8_t* host = nullptr;
    size_t n = 0, stride = 0;
    std::shared_ptr<snarkvm_hip_bases> h;  // null: seen once, not registered yet (shared: a running call keeps a dropped entry's tables alive)
    std::vector<uint8_t> samples;     // sampled mode: 97 bytes (x, y, infinity) of points 0, CACHE_STEP, 2 * CACHE_STEP, ...
    std::shared_ptr<const host_shadow_t> shadow;  // verified mode, registered: every point's payload (shared: like `h`, for a running compare)
    bool verified = false;            // remembered in verified mode
    uint64_t last_use = 0;
    bool failed = false;              // registration failed once (out of memory): never retried
    size_t bytes() const { return h ? (size_t)h->tables * h->n * sizeof(g1_aff_mem_t) : 0; }
    size_t host_bytes() const { return shadow ? shadow->n * PAYLOAD : 0; }
};
static constexpr size_t CACHE_STEP = 64, CACHE_MAX = 8;
static constexpr int CACHE_VERIFIED = 0x100;  // mode bit beside the table count
static std::mutex g_cache_mu;
static std::vector<base_cache_entry> g_base_cache;
static uint64_t g_cache_tick = 0;
// lookups, hits, registrations, verification mismatches, bytes compared, microseconds waited for a comparison
static std::atomic<uint64_t> g_bc_stats[6];
static std::atomic<int> g_base_cache_override{-1};  // snarkvm_hip_set_base_cache*: >= 0 replaces the environment's value
// "4" -> 4, "verified" -> 16 | CACHE_VERIFIED, "verified:4" -> 4 | CACHE_VERIFIED (an invalid count is caught by base_cache_tables)
static int base_cache_parse(const char* s) {
    if (!s) return 0;
    if (strncmp(s, "verified", 8) == 0) {
        if (s[8] == 0) return 16 | CACHE_VERIFIED;
        if (s[8] == ':' && s[9] >= '0' && s[9] <= '9') return (atoi(s + 9) & 0xff) | CACHE_VERIFIED;
        return 0;
    }
    return atoi(s);
}
static int base_cache_mode() {
    static const int env = base_cache_parse(getenv("SNARKVM_HIP_BASE_CACHE"));  // off unless asked for
    const int o = g_base_cache_override.load(std::memory_order_relaxed);
    return o >= 0 ? o : env;
}
static int base_cache_tables() {
    const int t = base_cache_mode() & ~CACHE_VERIFIED;
    return (t == 1 || t == 2 || t == 4 || t == 8 || t == 16) ? t : 0;
}
static bool base_cache_verified() { return base_cache_tables() && (base_cache_mode() & CACHE_VERIFIED); }
static size_t base_cache_cap() {
    static const size_t mb = getenv("SNARKVM_HIP_BASE_CACHE_MB") ? (size_t)atoll(getenv("SNARKVM_HIP_BASE_CACHE_MB")) : 65536;
    return mb << 20;
}
static size_t base_cache_host_cap() {
    static const size_t mb = getenv("SNARKVM_HIP_BASE_CACHE_HOST_MB") ? (size_t)atoll(getenv("SNARKVM_HIP_BASE_CACHE_HOST_MB")) : 4096;
    return mb << 20;
}
static void base_cache_drop(size_t i) { g_base_cache.erase(g_base_cache.begin() + (long)i); }
// every sampled point of [off, off + npoints) still equals its raw copy
static bool samples_match(const base_cache_entry& e, size_t off, size_t npoints) {
    if (!npoints) return false;
    const size_t k0 = (off + CACHE_STEP - 1) / CACHE_STEP, k1 = (off + npoints - 1) / CACHE_STEP;  // sample indices inside the slice
    if (k0 > k1) return false;                                                                     // no sample inside: cannot vouch for it
    for (size_t k = k0; k <= k1; k++)
        if (memcmp(&e.samples[k * 97], e.host + k * CACHE_STEP * e.stride, 97) != 0) return false;
    return true;
}
// first sighting (under g_cache_mu): remember the range (a bigger range supersedes the ranges it contains)
static void base_cache_remember(const uint8_t* p, size_t npoints, size_t stride, bool verified) {
    for (size_t i = g_base_cache.size(); i-- > 0;)
        if (g_base_cache[i].stride == stride && g_base_cache[i].host >= p && g_base_cache[i].host + g_base_cache[i].n * stride <= p + npoints * stride)
            base_cache_drop(i);
    while (g_base_cache.size() >= CACHE_MAX) {
        size_t lru = 0;
        for (size_t i = 1; i < g_base_cache.size(); i++)
            if (g_base_cache[i].last_use < g_base_cache[lru].last_use) lru = i;
        base_cache_drop(lru);
    }
    base_cache_entry e;
    e.host = p;
    e.n = npoints;
    e.stride = stride;
    e.verified = verified;
    if (!verified)
        for (size_t k = 0; k * CACHE_STEP < e.n; k++) e.samples.insert(e.samples.end(), e.host + k * CACHE_STEP * e.stride, e.host + k * CACHE_STEP * e.stride + 97);
    e.last_use = ++g_cache_tick;
    g_base_cache.push_back(std::move(e));
}
struct base_cache_use {
    std::shared_ptr<snarkvm_hip_bases> h;         // null: use the uncached path this time
    std::shared_ptr<const host_shadow_t> shadow;  // non-null: a verified-mode hit, the slice must still be compared with it
    size_t offset = 0;
};
// registered handle + offset covering [points, points + npoints * stride)
static base_cache_use base_cache_lookup(const void* points, size_t npoints, size_t stride) {
    base_cache_use u;
    const bool verified = base_cache_verified();
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_bc_stats[0]++;
    for (size_t i = g_base_cache.size(); i-- > 0;)  // entries of the other mode (a switch raced with this call) are never used
        if (g_base_cache[i].verified != verified) base_cache_drop(i);
    const uint8_t* p = (const uint8_t*)points;
    for (size_t i = 0; i < g_base_cache.size(); i++) {
        if (g_base_cache[i].stride != stride || p < g_base_cache[i].host || p + npoints * stride > g_base_cache[i].host + g_base_cache[i].n * stride ||
            (size_t)(p - g_base_cache[i].host) % stride)
            continue;
        const size_t off = (size_t)(p - g_base_cache[i].host) / stride;
        if (!verified && !samples_match(g_base_cache[i], off, npoints)) {  // the memory behind the range changed: forget it
            base_cache_drop(i);
            break;
        }
        g_base_cache[i].last_use = ++g_cache_tick;
        if (!g_base_cache[i].h) {
            // second sighting.  Only the memory of THIS call may be read: the range is registered when the call passes exactly
            // the remembered range (every sample of it was just verified above); a sub-slice of a range that is not registered
            // yet takes the stateless path.
            if (g_base_cache[i].failed || off != 0 || npoints != g_base_cache[i].n) return u;
            // table geometry by size, as measured (profiles/r02_size_sweep.md, r04_geometry_23.md): 12 x 22-bit windows from 2^24 points, 13 x 20-bit from
            // 2^21, 17 x 15-bit below 2^18 (half the buckets of 16 x 16: the whole fold is one round of 256 workgroups), else the
            // configured count of 256 / tables-bit tables
            int tables = base_cache_tables(), bits = 0;
            if (tables == 16 && g_base_cache[i].n >= ((size_t)1 << 24)) tables = 12, bits = 22;  // 2^23: 13 x 20 is 4 % faster (profiles/r04_geometry_23.md)
            else if (tables == 16 && g_base_cache[i].n >= ((size_t)1 << 21)) tables = 13, bits = 20;
            else if (tables == 16 && g_base_cache[i].n < ((size_t)1 << 18)) tables = 17, bits = 15;
            const size_t need = (size_t)tables * g_base_cache[i].n * sizeof(g1_aff_mem_t), need_host = verified ? npoints * PAYLOAD : 0;
            if (need > base_cache_cap() || need_host > base_cache_host_cap()) return u;
            for (;;) {  // make room: least recently used registered entries go first (device and shadow bytes alike)
                size_t used = 0, used_host = 0, lru = (size_t)-1;
                for (size_t j = 0; j < g_base_cache.size(); j++) {
                    used += g_base_cache[j].bytes();
                    used_host += g_base_cache[j].host_bytes();
                    if (j != i && g_base_cache[j].h && (lru == (size_t)-1 || g_base_cache[j].last_use < g_base_cache[lru].last_use)) lru = j;
                }
                if ((used + need <= base_cache_cap() && used_host + need_host <= base_cache_host_cap()) || lru == (size_t)-1) break;
                base_cache_drop(lru);
                if (lru < i) i--;
            }
            std::shared_ptr<host_shadow_t> shadow;
            snarkvm_hip_bases_t* nh = nullptr;
            try {
                if (verified) {  // the payload of this call's memory, copied on the verification pool
                    shadow = std::make_shared<host_shadow_t>();
                    shadow->b.reset(new uint8_t[npoints * PAYLOAD]);
                    shadow->n = npoints;
                    auto job = std::make_shared<host_job_t>();
                    job->nchunks = (npoints + VERIFY_CHUNK - 1) / VERIFY_CHUNK;
                    uint8_t* dst = shadow->b.get();
                    job->fn = [p, dst, npoints, stride](host_job_t&, size_t k) {
                        const size_t lo = k * VERIFY_CHUNK, hi = lo + VERIFY_CHUNK < npoints ? lo + VERIFY_CHUNK : npoints;
                        for (size_t j = lo; j < hi; j++) memcpy(dst + j * PAYLOAD, p + j * stride, PAYLOAD);
                    };
                    verify_pool().submit(job);
                    job->wait();
                }
                register_bases_impl(&nh, points, npoints, stride, 0, tables, bits);
            } catch (...) {  // nothing leaks (register_bases_impl frees its replicas); this call and later ones go stateless
                (void)hipGetLastError();
                g_base_cache[i].failed = true;
                return u;
            }
            g_base_cache[i].h = std::shared_ptr<snarkvm_hip_bases>(nh, [](snarkvm_hip_bases* b) { snarkvm_hip_free_bases(b); });
            g_base_cache[i].shadow = shadow;
            g_bc_stats[2]++;
        } else if (verified) {
            u.shadow = g_base_cache[i].shadow;  // counted as a hit once the comparison agrees
        } else {
            g_bc_stats[1]++;
        }
        u.offset = off;
        u.h = g_base_cache[i].h;
        return u;
    }
    base_cache_remember(p, npoints, stride, verified);
    return u;
}

// A verified hit: the comparison of the caller's slice with the shadow runs on the pool while the cached MSM runs on the device into
// a temporary; the result is only handed out if every byte agreed.  Otherwise the entry goes, the slice is remembered as a first
// sighting, and the call is computed from the bytes passed in on the stateless path.
static void msm_cached_verified(void* out, const base_cache_use& u, const void* points, size_t npoints, const void* scalars, size_t stride) {
    auto job = std::make_shared<host_job_t>();
    job->nchunks = (npoints + VERIFY_CHUNK - 1) / VERIFY_CHUNK;
    const uint8_t* host = (const uint8_t*)points;
    const std::shared_ptr<const host_shadow_t> keep = u.shadow;
    const size_t off = u.offset;
    job->fn = [host, keep, off, npoints, stride](host_job_t& j, size_t k) {
        if (j.flag.load(std::memory_order_relaxed)) return;
        const size_t lo = k * VERIFY_CHUNK, cnt = lo + VERIFY_CHUNK < npoints ? VERIFY_CHUNK : npoints - lo;
        if (payload_equal(host + lo * stride, stride, keep->b.get() + (off + lo) * PAYLOAD, cnt))
            j.bytes.fetch_add(cnt * PAYLOAD, std::memory_order_relaxed);
        else
            j.flag.store(true, std::memory_order_relaxed);
    };
    verify_pool().submit(job);
    alignas(16) uint8_t res[144];
    try {
        if (msm_coalescible(*u.h, npoints, 0))
            msm_single_coalesced(res, u.h.get(), u.offset, npoints, 0, 0, scalars, 0, 0, 0);
        else
            msm_registered_host_scalars(res, u.h.get(), u.offset, npoints, 0, 0, scalars, 0, 0);
    } catch (...) {
        job->flag.store(true);  // the job reads the caller's memory: never return before it has finished
        job->wait();
        throw;
    }
    const double t_ready = host_now_ms();
    job->wait();
    g_bc_stats[5] += (uint64_t)((host_now_ms() - t_ready) * 1e3);
    g_bc_stats[4] += job->bytes.load();
    if (!job->flag.load()) {
        memcpy(out, res, 144);
        g_bc_stats[1]++;
        return;
    }
    g_bc_stats[3]++;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (size_t i = 0; i < g_base_cache.size(); i++)
            if (g_base_cache[i].h == u.h) {
                base_cache_drop(i);
                break;
            }
        if (base_cache_verified()) base_cache_remember(host, npoints, stride, true);
    }
    msm_host_chunked<fq_t>(out, points, npoints, scalars, stride);
}

extern "C" {

// The API form of SNARKVM_HIP_BASE_CACHE (a host that cannot set the environment before the library is loaded; A/B runs in one process).
// 0, and every switch between the sampled and the verified mode, drops every cached range (calls in flight keep the tables they hold
// until they return).
static RustError base_cache_set(int tables, bool verified, const char* who) {
    if (!(tables == 0 || tables == 1 || tables == 2 || tables == 4 || tables == 8 || tables == 16))
        return fail(1, std::string(who) + ": tables must be 0, 1, 2, 4, 8 or 16");
    const bool was_verified = base_cache_verified();
    g_base_cache_override.store(tables | (verified && tables ? CACHE_VERIFIED : 0), std::memory_order_relaxed);
    if (tables == 0 || was_verified != base_cache_verified()) {
        std::vector<base_cache_entry> drop;
        {
            std::lock_guard<std::mutex> lk(g_cache_mu);
            drop.swap(g_base_cache);
        }
        // the entries' tables are freed here, outside the lock (hipFree waits for the device)
    }
    return ok();
}
RustError snarkvm_hip_set_base_cache(int tables) { return base_cache_set(tables, false, "snarkvm_hip_set_base_cache"); }
RustError snarkvm_hip_set_base_cache_verified(int tables) { return base_cache_set(tables, true, "snarkvm_hip_set_base_cache_verified"); }
void snarkvm_hip_base_cache_stats(uint64_t* out, int reset) {
    for (int i = 0; i < 6; i++) {
        if (out) out[i] = g_bc_stats[i].load();
        if (reset) g_bc_stats[i].store(0);
    }
    if (out) {
        out[6] = (uint64_t)base_cache_tables();
        out[7] = base_cache_verified() ? 1 : 0;
    }
}

}  // extern "C"
