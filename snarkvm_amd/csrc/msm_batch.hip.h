#pragma once
// msm_batch.hip.h - many MSMs: registered base vectors (bases_handle_t), the lane ring and the chunked host-buffer MSM, requests, fused
// multi-instance groups, batches over devices x lanes, MSMs enqueued inside a scope, and the coalescer of concurrent callers.
// Builds on the single MSM of msm_run.hip.h.
#include "msm_run.hip.h"

// one MSM of a batch: bases [off0, off0 + n0) followed by [off1, off1 + n1) (KZG10's hiding range; n1 = 0: none) against n0 + n1
// consecutive scalars; `out`: where its Jacobian memory image goes
struct msm_req_t {
    size_t off0 = 0, n0 = 0, off1 = 0, n1 = 0;
    const void* scalars = nullptr;
    void* out = nullptr;
};
// a queued call of the coalescer (msm_coalesced below); bases_handle_t holds the queue
struct msm_ticket_t {
    msm_req_t req;
    int on_device = 0, montgomery = 0, window_bits = 0;
    int state = 0;  // 0 queued, 1 in flight, 2 done, 3 failed
    std::exception_ptr err;
};
// registered base vectors: one replica per logical device (every device holds its own copy of the static SRS)
template <class F>
struct bases_handle_t {
    std::vector<aff_mem_t<F>*> d;  // [logical device]: tables * n entries: table j at d + j * n holds 2^(table_bits * j) * P_i
    size_t n = 0;
    int tables = 1;
    int table_bits = 256;  // table j = 2^(table_bits * j) * P
    // tickets of concurrent callers waiting to be fused (msm_coalesced)
    mutable std::mutex co_mu;
    mutable std::condition_variable co_cv;
    mutable std::deque<msm_ticket_t*> co_q;
    mutable int co_leaders = 0;
    void free_all() {
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (size_t i = 0; i < d.size(); i++)
            if (d[i]) {
                (void)hipSetDevice(g_rt.devs[i]->physical);
                (void)hipFree(d[i]);
                d[i] = nullptr;
            }
        (void)hipSetDevice(prev);
    }
};
struct snarkvm_hip_bases : bases_handle_t<fq_t> {};
// the table geometries a registration accepts (G1 and G2 entry points)
static void check_tables(int tables, int table_bits, const char* who) {
    const bool legacy = table_bits == 0 && (tables == 1 || tables == 2 || tables == 4 || tables == 8 || tables == 16);
    // upper bound: the recoding bias holds one bit per digit row below MSM_BIAS_BITS (msm_plan_t::bias, the digit kernels' 11-word scalar)
    const bool windowed = table_bits >= 2 && table_bits <= MSM_C_MAX && tables >= 1 && tables <= 127 && tables * table_bits >= 254 &&
                          tables * table_bits <= MSM_BIAS_BITS;
    if (!legacy && !windowed)
        throw std::runtime_error(std::string(who) + ": tables must be 1, 2, 4, 8 or 16, or 254 <= tables * window_bits <= 288 with window_bits in 2..23");
}

// lanes a batch cycles through per device: more lanes hide more of the latency-bound tail of small MSMs, fewer keep the
// workspace footprint of big ones down (a 2^24 lane holds ~4 GB)
static int batch_lanes(size_t npoints) {
    const int env = tuning().lanes;
    int l = env > 0 ? env : (npoints >= ((size_t)1 << 20) ? 3 : 8);  // measured: 8 lanes +7 % below 2^20, no gain above
    return l < 1 ? 1 : (l > device_t::LANES ? device_t::LANES : l);
}
static constexpr size_t MSM_SPLIT_MIN = (size_t)1 << 18;  // pairs per device below which a point-range split costs more than it saves
static size_t msm_chunk_pairs() {  // pairs per upload / compute chunk of an MSM whose bases arrive from the host
    const int lg = tuning().msm_chunk_lg;
    return (size_t)1 << (lg < 16 ? 16 : (lg > 30 ? 30 : lg));
}
// pairs per scalar chunk of a host-scalar MSM over registered bases (tuning scalar_chunk_lg, default 2^22: the tail of
// a chunk costs < 1 ms, its upload 2.4 ms)
static size_t msm_scalar_chunk_pairs() {
    const int lg = tuning().scalar_chunk_lg;
    return (size_t)1 << (lg < 18 ? 18 : lg > 30 ? 30 : lg);
}

// `count` chunks of one call on the lanes of `lg` (a ring: chunk j uses lane j mod L).  A dedicated uploader thread runs
// upload(j, stream) - host-blocking copies of pageable caller memory - chunk after chunk, so PCIe stays busy back to back
// while the calling thread runs compute(j) (kernel launches plus the read-back that sizes the reduce rounds) for the chunks
// that have arrived.  up[j]: "chunk j is on the device" (event on the lane's second stream); used[j]: "the work of chunk j
// has consumed the lane's staging buffers" (event on the lane's stream).
template <class Upload, class Compute>
static void lane_ring_run(lane_guard& lg, size_t count, Upload&& upload, Compute&& compute, int trace, double t_begin) {
    const size_t L = lg.lanes.size();
    const int phys = lg.lanes[0]->dev->physical;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> uploaded(count, 0), enqueued(count, 0);
    std::vector<hipEvent_t> up(count), used(count);
    for (size_t j = 0; j < count; j++) {
        up[j] = lg.lanes[j % L]->new_event();
        used[j] = lg.lanes[j % L]->new_event();
    }
    std::exception_ptr up_err, cp_err;
    std::thread uploader([&] {
        try {
            HIP_TRY(hipSetDevice(phys));
            for (size_t j = 0; j < count; j++) {
                lane_t& c = *lg.lanes[j % L];
                if (j >= L) {  // the lane's previous chunk must have been consumed on the GPU
                    char state;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return enqueued[j - L] != 0; });
                        state = enqueued[j - L];
                    }
                    if (state == 2) break;  // the compute side failed
                    HIP_TRY(hipEventSynchronize(used[j - L]));
                }
                const double t0 = host_now_ms();
                upload(j, c.alt);
                HIP_TRY(hipEventRecord(up[j], c.alt));
                if (trace) fprintf(stderr, "[snarkvm_hip] chunk %zu dev %d lane %d: uploaded t+%.2f .. t+%.2f ms\n", j, c.dev->logical, c.index, t0 - t_begin, host_now_ms() - t_begin);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    uploaded[j] = 1;
                }
                cv.notify_all();
            }
        } catch (...) {
            up_err = std::current_exception();
            std::lock_guard<std::mutex> lk(mu);
            for (auto& u : uploaded) u = 2;
            cv.notify_all();
        }
    });
    try {
        for (size_t j = 0; j < count; j++) {
            lane_t& c = *lg.lanes[j % L];
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return uploaded[j] != 0; });
                if (uploaded[j] == 2) break;
            }
            HIP_TRY(hipStreamWaitEvent(c.stream, up[j], 0));
            const double t0 = host_now_ms();
            compute(j);
            HIP_TRY(hipEventRecord(used[j], c.stream));
            if (trace) fprintf(stderr, "[snarkvm_hip] chunk %zu: enqueued t+%.2f .. t+%.2f ms\n", j, t0 - t_begin, host_now_ms() - t_begin);
            {
                std::lock_guard<std::mutex> lk(mu);
                enqueued[j] = 1;
            }
            cv.notify_all();
        }
    } catch (...) {
        cp_err = std::current_exception();
        std::lock_guard<std::mutex> lk(mu);
        for (auto& e : enqueued) e = 2;
        cv.notify_all();
    }
    uploader.join();
    if (cp_err || up_err) {  // nothing of this call may still be in flight when the lanes go back to the pool
        for (lane_t* l : lg.lanes) {
            (void)hipStreamSynchronize(l->alt);
            (void)hipStreamSynchronize(l->stream);
        }
        std::rethrow_exception(cp_err ? cp_err : up_err);
    }
}

// The reference's FFI MSM (host bases, host scalars, no registration): G1: F = fq_t (stride >= 104), G2: F = fq2_t (>= 200).
// A big call is cut into point-range chunks that are dealt round-robin to the devices (the reference's per-GPU slices,
// snarkvm.cu:254-270) and, on each device, to a ring of up to three lanes: an uploader thread copies chunk after chunk into
// the lanes' staging buffers without a pause while the calling thread converts, sorts and accumulates the chunks that have
// arrived - the upload (PCIe, ~2.4 ns per pair) is the critical path and the compute (~2.4 ns per pair without precomputed
// tables) hides behind it.  Every chunk leaves only its bit-plane sums; they are added on the host before the one Horner chain.
template <class F>
static void msm_host_chunked(void* out, const void* points, size_t npoints, const void* scalars, size_t stride) {
    const size_t min_stride = 2 * sizeof(typename F::mem_t) + 8;
    if (stride < min_stride || (stride & 7)) throw hip_failure{hipErrorInvalidValue, "msm: bad ffi_affine_sz for this curve", __LINE__};
    scope_flush();  // (the per-device workers of a multi-GPU call are other threads)
    const int nd = g_rt.ndev();
    static const int trace = getenv("SNARKVM_HIP_TRACE") ? atoi(getenv("SNARKVM_HIP_TRACE")) : 0;
    const double t_begin = host_now_ms();
    size_t nchunks = npoints < 2 * MSM_SPLIT_MIN ? 1 : (npoints + msm_chunk_pairs() - 1) / msm_chunk_pairs();
    if (nchunks == 1 && npoints >= 2 * MSM_SPLIT_MIN && (nd > 1 || npoints >= ((size_t)1 << 20))) nchunks = 2;  // 2^20: 7.2 -> 7.0 ms, 2^21: 13.0 -> 12.4
    // chunk boundaries.  The upload is the critical path and nothing of the last chunk can start before its last byte has
    // arrived, so the LAST chunk is cut again into 1/2, 1/4, 1/4 (tuning taper): what is exposed after the final upload is the
    // computation of a quarter chunk plus the one tail (round 3: a whole 2^21-pair chunk, 8.4 ms of the 62 at 2^24).
    std::vector<size_t> bound;
    for (size_t i = 0; i <= nchunks; i++) bound.push_back(npoints * i / nchunks);
    const bool taper = tuning().taper != 0 && nchunks >= 3 && bound[nchunks] - bound[nchunks - 1] >= MSM_SPLIT_MIN;
    if (taper) {
        const size_t lo = bound[nchunks - 1], len = npoints - lo;
        bound.back() = lo + len / 2;
        bound.push_back(lo + len / 2 + len / 4);
        bound.push_back(npoints);
        nchunks += 2;
    }
    // ... and nothing can be computed before the FIRST chunk has arrived: at 2^24 the table-less arithmetic (16 digit rows per
    // point, ~47 ms of GPU time) outlasts the 41 ms of upload, so the 5 ms the GPU idles through the first 2^21-pair upload are 5 ms
    // of the call.  The first chunk is cut into 1/2^r, 1/2^r, 1/2^(r-1), ..., 1/2 (tuning ramp = r; pieces of >= 2^17 pairs).
    int ramp = tuning().taper != 0 && nchunks >= 2 ? tuning().ramp : 0;
    while (ramp > 0 && (bound[1] >> ramp) < ((size_t)1 << 17)) ramp--;
    if (ramp > 0) {
        const size_t len = bound[1];
        std::vector<size_t> front;
        size_t pos = len >> ramp;
        front.push_back(pos);
        for (int k = ramp; k >= 1; k--) {
            pos += len >> k;
            front.push_back(k == 1 ? len : pos);
        }
        bound.erase(bound.begin() + 1);
        bound.insert(bound.begin() + 1, front.begin(), front.end());
        nchunks += (size_t)ramp;
    }
    const int ndu = (int)(nchunks < (size_t)nd ? nchunks : (size_t)nd);
    std::unique_ptr<msm_accum_t<F>> acc(new msm_accum_t<F>());
    std::mutex acc_mu;
    std::vector<int> devs;
    if (ndu == 1)
        devs.push_back(-1);
    else
        for (int d = 0; d < ndu; d++) devs.push_back(d);
    const size_t slot = msm_plane_bytes<F>();
    for_each_device(devs, [&](int dev) {
        std::vector<size_t> mine;
        for (size_t i = (dev < 0 ? 0 : (size_t)dev); i < nchunks; i += (size_t)ndu) mine.push_back(i);
        lane_guard lg;
        const int ring = tuning().ring_lanes < 2 ? 2 : (tuning().ring_lanes > device_t::LANES ? device_t::LANES : tuning().ring_lanes);
        lg.acquire(dev, mine.size() > (size_t)ring ? ring : (int)mine.size());
        const int L = (int)lg.lanes.size();
        // Several chunks on this device: they share ONE set of buckets (16-bit windows whatever the chunk length) - every chunk
        // adds its per-bucket partial sums to a sink and the fold / bit-plane tail runs once, after the last chunk, instead of once
        // per chunk (~1.5 ms each at 2^21 pairs x 16 windows).  tuning taper=0: every chunk runs its own tail (round 3).
        const bool use_sink = tuning().taper != 0 && mine.size() >= 2;
        const int chunk_c = use_sink ? 16 : 0;
        std::vector<msm_pending_t> pend(use_sink ? 1 : mine.size());
        size_t max_cnt = 0;
        for (size_t j = 0; j < mine.size(); j++) {
            const size_t cnt = bound[mine[j] + 1] - bound[mine[j]];
            max_cnt = cnt > max_cnt ? cnt : max_cnt;
        }
        const size_t aff_bytes = (max_cnt * sizeof(aff_mem_t<F>) + 255) & ~(size_t)255;
        for (int l = 0; l < L; l++) {
            lane_t& c = *lg.lanes[l];
            c.begin_call();
            c.pin.ensure(slot * (use_sink ? 1 : (mine.size() + L - 1) / L));
            c.bases_tmp.ensure(aff_bytes + max_cnt * stride);
            c.scalars_tmp.ensure(max_cnt * 32);
        }
        msm_bucket_sink_t sink;
        hipEvent_t sink_ready = nullptr;
        if (use_sink) {
            lane_t& c0 = *lg.lanes[0];
            const msm_plan_t pl = msm_make_plan(max_cnt, chunk_c, 1, 0);
            sink.nbt = (uint32_t)pl.W * pl.nb;
            sink.L = (uint32_t)L;
            const size_t bytes = (size_t)sink.nbt * L * msm_partial_bytes<F>();
            c0.sink_acc.ensure(bytes);
            sink.acc = c0.sink_acc.p;
            HIP_TRY(hipMemsetAsync(sink.acc, 0, bytes, c0.stream));  // all-zero = the point at infinity
            sink_ready = c0.new_event();
            HIP_TRY(hipEventRecord(sink_ready, c0.stream));
            for (int l = 1; l < L; l++) HIP_TRY(hipStreamWaitEvent(lg.lanes[l]->stream, sink_ready, 0));
        }
        auto chunk_lo = [&](size_t j) { return bound[mine[j]]; };
        auto chunk_cnt = [&](size_t j) { return bound[mine[j] + 1] - bound[mine[j]]; };
        // upload of chunk j into its lane's staging buffers (host-blocking: the caller's memory is pageable)
        auto upload = [&](size_t j, hipStream_t st) {
            lane_t& c = *lg.lanes[j % L];
            uint8_t* raw = c.bases_tmp.template as<uint8_t>() + aff_bytes;
            HIP_TRY(hipMemcpyAsync(raw, (const uint8_t*)points + chunk_lo(j) * stride, chunk_cnt(j) * stride, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(c.scalars_tmp.p, (const uint8_t*)scalars + chunk_lo(j) * 32, chunk_cnt(j) * 32, hipMemcpyHostToDevice, st));
        };
        auto compute = [&](size_t j, bool prof) {
            lane_t& c = *lg.lanes[j % L];
            uint8_t* raw = c.bases_tmp.template as<uint8_t>() + aff_bytes;
            if (prof) c.phase_begin("msm_convert_bases");
            convert_bases<F>(c, raw, stride, chunk_cnt(j), c.bases_tmp.template as<aff_mem_t<F>>(), nullptr, true);
            if (prof) c.phase_end();
            msm_bucket_sink_t mine_sink = sink;
            mine_sink.slot = (uint32_t)(j % L);
            msm_job_t<F> job;
            job.bases = c.bases_tmp.template as<aff_mem_t<F>>();
            job.scalars = c.scalars_tmp.template as<uint4>();
            job.n = chunk_cnt(j);
            job.window_bits = chunk_c;
            job.host_planes = c.pin.template as<uint8_t>() + (use_sink ? 0 : slot * (j / L));
            job.profile = prof;
            job.sink = use_sink ? &mine_sink : nullptr;
            const msm_pending_t pd = msm_run<F>(c, job);
            if (!use_sink) pend[j] = pd;
        };
        if (mine.size() == 1) {
            lane_t& c = *lg.lanes[0];
            c.phase_begin("msm_h2d");
            upload(0, c.stream);
            c.phase_end();
            compute(0, true);
        } else {
            lane_ring_run(lg, mine.size(), upload, [&](size_t j) { compute(j, false); }, trace, t_begin);
        }
        if (use_sink) {  // every lane's last merge, then the one tail on lane 0
            lane_t& c0 = *lg.lanes[0];
            for (int l = 1; l < L; l++) {
                hipEvent_t e = lg.lanes[l]->new_event();
                HIP_TRY(hipEventRecord(e, lg.lanes[l]->stream));
                HIP_TRY(hipStreamWaitEvent(c0.stream, e, 0));
            }
            msm_job_t<F> tail;  // the chunks' plan: the largest chunk, no tables
            tail.n = max_cnt;
            tail.window_bits = chunk_c;
            tail.host_planes = c0.pin.p;
            pend[0] = msm_tail_from_sink<F>(c0, tail, sink);
        }
        for (int l = 0; l < L; l++) {
            HIP_TRY(hipStreamSynchronize(lg.lanes[l]->alt));
            HIP_TRY(hipStreamSynchronize(lg.lanes[l]->stream));
        }
        const double t_sync = host_now_ms();
        {
            std::lock_guard<std::mutex> lk(acc_mu);
            for (auto& pd : pend) msm_collect<F>(*acc, pd);
        }
        if (trace) fprintf(stderr, "[snarkvm_hip] all chunks done at t+%.2f ms, planes collected in %.2f ms\n", t_sync - t_begin, host_now_ms() - t_sync);
        for (int l = 0; l < L; l++) lg.lanes[l]->end_call();
    });
    acc->finish(out);
}

// A batch of independent MSMs over one registered base vector, fanned out over devices x lanes (see
// snarkvm_hip_msm_registered_batch).  Every request names its own 144 / 288-byte output (Jacobian memory image).
//
// Instances of up to 2^18 pairs over windowed tables (one bucket window per table set: the geometries registered for proof-sized
// commitments, 17 x 15 / 16 x 16 bit) are FUSED: the instances a device received travel as groups through ONE launch sequence
// each (msm_sort.hip.h: instance id = top key of the radix partition, one accumulate grid, one fold and one bit-plane launch
// for the whole group, then one host finish per instance).  A prover round is such a batch (sonic_pc/mod.rs:186-245: the
// commitments of a round are independent MSMs over one committer key).  Per instance the fused run leaves fewer partial sums
// for the tail (the accumulate grid is sized for the group, not per instance) and ~25 launches are shared by the group.
static constexpr size_t MSM_FUSE_MAX_PAIRS = (size_t)1 << 18;   // per instance
static constexpr size_t MSM_FUSE_MAX_ENTRIES = (size_t)1 << 26;  // digit entries (tables x padded pairs) per fused group
static bool msm_fuse_enabled() {
    return tuning().fuse_batch != 0;  // A/B switch
}
static size_t msm_fuse_max_k() {
    const int k = tuning().fuse_max_k;
    return (size_t)(k < 2 ? 2 : (k > 256 ? 256 : k));
}
// A job over registered bases: its bases group - request r's ranges on logical device `dev`, the handle's tables - and n = n0 + n1.
template <class F>
static msm_job_t<F> msm_handle_job(const bases_handle_t<F>& h, int dev, const msm_req_t& r) {
    msm_job_t<F> j;
    j.bases = h.d[dev] + r.off0;
    j.bases1 = r.n1 ? h.d[dev] + r.off1 : nullptr;
    j.n0 = r.n0;
    j.tables = h.tables;
    j.table_stride = h.n;
    j.table_bits = h.table_bits;
    j.n = r.n0 + r.n1;
    return j;
}
// the handle's geometry admits fused multi-instance groups: one bucket window of 12 .. 16 bits per table set, slots addressable in 31 bits
template <class F>
static bool msm_handle_fusable(const bases_handle_t<F>& h, int window_bits) {
    if (!msm_fuse_enabled() || h.tables <= 1 || h.table_bits < 12 || h.table_bits > 16 || (window_bits != 0 && window_bits != h.table_bits) ||
        (size_t)h.tables * h.n >= ((size_t)1 << 31) || h.n >= ((size_t)1 << 31))
        return false;
    const msm_plan_t pl = msm_make_plan(SORT_TILE, h.table_bits, h.tables, h.table_bits);  // what msm_run will ask of a fused group
    return pl.W == 1 && pl.c == h.table_bits;
}
// planes a fused instance leaves: two tail windows (row sums, column sums) of fold_m + 1 bits, fold_m = table_bits / 2 (msm_run)
template <class F>
static size_t msm_fuse_planes(const bases_handle_t<F>& h) {
    return 2 * ((size_t)h.table_bits / 2 + 1);
}
static size_t msm_padded(size_t n) { return (n + SORT_TILE - 1) / SORT_TILE * SORT_TILE; }
// the jobs the instances `mine` (indices into req) make on one device: fused groups of small instances (in order of appearance), single
// instances otherwise
template <class F>
static std::vector<std::vector<size_t>> msm_make_jobs(const bases_handle_t<F>& h, const msm_req_t* req, const std::vector<size_t>& mine, bool fusable_handle) {
    std::vector<std::vector<size_t>> jobs;
    std::vector<size_t> group;
    size_t group_entries = 0;
    auto flush = [&] {
        if (!group.empty()) jobs.push_back(group);  // a lone instance takes the single-MSM path (its own planner)
        group.clear();
        group_entries = 0;
    };
    for (size_t k : mine) {
        const size_t tot = req[k].n0 + req[k].n1;
        const bool small = fusable_handle && tot > 0 && tot <= MSM_FUSE_MAX_PAIRS;
        if (!small) {
            jobs.push_back({k});
            continue;
        }
        const size_t e = msm_padded(tot) * (size_t)h.tables;
        if (!group.empty() && (group.size() >= msm_fuse_max_k() || group_entries + e > MSM_FUSE_MAX_ENTRIES)) flush();
        group.push_back(k);
        group_entries += e;
    }
    flush();
    return jobs;
}
// pinned bytes job `job` needs: its bit planes, then (fused groups) its instance table
template <class F>
static void msm_job_staging(const bases_handle_t<F>& h, const std::vector<size_t>& job, size_t& plane_bytes, size_t& table_bytes) {
    const size_t K = job.size();
    plane_bytes = K > 1 ? K * msm_fuse_planes(h) * msm_point_bytes<F>() : msm_plane_bytes<F>();
    table_bytes = K > 1 ? ((K + 1) * sizeof(msm_inst_t) + 255) / 256 * 256 : 0;
}
// Enqueue job `job` on lane c (device `dev`): host_planes / tab = its pinned staging (valid until the planes have been collected).
template <class F>
static msm_pending_t msm_enqueue_job(lane_t& c, const bases_handle_t<F>& h, int dev, const msm_req_t* req, const std::vector<size_t>& job, uint8_t* host_planes,
                                     msm_inst_t* tab, int scalars_on_device, int scalars_montgomery, int window_bits, hipEvent_t scalars_read = nullptr) {
    if (job.size() == 1) {
        const msm_req_t& r = req[job[0]];
        const size_t n = r.n0 + r.n1;
        const uint4* d_sc = (const uint4*)r.scalars;
        if (!scalars_on_device && n) {
            // the lane's previous instance may still be reading its scalar buffer: stream order serialises the copy behind it
            c.scalars.ensure(n * 32);
            HIP_TRY(hipMemcpyAsync(c.scalars.p, r.scalars, n * 32, hipMemcpyHostToDevice, c.stream));
            d_sc = c.scalars.template as<uint4>();
        }
        msm_job_t<F> one = msm_handle_job(h, dev, r);
        one.scalars = d_sc;
        one.scalars_montgomery = scalars_montgomery;
        one.window_bits = window_bits;
        one.host_planes = host_planes;
        one.profile = false;
        one.scalars_read = scalars_read;
        return msm_run<F>(c, one);
    }
    // fused group: instance table (pinned -> device), scalars of host callers packed into the lane's scalar buffer
    const size_t K = job.size();
    size_t npad = 0, sc_bytes = 0;
    for (size_t q = 0; q < K; q++) sc_bytes += (req[job[q]].n0 + req[job[q]].n1) * 32;
    if (!scalars_on_device) c.scalars.ensure(sc_bytes);
    size_t sc_off = 0;
    for (size_t q = 0; q < K; q++) {
        const msm_req_t& r = req[job[q]];
        const size_t n = r.n0 + r.n1;
        msm_inst_t& in = tab[q];
        in.n = (uint32_t)n;
        in.n0 = r.n1 ? (uint32_t)r.n0 : in.n;
        in.off0 = (uint32_t)r.off0;
        in.off1 = r.n1 ? (uint32_t)r.off1 : 0u;
        in.pstart = (uint32_t)npad;
        in.ptiles = (uint32_t)(msm_padded(n) / SORT_TILE);
        npad += msm_padded(n);
        if (scalars_on_device) {
            in.scalars = (const uint4*)r.scalars;
        } else {
            uint8_t* dst = c.scalars.template as<uint8_t>() + sc_off;
            HIP_TRY(hipMemcpyAsync(dst, r.scalars, n * 32, hipMemcpyHostToDevice, c.stream));
            in.scalars = (const uint4*)dst;
            sc_off += n * 32;
        }
    }
    tab[K] = msm_inst_t{nullptr, 0, 0, 0, 0, (uint32_t)npad, 0};  // sentinel
    c.poly[4].ensure((K + 1) * sizeof(msm_inst_t));
    HIP_TRY(hipMemcpyAsync(c.poly[4].p, tab, (K + 1) * sizeof(msm_inst_t), hipMemcpyHostToDevice, c.stream));
    msm_multi_t mu;
    mu.d_inst = c.poly[4].template as<msm_inst_t>();
    mu.K = (uint32_t)K;
    mu.npad = npad;
    mu.hn = h.n;
    mu.plane_capacity = K * msm_fuse_planes(h);  // checked by msm_run BEFORE it enqueues the copy into the staging area
    msm_job_t<F> group = msm_handle_job(h, dev, msm_req_t{});  // the whole table array: the instance table names the ranges
    group.n = npad;
    group.scalars_montgomery = scalars_montgomery;
    group.host_planes = host_planes;
    group.profile = false;
    group.multi = &mu;
    group.scalars_read = scalars_read;
    return msm_run<F>(c, group);
}
// the host finish of job `job` (its planes have arrived): one Horner chain per instance, the instances of a fused group on several threads
template <class F>
static void msm_finish_job(const msm_req_t* req, const std::vector<size_t>& job, const msm_pending_t& pd, int max_threads = 8) {
    if (job.size() == 1) {
        std::unique_ptr<msm_accum_t<F>> acc(new msm_accum_t<F>());
        msm_collect<F>(*acc, pd);
        acc->finish(req[job[0]].out);
        return;
    }
    host_parallel_for(job.size(), max_threads, [&](size_t q) {
        std::unique_ptr<msm_accum_t<F>> acc(new msm_accum_t<F>());
        msm_collect_inst<F>(*acc, pd, (int)q);
        acc->finish(req[job[q]].out);
    });
}
static void msm_check_requests(size_t hn, const msm_req_t* req, size_t count) {
    for (size_t k = 0; k < count; k++) {
        if (req[k].off0 + req[k].n0 > hn || (req[k].n1 && req[k].off1 + req[k].n1 > hn))
            throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: range exceeds the registered bases", __LINE__};
        if ((req[k].n0 + req[k].n1) && !req[k].scalars) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: null scalar vector", __LINE__};
        if (!req[k].out) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: null output", __LINE__};
    }
}
template <class F>
static void msm_batch_run(const bases_handle_t<F>& h, const msm_req_t* req, size_t count, int scalars_on_device, int scalars_montgomery, int window_bits) {
    auto total = [&](size_t k) { return req[k].n0 + req[k].n1; };
    scope_flush();  // the per-device workers below are other threads: what they read must be complete (and they cannot flush this thread's scope)
    const int nd = g_rt.ndev();
    std::vector<std::vector<size_t>> per_dev(nd);
    size_t largest = 0;
    msm_check_requests(h.n, req, count);
    for (size_t k = 0; k < count; k++) {
        largest = total(k) > largest ? total(k) : largest;
        int dev = (int)(k % (size_t)nd);
        if (scalars_on_device && total(k)) {
            dev = g_rt.device_of(req[k].scalars);
            if (dev < 0) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: scalars are not on a device in use", __LINE__};
        }
        per_dev[dev].push_back(k);
    }
    const int nlanes = batch_lanes(largest);
    std::vector<int> devs;
    for (int d = 0; d < nd; d++)
        if (!per_dev[d].empty()) devs.push_back(d);
    const bool fusable_handle = msm_handle_fusable(h, window_bits);
    for_each_device(devs, [&](int dev) {
        const std::vector<std::vector<size_t>> jobs = msm_make_jobs(h, req, per_dev[dev], fusable_handle);
        lane_guard lg;
        lg.acquire(dev, nlanes < (int)jobs.size() ? nlanes : (int)jobs.size());
        const int L = (int)lg.lanes.size();
        std::vector<msm_pending_t> pend(jobs.size());
        std::vector<hipEvent_t> done(jobs.size());
        // pinned staging per lane: the bit planes of its jobs, then the instance tables of its fused jobs
        std::vector<size_t> plane_off(jobs.size()), table_off(jobs.size()), lane_bytes(L, 0);
        for (size_t i = 0; i < jobs.size(); i++) {
            size_t pb, tb;
            msm_job_staging(h, jobs[i], pb, tb);
            plane_off[i] = lane_bytes[i % L];
            table_off[i] = plane_off[i] + pb;
            lane_bytes[i % L] += pb + tb;
        }
        for (int l = 0; l < L; l++) {
            lg.lanes[l]->begin_call();
            lg.lanes[l]->pin.ensure(lane_bytes[l] ? lane_bytes[l] : 256);
        }
        for (size_t i = 0; i < jobs.size(); i++) {
            lane_t& c = *lg.lanes[i % L];
            pend[i] = msm_enqueue_job<F>(c, h, dev, req, jobs[i], c.pin.template as<uint8_t>() + plane_off[i], (msm_inst_t*)(c.pin.template as<uint8_t>() + table_off[i]),
                                         scalars_on_device, scalars_montgomery, window_bits);
            done[i] = c.new_event();
            HIP_TRY(hipEventRecord(done[i], c.stream));
        }
        // the host finishes job i while the GPU works on the later ones; the instances of a fused group on several host threads
        for (size_t i = 0; i < jobs.size(); i++) {
            HIP_TRY(hipEventSynchronize(done[i]));
            msm_finish_job<F>(req, jobs[i], pend[i]);
        }
        for (int l = 0; l < L; l++) lg.lanes[l]->end_call();
    });
}
// An MSM call of a thread inside an SNARKVM_HIP_SCOPE_ASYNC_MSM scope, scalars in the scope device's memory: the instances are only ENQUEUED -
// on the next of the scope's MSM lanes, behind everything the scope's stream has been given so far - and the scope's stream in turn waits
// until the MSM has read its scalars (the caller may reuse those buffers in its next calls).  The outputs are written by the scope's flush
// (snarkvm_hip_scope_end, or any call that has to wait for the scope).  Returns false when the call does not qualify (the caller then
// takes the synchronous path).
template <class F>
static bool msm_scope_enqueue(const bases_handle_t<F>& h, const msm_req_t* req, size_t count, int scalars_on_device, int scalars_montgomery, int window_bits) {
    thread_scope_t& sc = tl_scope();
    if (!sc.lane || !(sc.flags & SNARKVM_HIP_SCOPE_ASYNC_MSM) || !scalars_on_device || !count || g_rt.profiling.load(std::memory_order_relaxed)) return false;
    msm_check_requests(h.n, req, count);
    device_t* d = sc.lane->dev;
    for (size_t k = 0; k < count; k++) {
        if (!(req[k].n0 + req[k].n1)) continue;
        const int dk = g_rt.device_of(req[k].scalars);
        if (dk < 0) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: scalars are not on a device in use", __LINE__};
        if (g_rt.devs[dk]->physical != d->physical) return false;  // another GPU: the synchronous path sorts that out
    }
    if ((size_t)d->logical >= h.d.size() || !h.d[d->logical]) return false;
    // the lane: the scope's MSM lanes in turn; a further one is added while fewer than SCOPE_AUX_MAX are held and one is free.
    // SNARKVM_HIP_SCOPE_MSM_IN_STREAM: the scope's own lane, in order with its transforms - no event hand-off between streams (what a caller
    // wants who collects this MSM before it issues anything else: nothing could run beside it anyway)
    const bool in_stream = (sc.flags & SNARKVM_HIP_SCOPE_MSM_IN_STREAM) != 0;
    if (!in_stream && sc.naux < SCOPE_AUX_MAX && !sc.aux_exhausted && (sc.naux == 0 || sc.aux_rr >= (unsigned)sc.naux)) {
        if (lane_t* l = d->take_for_scope(false)) {
            l->begin_call();
            l->pin_used = 0;
            l->scope_events_used = 0;
            sc.aux[sc.naux++] = l;
        } else {
            sc.aux_exhausted = true;
        }
    }
    lane_t& c = (sc.naux && !in_stream) ? *sc.aux[sc.aux_rr++ % (unsigned)sc.naux] : *sc.lane;
    std::vector<size_t> all(count);
    for (size_t k = 0; k < count; k++) all[k] = k;
    const std::vector<std::vector<size_t>> jobs = msm_make_jobs(h, req, all, msm_handle_fusable(h, window_bits));
    size_t need = 0;
    for (const auto& j : jobs) {
        size_t pb, tb;
        msm_job_staging(h, j, pb, tb);
        need += pb + tb;
    }
    // a scope's staging area is at least 1 MB from its first MSM on the lane: how far `pin_used` climbs inside a scope depends on when the pending MSMs happen to be
    // delivered (scope_collect hands over what has arrived) - an area sized by other paths (a few KB of planes) would be outgrown in SOME replay of a warmed shape
    // only, with a flush of the whole scope in front of the allocation
    if (c.pin_used == 0 && c.pin.cap < ((size_t)1 << 20)) c.pin.ensure((size_t)1 << 20);
    if (c.pin_used + need > c.pin.cap) {  // staging full: collect what is pending (its planes live there), then start over with a bigger area
        if (c.pin_used) scope_flush();    // (first use of a lane: nothing of the scope is in its area - no reason to deliver other MSMs early)
        c.pin.ensure(need > ((size_t)1 << 20) ? need : (size_t)1 << 20);
    }
    // shared by the finish closures: the requests (outputs) of this call
    std::shared_ptr<std::vector<msm_req_t>> rq(new std::vector<msm_req_t>(req, req + count));
    if (&c != sc.lane) {
        hipEvent_t ready = sc.lane->scope_event();
        HIP_TRY(hipEventRecord(ready, sc.lane->stream));
        HIP_TRY(hipStreamWaitEvent(c.stream, ready, 0));
    }
    // All or nothing: a failure on job k > 0 must not leave jobs 0 .. k-1 pending - the caller sees an error and may free or reuse the `out`
    // buffers their finishes would write at scope_end.  What this call added is taken back (after the lanes have drained: the kernels already
    // enqueued write into the staging that is being handed back).
    const size_t pending0 = sc.pending.size(), pin0 = c.pin_used, ev0 = c.scope_events_used;
    try {
        for (const auto& j : jobs) {
            size_t pb, tb;
            msm_job_staging(h, j, pb, tb);
            uint8_t* planes = c.pin.template as<uint8_t>() + c.pin_used;
            msm_inst_t* tab = (msm_inst_t*)(planes + pb);
            c.pin_used += pb + tb;
            // SNARKVM_HIP_SCOPE_STABLE_INPUTS: the caller leaves the scalar vectors alone until the scope ends - the scope's stream does not wait
            hipEvent_t read = (&c != sc.lane && !(sc.flags & SNARKVM_HIP_SCOPE_STABLE_INPUTS)) ? c.scope_event() : nullptr;
            const msm_pending_t pd = msm_enqueue_job<F>(c, h, d->logical, rq->data(), j, planes, tab, 1, scalars_montgomery, window_bits, read);
            if (read) HIP_TRY(hipStreamWaitEvent(sc.lane->stream, read, 0));
            hipEvent_t done = c.scope_event();
            HIP_TRY(hipEventRecord(done, c.stream));
            sc.pending.push_back(scope_pending_t{done, [rq, j, pd] { msm_finish_job<F>(rq->data(), j, pd, 4); }, req[0].out});
        }
    } catch (...) {
        (void)hipStreamSynchronize(c.stream);
        if (&c != sc.lane) (void)hipStreamSynchronize(sc.lane->stream);
        (void)hipGetLastError();
        sc.pending.erase(sc.pending.begin() + (ptrdiff_t)pending0, sc.pending.end());
        c.pin_used = pin0;
        c.scope_events_used = ev0;  // only this call's "read" / "done" marks were taken from c's pool since ev0, and c has drained
        throw;
    }
    return true;
}
// contiguous outputs (outs + k * sizeof(Jacobian)): the batch entry points of the C ABI
template <class F>
static std::vector<msm_req_t> msm_requests(void* outs, size_t count, const size_t* off0, const size_t* n0, const size_t* off1, const size_t* n1,
                                           const void* const* scalars) {
    std::vector<msm_req_t> req(count);
    for (size_t k = 0; k < count; k++) {
        req[k].off0 = off0[k];
        req[k].n0 = n0[k];
        req[k].off1 = (n1 && n1[k]) ? off1[k] : 0;
        req[k].n1 = n1 ? n1[k] : 0;
        req[k].scalars = scalars[k];
        req[k].out = (uint8_t*)outs + sizeof(jac_mem_t<F>) * k;
    }
    return req;
}

// ---- in-library coalescing of concurrent callers ---------------------------------------------------------------------------
// The reference prover issues one MSM per polynomial from rayon workers (sonic_pc/mod.rs:186-245, kzg10/mod.rs:117-119): many
// threads inside snarkvm_hip_msm_registered* at the same time, each with ONE proof-sized instance - the shape that runs at a
// third of the fused rate when every call travels alone.  Here such calls meet: a caller whose MSM is small enough for a fused
// group (msm_handle_fusable, <= 2^18 pairs) queues a ticket on the HANDLE; whoever finds a free dispatcher slot (two per handle:
// while one batch computes, the next is being enqueued) takes every compatible ticket that is waiting and runs them as ONE
// msm_batch_run - group commit.  While a batch is in flight new arrivals pile up, so the batch size adapts to the concurrency by
// itself; a dispatcher additionally waits `coalesce_us` for stragglers when another thread called within the last 300 us (a
// rayon fan-out arrives within tens of microseconds).  A lone caller (one thread, sequential calls) never waits and runs exactly
// the launch sequence of the direct path.  Results are bit-identical to the per-instance path: the same kernels on the same
// operands, only grouped (tests/test_gpu_proofs.py::test_coalesced_*).  tuning coalesce=0 switches it off.
// Errors stay with the caller that caused them: every ticket is validated before it is queued, and when a fused batch fails as a whole
// its tickets are run again one by one, so that one caller's bad request (or a failure only the group provokes) cannot make the other
// callers fall back to their CPU paths.
// how the coalescer grouped its callers so far: {batches dispatched, tickets in them, largest batch, batches of one ticket}
extern std::atomic<uint64_t> g_co_stats[4];  // api.hip (process-wide: G1 and G2 callers)
static bool msm_other_caller_recently() {
    static std::atomic<uint64_t> last_ns{0}, last_tid{0};
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    const uint64_t now = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
    const uint64_t tid = (uint64_t)std::hash<std::thread::id>()(std::this_thread::get_id()) | 1u;
    const uint64_t pt = last_ns.exchange(now), pid = last_tid.exchange(tid);
    return pid != 0 && pid != tid && now - pt < 300000ull;
}
template <class F>
static bool msm_coalescible(const bases_handle_t<F>& h, size_t n, int window_bits) {
    return tuning().coalesce && n > 0 && n <= MSM_FUSE_MAX_PAIRS && !g_rt.profiling.load(std::memory_order_relaxed) && msm_handle_fusable(h, window_bits);
}
template <class F>
static void msm_coalesced(const bases_handle_t<F>& h, msm_ticket_t* tix, size_t count) {
    if (!count) return;
    scope_flush();  // another thread may run these tickets: what they read must be complete
    for (size_t i = 0; i < count; i++) {  // a request that cannot run never reaches the queue (it would fail the group it lands in)
        msm_check_requests(h.n, &tix[i].req, 1);
        if (tix[i].on_device && (tix[i].req.n0 + tix[i].req.n1) && g_rt.device_of(tix[i].req.scalars) < 0)
            throw hip_failure{hipErrorInvalidValue, "msm_registered: scalars are not on a device in use", __LINE__};
    }
    const bool hint = msm_other_caller_recently();
    std::unique_lock<std::mutex> lk(h.co_mu);
    for (size_t i = 0; i < count; i++) h.co_q.push_back(&tix[i]);
    auto mine_done = [&] {
        for (size_t i = 0; i < count; i++)
            if (tix[i].state < 2) return false;
        return true;
    };
    bool waited = false;
    while (!mine_done()) {
        if (h.co_leaders < tuning().coalesce_slots && !h.co_q.empty()) {
            h.co_leaders++;
            if (!waited && (hint || h.co_leaders > 1) && tuning().coalesce_us > 0) {
                waited = true;  // once per call: stragglers of the same fan-out
                h.co_cv.wait_for(lk, std::chrono::microseconds(tuning().coalesce_us));
            }
            std::vector<msm_ticket_t*> batch;
            if (!h.co_q.empty()) {
                const msm_ticket_t key = *h.co_q.front();
                std::deque<msm_ticket_t*> rest;
                for (msm_ticket_t* t : h.co_q) {
                    if (batch.size() < 1024 && t->on_device == key.on_device && t->montgomery == key.montgomery && t->window_bits == key.window_bits) {
                        t->state = 1;
                        batch.push_back(t);
                    } else {
                        rest.push_back(t);
                    }
                }
                h.co_q.swap(rest);
            }
            lk.unlock();
            std::exception_ptr err;
            std::vector<std::exception_ptr> errs;  // per ticket, after a failed group was re-run singly
            if (!batch.empty()) {
                g_co_stats[0].fetch_add(1, std::memory_order_relaxed);
                g_co_stats[1].fetch_add(batch.size(), std::memory_order_relaxed);
                if (batch.size() == 1) g_co_stats[3].fetch_add(1, std::memory_order_relaxed);
                for (uint64_t cur = g_co_stats[2].load(); cur < batch.size() && !g_co_stats[2].compare_exchange_weak(cur, batch.size());) {
                }
                try {
                    std::vector<msm_req_t> req(batch.size());
                    for (size_t i = 0; i < batch.size(); i++) req[i] = batch[i]->req;
                    msm_batch_run<F>(h, req.data(), req.size(), batch[0]->on_device, batch[0]->montgomery, batch[0]->window_bits);
                } catch (...) {
                    err = std::current_exception();
                }
                if (err && batch.size() > 1) {
                    errs.assign(batch.size(), nullptr);
                    for (size_t i = 0; i < batch.size(); i++) {
                        try {
                            msm_batch_run<F>(h, &batch[i]->req, 1, batch[i]->on_device, batch[i]->montgomery, batch[i]->window_bits);
                        } catch (...) {
                            errs[i] = std::current_exception();
                        }
                    }
                }
            }
            lk.lock();
            for (size_t i = 0; i < batch.size(); i++) {
                msm_ticket_t* t = batch[i];
                t->err = errs.empty() ? err : errs[i];
                t->state = t->err ? 3 : 2;
            }
            h.co_leaders--;
            h.co_cv.notify_all();
        } else {
            h.co_cv.wait(lk);
        }
    }
    lk.unlock();
    for (size_t i = 0; i < count; i++)
        if (tix[i].state == 3 && tix[i].err) std::rethrow_exception(tix[i].err);
}
// a batch of requests through the coalescer when every one of them qualifies, else straight to msm_batch_run
template <class F>
static void msm_batch_dispatch(const bases_handle_t<F>& h, std::vector<msm_req_t>& req, int scalars_on_device, int scalars_montgomery, int window_bits) {
    if (msm_scope_enqueue<F>(h, req.data(), req.size(), scalars_on_device, scalars_montgomery, window_bits)) return;
    bool all_small = !req.empty();
    for (const msm_req_t& r : req) {
        if (r.off0 + r.n0 > h.n || (r.n1 && r.off1 + r.n1 > h.n)) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: range exceeds the registered bases", __LINE__};
        if ((r.n0 + r.n1) && !r.scalars) throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: null scalar vector", __LINE__};
        if (scalars_on_device && (r.n0 + r.n1) && g_rt.device_of(r.scalars) < 0)
            throw hip_failure{hipErrorInvalidValue, "msm_registered_batch: scalars are not on a device in use", __LINE__};
        all_small = all_small && msm_coalescible(h, r.n0 + r.n1, window_bits);
    }
    if (!all_small) {
        msm_batch_run<F>(h, req.data(), req.size(), scalars_on_device, scalars_montgomery, window_bits);
        return;
    }
    std::vector<msm_ticket_t> tix(req.size());
    for (size_t i = 0; i < req.size(); i++) {
        tix[i].req = req[i];
        tix[i].on_device = scalars_on_device ? 1 : 0;
        tix[i].montgomery = scalars_montgomery ? 1 : 0;
        tix[i].window_bits = window_bits;
    }
    msm_coalesced<F>(h, tix.data(), tix.size());
}
