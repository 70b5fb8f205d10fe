#pragma once
// msm_registered.hip.h - the host-side front end of the registered-bases ABI, once for G1 (fq_t, api.hip / api_serde.hip) and G2 (fq2_t, api_g2.hip):
// building one replica of a base vector per logical device (bases_build) and the dispatch of ONE MSM over a registered range
// (msm_registered_single).  The entry points above it validate their arguments, with their own names in the texts, and call into here; the
// engine below it (msm_batch.hip.h, msm_run.hip.h) is a template over the field already.
//
// What still differs between the curves, and why it is kept:
//   host-scalar route      G1: msm_registered_host_scalars - a split by point range over the devices, scalar chunks whose upload hides behind the previous
//                          chunk's accumulation, one bucket sink.  G2: one upload on the lane the call holds, then msm_run_sync.  G2 vectors are proof-sized
//                          (BASELINE configs[4]); nobody has measured the chunked route over fq2_t.
//   n == 0 inside a scope  G1 hands an empty MSM to the scope's queue like any other (the point at infinity arrives with the scope's flush); G2 keeps it out and
//                          answers on return.  Callers may rely on either, so the rule is a parameter (scope_takes_empty), not a choice made here.
//   window_bits refusal    G1 throws std::runtime_error (code 1, "snarkvm_hip: <who>: window_bits must be 0 or 2..23"), G2 hip_failure (hipErrorInvalidValue,
//                          "... failed at api.hip:<line>: invalid argument").  Both texts are observable; msm_window_bits_ok is the one predicate, the throw stays
//                          with each entry point.
//   (no longer differs)    snarkvm_hip_msm_g2_registered used to take its lane - and resolve the owner of device scalars - BEFORE it validated; it validates first
//                          now, like G1.  A call that is invalid in two ways at once (a host pointer passed as device scalars AND window_bits 1, say) reports the
//                          argument refusal where it used to report the pointer's; every singly invalid call reports what it did (tests/test_gpu_msm_refusals.py
//                          passes on both libraries; no test pins a doubly invalid call).
//   G2 only from the host  no device-source registration (hence no owner / peer-copy route), no two-range form (KZG10's hiding range is a G1 matter) and no
//                          Montgomery flag (its callers pass canonical integers): the G2 entry points have no such parameters.
#include "msm_batch.hip.h"

struct snarkvm_hip_bases_g2 : bases_handle_t<fq2_t> {};
template <class F>
struct registered_t;  // the ABI's handle type over the field
template <>
struct registered_t<fq_t> {
    typedef snarkvm_hip_bases type;
};
template <>
struct registered_t<fq2_t> {
    typedef snarkvm_hip_bases_g2 type;
};

static bool msm_window_bits_ok(int window_bits) { return !window_bits || (window_bits >= 2 && window_bits <= MSM_C_MAX); }

// ---- registered bases ---------------------------------------------------------------------------------
// One replica per logical device: tables * npoints slots, table 0 filled by fill(lane, table0) - a host upload and convert_bases, a decode kernel - and tables
// 1 .. J-1 derived from it (table j = 2^table_bits * table j-1).  Every device fills and precomputes for itself, in parallel - unless the points live in a
// device's memory (device_source, G1 only): then that device alone does, and the others receive the finished tables by peer copies over xGMI.  Nothing is
// left allocated when any of it fails.
template <class F, class Fill>
static typename registered_t<F>::type* bases_build(size_t npoints, int tables, int table_bits, Fill fill, const void* device_source = nullptr) {
    typedef typename registered_t<F>::type handle_t;
    const int nd = g_rt.ndev();
    std::unique_ptr<handle_t> h(new handle_t());
    h->n = npoints;
    h->tables = tables;
    h->table_bits = table_bits;
    h->d.assign(nd, nullptr);
    if (!npoints) return h.release();
    const size_t bytes = (size_t)tables * npoints * sizeof(aff_mem_t<F>);
    auto build = [&](int dev) {
        lane_guard lg(dev);
        lane_t& c = lg.c();
        HIP_TRY(hipMalloc((void**)&h->d[dev], bytes));
        fill(c, h->d[dev]);
        precompute_tables_run<F>(c, h->d[dev], npoints, tables, table_bits);
        bases_to_lazy_form(c, h->d[dev], (size_t)tables * npoints);  // last: the tables are derived from one another in the exact form
        HIP_TRY(hipStreamSynchronize(c.stream));
    };
    try {
        if (!device_source) {
            std::vector<int> all;
            for (int d = 0; d < nd; d++) all.push_back(d);
            for_each_device(all, build);
        } else {
            const int owner = device_for(device_source, 1);
            build(owner);
            for (int d = 0; d < nd; d++) {
                if (d == owner) continue;
                lane_guard lg(d);
                HIP_TRY(hipMalloc((void**)&h->d[d], bytes));
                HIP_TRY(hipMemcpyPeerAsync(h->d[d], g_rt.devs[d]->physical, h->d[owner], g_rt.devs[owner]->physical, bytes, lg.c().stream));
                HIP_TRY(hipStreamSynchronize(lg.c().stream));
            }
        }
    } catch (...) {
        h->free_all();
        throw;
    }
    return h.release();
}
// the fill of a registration from host points: upload, then convert into table 0
template <class F>
static void bases_fill_from_host(lane_t& c, const void* points, size_t npoints, size_t ffi_affine_sz, aff_mem_t<F>* table0) {
    c.bases_tmp.ensure(npoints * ffi_affine_sz);
    HIP_TRY(hipMemcpyAsync(c.bases_tmp.p, points, npoints * ffi_affine_sz, hipMemcpyHostToDevice, c.stream));
    convert_bases<F>(c, c.bases_tmp.as<uint8_t>(), ffi_affine_sz, npoints, table0);
}

// ---- MSM over registered bases ----------------------------------------------------------------------------
// One MSM over a registered range with HOST scalars, split by point range over the devices when it is big enough (the
// reference's multi-GPU MSM, snarkvm.cu:254-295): device d sums its n / ndev pairs over its own replica with the full
// window set; the per-device bit-plane sums are added on the host before the one Horner chain.  (off1, n1): KZG10's second
// base range (see snarkvm_hip_msm_registered_ex).  A template so that only the unit that asks for it compiles the MSM it runs: used over fq_t alone.
template <class F>
static void msm_registered_host_scalars(void* out, const bases_handle_t<F>* h, size_t off0, size_t n0, size_t off1, size_t n1, const void* scalars,
                                        int scalars_montgomery, int window_bits) {
    const size_t n = n0 + n1;
    scope_flush();
    const int nd = g_rt.ndev();
    static const int trace = getenv("SNARKVM_HIP_TRACE") ? atoi(getenv("SNARKVM_HIP_TRACE")) : 0;
    const double t_begin = host_now_ms();
    // one part per device once every part keeps >= MSM_SPLIT_MIN pairs; big calls are cut further into scalar chunks whose
    // upload (32 B per pair over PCIe) hides behind the previous chunk's accumulation (lane_ring_run)
    size_t parts = n / MSM_SPLIT_MIN;
    if (parts > (size_t)nd) parts = (size_t)nd;
    if (parts < 1) parts = 1;
    const size_t chunk = msm_scalar_chunk_pairs();
    if (n >= 2 * chunk && (n + chunk - 1) / chunk > parts) parts = (n + chunk - 1) / chunk;
    // One device: GEOMETRIC chunks (tuning scalar_geo = g, default 4: sizes 1 : g [: g^2]).  Every chunk pays the bucket overhead of a
    // whole MSM (partial sums, their conversion, reduce rounds and the merge over 2^21 buckets at 22-bit windows: equal quarters of a 2^24 call cost 9.6 ms
    // each against 7.85 ms for a quarter of the unchunked MSM), so few chunks are better than many - and a chunk only has to keep
    // the GPU busy for as long as the NEXT chunk's scalars take to arrive (0.6 ms per 2^20 over PCIe against ~2 ms of arithmetic).
    std::vector<size_t> bound;
    const int geo = tuning().scalar_geo;
    if (nd == 1 && geo > 1 && tuning().taper != 0 && n >= ((size_t)1 << 22)) {
        parts = n >= ((size_t)1 << 23) ? 3 : 2;
        size_t wsum = 0, w = 1;
        for (size_t i = 0; i < parts; i++, w *= (size_t)geo) wsum += w;
        size_t acc_w = 0;
        w = 1;
        bound.push_back(0);
        for (size_t i = 0; i < parts; i++, w *= (size_t)geo) {
            acc_w += w;
            bound.push_back(i + 1 == parts ? n : (size_t)((unsigned __int128)n * acc_w / wsum));
        }
    } else {
        for (size_t i = 0; i <= parts; i++) bound.push_back(n * i / parts);
    }
    const int ndu = (int)(parts < (size_t)nd ? parts : (size_t)nd);
    std::unique_ptr<msm_accum_t<F>> acc(new msm_accum_t<F>());
    std::mutex acc_mu;
    std::vector<int> devs;
    if (ndu == 1) {
        devs.push_back(-1);  // any device with a free lane
    } else {
        for (int d = 0; d < ndu; d++) devs.push_back(d);
    }
    const size_t slot = msm_plane_bytes<F>();
    for_each_device(devs, [&](int dev) {
        std::vector<size_t> mine;
        for (size_t i = (dev < 0 ? 0 : (size_t)dev); i < parts; i += (size_t)ndu) mine.push_back(i);
        lane_guard lg;
        lg.acquire(dev, mine.size() > 2 ? 3 : (int)mine.size());
        const size_t L = lg.lanes.size();
        size_t max_cnt = 0;
        for (size_t j = 0; j < mine.size(); j++) {
            const size_t cnt = bound[mine[j] + 1] - bound[mine[j]];
            max_cnt = cnt > max_cnt ? cnt : max_cnt;
        }
        // Several scalar chunks on this device share ONE set of buckets (the geometry of the largest chunk for all of them): every
        // chunk adds its per-bucket partial sums to a sink - one slot per bucket, the merges chained by events across the lanes - and
        // the reduce / fold / bit-plane tail runs once after the last chunk instead of once per chunk (2^24 pairs over 12 x 22-bit
        // tables: four tails of ~2.5 ms over 2^21 buckets each).  tuning taper=0: every chunk runs its own tail (round 3).
        const bool use_sink = tuning().taper != 0 && mine.size() >= 2;
        std::vector<msm_pending_t> pend(use_sink ? 1 : mine.size());
        int chunk_c = window_bits;
        msm_bucket_sink_t sink;
        std::vector<hipEvent_t> merged;
        for (size_t l = 0; l < L; l++) {
            lane_t& c = *lg.lanes[l];
            c.begin_call();
            c.scalars_tmp.ensure(max_cnt * 32 + 32);
            c.pin.ensure(slot * (use_sink ? 1 : (mine.size() + L - 1) / L));
        }
        if (use_sink) {
            lane_t& c0 = *lg.lanes[0];
            const msm_plan_t pl = msm_make_plan(max_cnt, window_bits, h->tables, h->table_bits);
            chunk_c = pl.c;
            sink.nbt = (uint32_t)pl.W * pl.nb;
            sink.L = 1;
            const size_t bytes = (size_t)sink.nbt * msm_partial_bytes<F>();
            c0.sink_acc.ensure(bytes);
            sink.acc = c0.sink_acc.p;
            HIP_TRY(hipMemsetAsync(sink.acc, 0, bytes, c0.stream));  // all-zero = the point at infinity
            hipEvent_t ready = c0.new_event();
            HIP_TRY(hipEventRecord(ready, c0.stream));
            for (size_t l = 1; l < L; l++) HIP_TRY(hipStreamWaitEvent(lg.lanes[l]->stream, ready, 0));
            for (size_t j = 0; j < mine.size(); j++) merged.push_back(lg.lanes[j % L]->new_event());
        }
        auto upload = [&](size_t j, hipStream_t st) {
            lane_t& c = *lg.lanes[j % L];
            const size_t lo = bound[mine[j]], hi = bound[mine[j] + 1];
            if (hi > lo) HIP_TRY(hipMemcpyAsync(c.scalars_tmp.p, (const uint8_t*)scalars + lo * 32, (hi - lo) * 32, hipMemcpyHostToDevice, st));
        };
        auto compute = [&](size_t j, bool prof) {
            lane_t& c = *lg.lanes[j % L];
            // slice [lo, hi) of the concatenation (range 0 | range 1)
            const size_t lo = bound[mine[j]], hi = bound[mine[j] + 1];
            const size_t a0 = lo < n0 ? lo : n0, a1 = hi < n0 ? hi : n0;  // part inside range 0
            const size_t m0 = a1 - a0;
            const size_t s1 = off1 + (lo > n0 ? lo - n0 : 0);  // where the part inside range 1 begins
            msm_req_t r;
            if (m0)
                r.off0 = off0 + a0, r.n0 = m0, r.off1 = s1, r.n1 = hi - lo - m0;
            else
                r.off0 = s1, r.n0 = hi - lo;
            msm_bucket_sink_t mine_sink = sink;
            if (use_sink) {
                mine_sink.after = j ? merged[j - 1] : nullptr;
                mine_sink.done = merged[j];
            }
            msm_job_t<F> job = msm_handle_job<F>(*h, lg.lanes[0]->dev->logical, r);
            job.scalars = c.scalars_tmp.as<uint4>();
            job.scalars_montgomery = scalars_montgomery;
            job.window_bits = chunk_c;
            job.host_planes = c.pin.as<uint8_t>() + (use_sink ? 0 : slot * (j / L));
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
            compute(0, parts == 1);
        } else {
            lane_ring_run(lg, mine.size(), upload, [&](size_t j) { compute(j, false); }, trace, t_begin);
        }
        if (use_sink) {  // the last merge (which waited for all earlier ones), then the one tail on lane 0
            lane_t& c0 = *lg.lanes[0];
            HIP_TRY(hipStreamWaitEvent(c0.stream, merged.back(), 0));
            msm_job_t<F> tail = msm_handle_job<F>(*h, c0.dev->logical, msm_req_t{});  // the chunks' plan: the largest chunk over the handle's tables
            tail.n = max_cnt;
            tail.window_bits = chunk_c;
            tail.host_planes = c0.pin.p;
            pend[0] = msm_tail_from_sink<F>(c0, tail, sink);
        }
        for (size_t l = 0; l < L; l++) {
            HIP_TRY(hipStreamSynchronize(lg.lanes[l]->alt));
            HIP_TRY(hipStreamSynchronize(lg.lanes[l]->stream));
        }
        {
            std::lock_guard<std::mutex> lk(acc_mu);
            for (auto& pd : pend) msm_collect<F>(*acc, pd);
        }
        if (trace) fprintf(stderr, "[snarkvm_hip] registered MSM, host scalars: %zu chunk(s) done at t+%.2f ms\n", mine.size(), host_now_ms() - t_begin);
        for (size_t l = 0; l < L; l++) lg.lanes[l]->end_call();
    });
    acc->finish(out);
}
// one proof-sized MSM of one caller: a ticket on the handle's coalescer (msm_batch.hip.h::msm_coalesced) - concurrent callers are fused
template <class F>
static void msm_single_coalesced(void* out, const bases_handle_t<F>* h, size_t off0, size_t n0, size_t off1, size_t n1, const void* scalars,
                                 int scalars_on_device, int scalars_montgomery, int window_bits) {
    if (scalars_on_device && g_rt.device_of(scalars) < 0)
        throw hip_failure{hipErrorInvalidValue, "device pointer does not belong to a device in use (snarkvm_hip_set_devices)", __LINE__};
    msm_ticket_t t;
    t.req.off0 = off0, t.req.n0 = n0, t.req.off1 = n1 ? off1 : 0, t.req.n1 = n1, t.req.scalars = scalars, t.req.out = out;
    t.on_device = scalars_on_device ? 1 : 0;
    t.montgomery = scalars_montgomery ? 1 : 0;
    t.window_bits = window_bits;
    msm_coalesced<F>(*h, &t, 1);
}
// One MSM over registered bases, whatever the entry point: enqueued on the caller's scope, fused with concurrent callers, cut into scalar chunks
// (G1, host scalars), or run synchronously on a lane - of the device that owns the scalars when they are device-resident.  The entry point has validated `one`.
template <class F>
static void msm_registered_single(const bases_handle_t<F>& h, const msm_req_t& one, int scalars_on_device, int scalars_montgomery, int window_bits,
                                  bool scope_takes_empty) {
    const size_t n = one.n0 + one.n1;
    if ((n || scope_takes_empty) && msm_scope_enqueue<F>(h, &one, 1, scalars_on_device, scalars_montgomery, window_bits)) return;
    if (msm_coalescible(h, n, window_bits)) {
        msm_single_coalesced<F>(one.out, &h, one.off0, one.n0, one.off1, one.n1, one.scalars, scalars_on_device, scalars_montgomery, window_bits);
        return;
    }
    if constexpr (std::is_same<F, fq_t>::value)
        if (!scalars_on_device) {
            msm_registered_host_scalars<F>(one.out, &h, one.off0, one.n0, one.off1, one.n1, one.scalars, scalars_montgomery, window_bits);
            return;
        }
    lane_guard lg(device_for(one.scalars, (scalars_on_device && n) ? 1 : 0));
    lane_t& c = lg.c();
    c.begin_call();
    msm_job_t<F> job = msm_handle_job<F>(h, c.dev->logical, one);
    job.scalars = (const uint4*)one.scalars;
    // Host scalars reach this lane over fq2_t only: fq_t returned above.  Whoever drops that `if constexpr` gives G1 this unchunked upload in
    // place of msm_registered_host_scalars - a route change, not a cleanup.
    if (!scalars_on_device && n) {
        c.scalars_tmp.ensure(n * 32);
        c.phase_begin("msm_h2d");
        HIP_TRY(hipMemcpyAsync(c.scalars_tmp.p, one.scalars, n * 32, hipMemcpyHostToDevice, c.stream));
        c.phase_end();
        job.scalars = c.scalars_tmp.as<uint4>();
    }
    job.scalars_montgomery = scalars_montgomery;
    job.window_bits = window_bits;
    msm_run_sync<F>(c, job, one.out);
    c.end_call();
}
