#pragma once
// msm_run.hip.h - ONE multi-scalar multiplication on one lane (runtime.hip.h): the host finish of the bit-plane sums, tail geometry and launch,
// the job record, msm_layout and the msm_stage_* functions, msm_run / msm_run_sync, base conversion and the table precompute.
// Many MSMs - rings, chunks, batches, fusion, the coalescer - build on this in msm_batch.hip.h.
#include "runtime.hip.h"
#include "ec.hip.h"
#include "msm.hip.h"
#include "msm_sort.hip.h"

// ------------------------------------------------------------------------------------------------
// MSM driver
// ------------------------------------------------------------------------------------------------
static const uint64_t FQ_R[6] = {202099033278250856ull,  5854854902718660529ull, 11492539364873682930ull,
                                 8885205928937022213ull, 5545221690922665192ull, 39800542322357402ull};  // fq.rs:134-141
// Projective::zero() = (0, 1, 0) in Montgomery form (projective.rs:49-54); Fq2 one = (R, 0)
template <class F>
static void write_infinity(void* out) {
    const size_t fb = sizeof(typename F::mem_t);
    memset(out, 0, 3 * fb);
    memcpy((uint8_t*)out + fb, FQ_R, 48);
}

// ---- host-side finish of an MSM --------------------------------------------------------------------------------------
// The device leaves `nplanes` bit-plane sums (msm.hip.h 7b): the MSM result is sum_i 2^(pos[i]) * plane[i].  The remaining
// Horner chain (<= ~270 doublings of wave-uniform data) runs here, on the host, with the SAME field / curve code compiled
// for the host - the counterpart of the reference's host-side `dadd` collapse of its per-GPU results
// (algorithms/cuda/cuda/snarkvm.cu:290-295).  Several devices / chunks of one MSM simply add their planes into the same
// accumulator before the chain (msm_accum_t::add_planes), which is the whole multi-GPU combine.
static constexpr int MSM_MAX_POS = 320;
template <class F>
struct msm_accum_t {
    xyzz_t<F> at[MSM_MAX_POS];
    bool used[MSM_MAX_POS];
    int top = -1;
    msm_accum_t() {
        for (int i = 0; i < MSM_MAX_POS; i++) used[i] = false;
    }
    void add(int pos, const xyzz_t<F>& p) {
        if (p.is_inf()) return;
        if (pos < 0 || pos >= MSM_MAX_POS) throw std::runtime_error("msm: bit position out of range");
        if (!used[pos]) {
            at[pos] = p;
            used[pos] = true;
        } else {
            at[pos].add(p);
        }
        if (pos > top) top = pos;
    }
    // total = sum_p 2^p at[p], Jacobian memory image (the reference's Projective; infinity = (0, 1, 0))
    void finish(void* out) const {
        xyzz_t<F> t = xyzz_t<F>::inf();  // the chain stays in XYZZ (9 products per doubling, 14 per addition, no conversions)
        for (int p = top; p >= 0; p--) {
            t = t.dbl();
            if (used[p]) t.add(at[p]);
        }
        const jac_t<F> j = t.to_jacobian();
        uint32_t w[3 * F::MEM_WORDS];
        j.x.to_raw_words(w);
        j.y.to_raw_words(w + F::MEM_WORDS);
        j.z.to_raw_words(w + 2 * F::MEM_WORDS);
        memcpy(out, w, sizeof w);
    }
};
// what one device-side MSM run leaves for the host: planes (pinned host memory, valid after the lane's stream has been
// synchronised) and the bit position of each plane
struct msm_pending_t {
    const void* planes = nullptr;  // xyzz_mem_t<F>[nplanes]
    int nplanes = 0;
    int tail_windows = 0, nbits = 0;
    // position of plane (tw, j): DENSE (folded): tw = 2 w + sub -> c w + sub m + j; else tw = w -> c w + j
    int c = 0, m = 0;
    bool folded = false;
    int ninst = 0;  // fused multi-instance run: window w IS instance w (every instance has ONE bucket window at bit position 0)
    bool lazy = false;  // G1: the planes are raw lazy points (xyzz_mem_t<fqz_t>, 208 B each; tuning lazy_tail) - msm_collect converts them
    int pos(int idx) const {
        const int tw = idx / nbits, j = idx % nbits;
        if (ninst) return (tw & 1) * m + j;
        return folded ? c * (tw >> 1) + (tw & 1) * m + j : c * tw + j;
    }
};
// bytes of one bit plane / partial sum in the staging areas: the larger of the exact and the raw lazy image (G1: 192 / 208 B)
template <class F>
static constexpr size_t msm_point_bytes() {
    return sizeof(F) == sizeof(fq_t) && sizeof(xyzz_mem_t<fqz_t>) > sizeof(xyzz_mem_t<F>) ? sizeof(xyzz_mem_t<fqz_t>) : sizeof(xyzz_mem_t<F>);
}
// plane i of a pending run as an exact point (a raw lazy plane: four products by 2^377 on the host)
template <class F>
static xyzz_t<F> msm_plane(const msm_pending_t& pd, int i) {
    if constexpr (sizeof(F) == sizeof(fq_t)) {
        if (pd.lazy) {
            const xyzz_t<fqz_t> z = load_xyzz<fqz_t>(&((const xyzz_mem_t<fqz_t>*)pd.planes)[i]);
            if (z.is_inf()) return xyzz_t<F>::inf();
            return {z.x.to_exact(), z.y.to_exact(), z.zz.to_exact(), z.zzz.to_exact()};
        }
    }
    return load_xyzz<F>(&((const xyzz_mem_t<F>*)pd.planes)[i]);
}
template <class F>
static void msm_collect(msm_accum_t<F>& acc, const msm_pending_t& pd) {
    for (int i = 0; i < pd.nplanes; i++) acc.add(pd.pos(i), msm_plane<F>(pd, i));
}
// the planes of instance `inst` of a fused multi-instance run (2 * nbits consecutive planes)
template <class F>
static void msm_collect_inst(msm_accum_t<F>& acc, const msm_pending_t& pd, int inst) {
    const int per = 2 * pd.nbits;
    for (int i = inst * per; i < (inst + 1) * per; i++) acc.add(pd.pos(i), msm_plane<F>(pd, i));
}
// host description of a fused multi-instance run (msm_sort.hip.h: msm_inst_t)
struct msm_multi_t {
    const msm_inst_t* d_inst = nullptr;  // device table, K + 1 entries (sentinel: pstart = npad)
    uint32_t K = 0;
    size_t npad = 0;  // padded positions of all instances (multiple of SORT_TILE)
    size_t hn = 0;    // points of the registered vector: virtual index = table * hn + base index
    size_t plane_capacity = 0;  // planes the caller's staging area holds (checked before the copy is enqueued)
};

// Single-round accumulate grids are 256 workgroups of 4 waves for 256 CUs - one wave per SIMD when every CU gets exactly one
// workgroup.  The registers would let a CU take two, and the dispatcher does hand some CUs two while others stay idle; asking for
// more than half of a CU's 160 KB of LDS (unused) makes the second workgroup impossible.  tuning acc_lds overrides (0: off).
static size_t msm_acc_lds() {
    const long env = tuning().acc_lds;
    return env < 0 ? 0 : (size_t)env;
}
// Accumulation runs on the lazily reduced arithmetic: G1 on ffl.hip.h (tuning lazy=0: the exact kernel), G2 on the lane pair of ffl2p.hip.h (tuning
// lazy2=0).  Process wide: every base slot an MSM of that group reads - registered tables and the staging of table-less calls - then
// holds form406.
template <class F>
static bool msm_lazy_on() {
    return sizeof(F) == sizeof(fq_t) ? tuning().lazy != 0 : tuning().lazy2 != 0;
}
// G1: the tail (reduce rounds, bucket merge, fold, bit planes) runs on the lazy arithmetic too (ffl.hip.h::fqz_t) and reads the accumulate
// kernel's raw partial sums as they are
template <class F>
static bool msm_lazy_tail_on() {
    return sizeof(F) == sizeof(fq_t) && msm_lazy_on<F>() && tuning().lazy_tail != 0;
}
// bytes of one partial sum / sink slot / plane on the device for the arithmetic the tail of an MSM over F runs on
template <class F>
static size_t msm_partial_bytes() {
    return msm_lazy_tail_on<F>() ? sizeof(xyzz_mem_t<fqz_t>) : sizeof(xyzz_mem_t<F>);
}
// Tail geometry of an MSM with `nwin` bucket windows of 2^(c - 1) buckets: windows of >= 2^11 buckets are first folded into two tail
// windows of 2^fold_m / 2^fold_hb - 1 entries; so are smaller windows when there are too few (window, bit) pairs to spread an
// unfolded tail over the chip (registered tables below 4 096 points: 2 windows x 8 bits would be 16 workgroups walking every
// partial sum; the fold gives 48).  Fills the pending record the host finish reads.
struct msm_tail_geom_t {
    int fold_m, fold_hb, tail_windows, nbits;
    bool fold;
};
static msm_tail_geom_t msm_tail_geometry(const msm_plan_t& pl, uint32_t nwin, msm_pending_t& pd, int ninst) {
    msm_tail_geom_t g;
    const int K = pl.c - 1;
    g.fold_m = (K + 1) / 2;
    g.fold_hb = K - g.fold_m;
    g.fold = K >= 11 || (K >= 4 && pl.c * pl.W < 128);
    g.tail_windows = g.fold ? 2 * (int)nwin : (int)nwin;
    g.nbits = g.fold ? g.fold_m + 1 : pl.c;  // weights run up to 2^fold_m (L sums) / 2^(c-1) (plain buckets)
    pd.tail_windows = g.tail_windows;
    pd.nbits = g.nbits;
    pd.nplanes = g.tail_windows * g.nbits;
    pd.c = pl.c;
    pd.m = g.fold_m;
    pd.folded = g.fold;
    pd.ninst = ninst;
    if ((!ninst && pd.nplanes > MSM_MAX_POS) || pl.c * (pl.W - 1) + (g.fold ? g.fold_m : 0) + g.nbits > MSM_MAX_POS)
        throw hip_failure{hipErrorInvalidValue, "msm: window geometry exceeds the tail's bit-position range", __LINE__};
    return g;
}
// 7.-9. of msm_run: per-bucket partial-sum lists (sums, start, cnt) -> fold -> bit-plane sums -> copy to `host_planes` (the host runs
// the Horner chain).  The fold takes any distribution of the partial sums over the buckets (msm.hip.h 7a: flattened lists).
template <class F>
static void msm_tail_launch(lane_t& c, const msm_plan_t& pl, const msm_tail_geom_t& g, uint32_t nwin, uint32_t nbt, const xyzz_mem_t<F>* sums,
                            const uint32_t* start, const uint32_t* cnt, const msm_pending_t& pd, void* host_planes) {
    hipStream_t st = c.stream;
    c.planes.ensure((size_t)pd.nplanes * sizeof(xyzz_mem_t<F>));
    const bool is_g2 = sizeof(F) == sizeof(fq2_t);
    const int hex = (is_g2 && tuning().hex2) ? 1 : 0;  // G2: the upper tree levels on sixteen lanes per addition (hex2.hip.h)
    // quad-strided accumulation in front of the trees (msm.hip.h), a bit mask: 1 = G2 bit planes, 2 = G2 fold, 4 = G1 bit planes, 8 = G1 fold.  Measured on the
    // 2^16 G2 tail (tools/g2_tail.sh, 17 x 15 geometry): bit planes 235 -> 202 us (186 with hex2 = 2), fold 375 -> 404 us; on one proof in transcript order (bench.py --workload proof1): 8.54 -> 8.29 - 8.37 ms with 13, 8.41 with 9, 8.37 with 15 - hence the default 13.
    // ... and only in the LATENCY regime (a small MSM's tail: a handful of entries per workgroup, the chip not full).  A big MSM's fold / bit planes are throughput-bound -
    // one wave per output walking thousands of entries - and four lanes repeating every addition there is four times the work: measured at 2^24 (12 x 22 geometry)
    // fold 1.31 -> 1.66 ms, bit planes 0.18 -> 0.20 ms (profiles/r06_summary.md), so the mask applies to folds that run 128 / 256 threads per output and planes of <= 256 entries.
    int quads_planes = (tuning().tail_quads >> (is_g2 ? 0 : 2)) & 1, quads_fold = (tuning().tail_quads >> (is_g2 ? 1 : 3)) & 1;
    if (g.fold_m > 8) quads_planes = 0;
    // Fq2: the kernels never compute P + P or P - P (msm.hip.h TAIL_FLAGGED): they flag the outputs whose additions met equal x coordinates, and a one-wave kernel per output kind
    // recomputes those with the plain law - an unflagged workgroup returns at once.  Flags: [fold slots | planes].
    uint32_t* fold_flags = nullptr;
    uint32_t* plane_flags = nullptr;
    if (is_g2) {
        const size_t nslots = g.fold ? ((size_t)nwin << (g.fold_m + 1)) : 0;
        c.tail_flags.ensure((nslots + (size_t)pd.nplanes) * 4);
        fold_flags = c.tail_flags.as<uint32_t>();
        plane_flags = fold_flags + nslots;
    }
    if (g.fold) {
        c.fold_sums.ensure(((size_t)nwin << (g.fold_m + 1)) * sizeof(xyzz_mem_t<F>));
        // 256 threads per output keep the serial part of a small fold short - as long as the whole grid is resident at once
        // (<= 512 workgroups at two waves per SIMD); many windows (table-less small MSMs: 20 windows x 128 outputs) or many
        // buckets are throughput-bound: one wave per output
        const unsigned fold_blocks = ((1u << g.fold_m) + (1u << g.fold_hb)) * (unsigned)nwin;
        // (G2 kernels hold one wave per SIMD: 256-thread workgroups sit one per CU, so 384 of them take two turns on 256 CUs; 128-thread
        // workgroups sit two per CU and lose one level of the tree besides - tuning fold_threads2)
        unsigned fold_threads = (nbt >= (1u << 18) || fold_blocks > 512u) ? 64u : 256u;
        // a fused group of three or four proof-sized G1 instances (768 / 1 024 workgroups; commitment rounds 4 and 5 of a proof): 128 threads per output still put the
        // whole grid on the chip at once (<= 2 048 waves at two per SIMD) and halve the serial walk of a lone wave - tuning fold_mid (64: round 5's one wave per output)
        if (sizeof(F) <= 64 && nbt < (1u << 18) && fold_blocks > 512u && fold_blocks <= 1024u && tuning().fold_mid == 128) fold_threads = 128u;
        // (measured, 17 x 15 geometry = 256 workgroups: 256 threads 0.38 ms, 128 threads 0.53 ms, 64 threads 0.83 ms - the halved workgroup only pays when the
        // grid would otherwise take two turns, tools/g2_tail.sh)
        if (sizeof(F) > 64 && fold_threads == 256u && fold_blocks > 256u && (tuning().fold_threads2 == 128 || tuning().fold_threads2 == 64)) fold_threads = (unsigned)tuning().fold_threads2;
        if (sizeof(F) > 64 && fold_threads == 256u && fold_blocks <= 256u && (tuning().fold_small2 == 128 || tuning().fold_small2 == 64)) fold_threads = (unsigned)tuning().fold_small2;
        if (fold_threads == 64u) quads_fold = 0;
        const dim3 fold_grid((1u << g.fold_m) + (1u << g.fold_hb), (unsigned)nwin);
        hipLaunchKernelGGL((msm_fold_kernel<F>), fold_grid, dim3(fold_threads), 0, st, sums, start, cnt, c.fold_sums.as<xyzz_mem_t<F>>(), g.fold_m, g.fold_hb, hex, quads_fold,
                           fold_flags);
        if constexpr (TAIL_FLAGGED<F>::value)
            hipLaunchKernelGGL((msm_fold_fix_kernel<F>), fold_grid, dim3(64), 0, st, sums, start, cnt, c.fold_sums.as<xyzz_mem_t<F>>(), g.fold_m, g.fold_hb,
                               (const uint32_t*)fold_flags);
        // one lane per entry of a plane (<= 2^fold_m); quad-strided: one QUAD per entry, up to 64 quads
        const unsigned plane_threads = quads_planes ? (g.fold_m <= 4 ? 64u : g.fold_m == 5 ? 128u : 256u) : (g.fold_m <= 6 ? 64u : g.fold_m == 7 ? 128u : 256u);
        const dim3 plane_grid((unsigned)g.nbits, (unsigned)g.tail_windows);
        hipLaunchKernelGGL((msm_bitplane_kernel<F, true>), plane_grid, dim3(plane_threads), 0, st, (const xyzz_mem_t<F>*)c.fold_sums.as<xyzz_mem_t<F>>(),
                           (const uint32_t*)nullptr, (const uint32_t*)nullptr, c.planes.as<xyzz_mem_t<F>>(), pl.nb, g.fold_m, g.fold_hb, hex, quads_planes, plane_flags);
        if constexpr (TAIL_FLAGGED<F>::value)
            hipLaunchKernelGGL((msm_bitplane_fix_kernel<F, true>), plane_grid, dim3(64), 0, st, (const xyzz_mem_t<F>*)c.fold_sums.as<xyzz_mem_t<F>>(), (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, c.planes.as<xyzz_mem_t<F>>(), pl.nb, g.fold_m, g.fold_hb, (const uint32_t*)plane_flags);
    } else {
        const dim3 plane_grid((unsigned)g.nbits, (unsigned)g.tail_windows);
        hipLaunchKernelGGL((msm_bitplane_kernel<F, false>), plane_grid, dim3(256), 0, st, sums, start, cnt, c.planes.as<xyzz_mem_t<F>>(), pl.nb, 0, 0, hex, 0, plane_flags);
        if constexpr (TAIL_FLAGGED<F>::value)
            hipLaunchKernelGGL((msm_bitplane_fix_kernel<F, false>), plane_grid, dim3(64), 0, st, sums, start, cnt, c.planes.as<xyzz_mem_t<F>>(), pl.nb, 0, 0,
                               (const uint32_t*)plane_flags);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_planes, c.planes.p, (size_t)pd.nplanes * sizeof(xyzz_mem_t<F>), hipMemcpyDeviceToHost, st));
}
// A bucket sink: the chunks of ONE big MSM (snarkvm_msm over host bases: point-range chunks that arrive over PCIe one after the other)
// leave their per-bucket partial sums in a persistent accumulator instead of each running its own fold / bit-plane tail; the tail runs
// once, over the accumulator, after the last chunk.  L lanes work on the chunks concurrently: each owns one slot per bucket
// (bucket k, lane l -> acc[k * L + l]), so no two streams ever touch the same slot.
struct msm_bucket_sink_t {
    void* acc = nullptr;  // xyzz_mem_t<F>[nbt * L], zero-initialised (the point at infinity)
    uint32_t L = 1, slot = 0, nbt = 0;
    // L == 1 with several lanes (2^21 buckets of a wide-window geometry: one slot per bucket, not one per lane): the merges are
    // chained - a chunk's merge waits for `after` (the previous chunk's merge) and records `done`
    hipEvent_t after = nullptr, done = nullptr;
};
// SNARKVM_HIP_TRACE=2 (diagnostics): wait for the stream after every phase and name it on stderr - locates a kernel that never returns
static int msm_trace_level() {
    static const int level = getenv("SNARKVM_HIP_TRACE") ? atoi(getenv("SNARKVM_HIP_TRACE")) : 0;
    return level;
}
// The phases of one msm_run, handed from stage to stage: profiling events on the lane (`profile`) and the trace lines (n: the size they quote).
struct msm_phases_t {
    lane_t& c;
    bool profile;
    int trace;
    size_t n;
    const char* cur = "";
    void begin(const char* name) {
        cur = name;
        if (trace >= 2) fprintf(stderr, "[snarkvm_hip] msm n=%zu: %s ...\n", n, name);
        if (profile) c.phase_begin(name);
    }
    void end() {
        if (profile) c.phase_end();
        if (trace >= 2) {
            const hipError_t e = hipStreamSynchronize(c.stream);
            fprintf(stderr, "[snarkvm_hip] msm n=%zu: %s done (%s)\n", n, cur, hipGetErrorString(e));
        }
    }
};
// Steps 6.-9. of msm_run on the tail arithmetic T (F itself, or fqz_t for a G1 MSM whose accumulate kernel left raw lazy partial sums):
// reduce rounds (cnt_a, start_a, part_a) -> (cnt_b, start_b, part_b) -> ..., then either the merge into a bucket sink (a chunk of a
// bigger MSM; pd.nplanes = 0) or fold -> bit planes -> copy to `host_planes`.
template <class T>
static void msm_reduce_and_tail(lane_t& c, const msm_plan_t& pl, const msm_tail_geom_t& tg, uint32_t nwin, uint32_t nbt, int rounds, size_t T0_max, size_t T1_max,
                                const msm_bucket_sink_t* sink, msm_pending_t& pd, void* host_planes, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    ph.begin("msm_reduce_partials");
    uint32_t *cnt_in = c.cnt_a.as<uint32_t>(), *cnt_out = c.cnt_b.as<uint32_t>();
    uint32_t *start_in = c.start_a.as<uint32_t>(), *start_out = c.start_b.as<uint32_t>();
    xyzz_mem_t<T> *pin = c.part_a.as<xyzz_mem_t<T>>(), *pout = c.part_b.as<xyzz_mem_t<T>>();
    size_t T_in_max = T0_max;
    for (int r = 0; r < rounds; r++) {
        size_t T_out_max = T_in_max / pl.S2 + nbt + 1;
        if (T_out_max > T1_max) T_out_max = T1_max;  // both ping-pong buffers hold >= T1_max partials
        hipLaunchKernelGGL(msm_alloc_kernel, dim3((nbt + 1 + 255) / 256), dim3(256), 0, st, cnt_in, cnt_out, nbt, pl.S2);
        exclusive_scan_u32(st, cnt_out, start_out, (size_t)nbt + 1, c.scan_tmp.as<uint32_t>());
        hipLaunchKernelGGL((msm_reduce_kernel<T>), dim3((unsigned)((T_out_max + 255) / 256)), dim3(256), 0, st, pin, start_in, cnt_in, start_out, pout, nbt,
                           pl.S2);
        std::swap(cnt_in, cnt_out);
        std::swap(start_in, start_out);
        std::swap(pin, pout);
        T_in_max = T_out_max;
    }
    ph.end();
    if (sink) {
        // a chunk of a bigger MSM: its per-bucket partial sums join the sink; the tail runs once, after the last chunk (msm_tail_from_sink)
        ph.begin("msm_bucket_merge");
        if (sink->after) HIP_TRY(hipStreamWaitEvent(st, sink->after, 0));
        hipLaunchKernelGGL((msm_bucket_merge_kernel<T>), dim3((nbt + 255) / 256), dim3(256), 0, st, (const xyzz_mem_t<T>*)pin, (const uint32_t*)start_in,
                           (const uint32_t*)cnt_in, (xyzz_mem_t<T>*)sink->acc, nbt, sink->L, sink->slot);
        if (sink->done) HIP_TRY(hipEventRecord(sink->done, st));
        ph.end();
        HIP_TRY(hipGetLastError());
        pd.nplanes = 0;
        return;
    }
    ph.begin("msm_bucket_reduce");
    msm_tail_launch<T>(c, pl, tg, nwin, nbt, pin, start_in, cnt_in, pd, host_planes);
    ph.end();
}
// Step 5 of msm_run: the accumulate launch for F - G1 on the lazy arithmetic (ffl.hip.h), G2 on a lane pair (ffl2p.hip.h), or F's exact kernel
// (tuning lazy / lazy2 = 0) - `nthreads` segments of pl.S sorted entries, per-bucket partial sums into part_a (start_a: their slots).
// one_wave: a single-round grid of at most 2^22 entries runs one wave per SIMD, where nothing else hides the base gather.
template <class F>
static void msm_launch_accumulate(lane_t& c, const msm_plan_t& pl, const aff_mem_t<F>* vbase, uint32_t* boffp, uint32_t nbt, size_t nthreads, bool one_wave,
                                  bool ltail) {
    hipStream_t st = c.stream;
#ifdef SV_BENCH  // profiling builds only (wrong results): restrict the gather to the first 2^k bases to separate ALU time from HBM gather time
    static const uint32_t dbg_mask = getenv("SNARKVM_HIP_DEBUG_IDX_MASK") ? (uint32_t)strtoul(getenv("SNARKVM_HIP_DEBUG_IDX_MASK"), nullptr, 0) : 0xffffffffu;
#else
    constexpr uint32_t dbg_mask = 0xffffffffu;
#endif
    const size_t tmax = nthreads + nbt + 1;  // every thread leaves >= 1 partial sum, one more per bucket boundary inside its segment
    if constexpr (sizeof(F) == sizeof(fq_t)) {
        if (msm_lazy_on<F>()) {
            // lazy tail: the raw partial sums (208 B each) ARE the tail's input (part_a holds T0_max >= tmax of them); else they go to their own
            // buffer and the dense conversion pass fills part_a
            if (!ltail) c.part_raw.ensure(tmax * sizeof(g1_lazy_partial_t));
            g1_lazy_partial_t* raw_out = ltail ? c.part_a.as<g1_lazy_partial_t>() : c.part_raw.as<g1_lazy_partial_t>();
            // One workgroup per CU (a dynamic LDS request no second workgroup fits beside) = one accumulate wave per SIMD with half
            // of the register file and ~64 KB of LDS left free: single-round grids always; multi-round grids when
            // tuning acc_one_wg is set - the sort and tail kernels of the NEXT instance of a pipelined batch (another
            // lane's stream) then find room beside the accumulate waves instead of waiting for gaps between its rounds.
            // (a 3-waves-per-SIMD build of this kernel - 168 VGPRs - was measured: no gain)
            hipLaunchKernelGGL((msm_accumulate_lazy_kernel<true>), dim3((unsigned)((nthreads + 255) / 256)), dim3(256), one_wave || tuning().acc_one_wg ? msm_acc_lds() : 0, st,
                               vbase, c.sorted.as<uint32_t>(), boffp, c.start_a.as<uint32_t>(), raw_out, nbt, pl.S, dbg_mask);
            if (!ltail)
                hipLaunchKernelGGL(g1_partials_to_exact_kernel, dim3((unsigned)((tmax + 255) / 256)), dim3(256), 0, st, (const g1_lazy_partial_t*)raw_out,
                                   c.part_a.as<g1_xyzz_mem_t>(), (const uint32_t*)c.start_a.as<uint32_t>(), nbt);
            return;
        }
    } else {
#ifndef SV_NO_G2
        if (msm_lazy_on<F>()) {
            // two lanes per segment, two waves per SIMD; raw 512-byte partial sums, then the dense conversion
            c.part_raw.ensure(tmax * sizeof(g2_pair_partial_t));
            hipLaunchKernelGGL((msm_accumulate_pair2_kernel<false>), dim3((unsigned)((2 * nthreads + 255) / 256)), dim3(256), 0, st, vbase, c.sorted.as<uint32_t>(),
                               boffp, c.start_a.as<uint32_t>(), c.part_raw.as<g2_pair_partial_t>(), nbt, pl.S, dbg_mask);
            hipLaunchKernelGGL(g2_pair_partials_to_exact_kernel, dim3((unsigned)((8 * tmax + 255) / 256)), dim3(256), 0, st,
                               (const g2_pair_partial_t*)c.part_raw.as<g2_pair_partial_t>(), c.part_a.as<xyzz_mem_t<fq2_t>>(),
                               (const uint32_t*)c.start_a.as<uint32_t>(), nbt);
            return;
        }
#endif
    }
    if (one_wave)  // software-pipelined gather
        hipLaunchKernelGGL((msm_accumulate_seg_kernel<F, 1, true>), dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, vbase, c.sorted.as<uint32_t>(), boffp,
                           c.start_a.as<uint32_t>(), c.part_a.as<xyzz_mem_t<F>>(), nbt, pl.S, dbg_mask);
    else
        hipLaunchKernelGGL((msm_accumulate_seg_kernel<F, 1, false>), dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, vbase, c.sorted.as<uint32_t>(), boffp,
                           c.start_a.as<uint32_t>(), c.part_a.as<xyzz_mem_t<F>>(), nbt, pl.S, dbg_mask);
}
template <class F>
static size_t msm_plane_bytes() {
    return (size_t)MSM_MAX_POS * msm_point_bytes<F>();  // upper bound on tail windows * bits
}
// One device-side MSM, as msm_run takes it.
template <class F>
struct msm_job_t {
    // bases (converted, on the lane's device): scalar i < n0 meets bases[i], the others bases1[i - n0]; bases1 == nullptr: one range, n0 is not read.
    // tables > 1: table j, 2^(table_bits * j) * P, lies table_stride slots behind table j - 1 (bases_handle_t).
    const aff_mem_t<F>* bases = nullptr;
    const aff_mem_t<F>* bases1 = nullptr;
    size_t n0 = 0;
    int tables = 1;
    size_t table_stride = 0;
    int table_bits = 0;
    // scalars: n of them on the device, 32 B each; scalars_montgomery: Fr memory images, the read fuses Fr::to_bigint
    const uint4* scalars = nullptr;
    size_t n = 0;
    int scalars_montgomery = 0;
    // geometry: the window width, 0 = the planner's choice
    int window_bits = 0;
    // output: pinned, >= msm_plane_bytes<F>() - the bit-plane sums (msm_run_sync, msm_tail_from_sink: set by the callee / read as the staging area)
    void* host_planes = nullptr;
    // options
    bool profile = true;  // the phases leave profiling events on the lane
    // fused multi-instance run (msm_sort.hip.h): n = multi->npad padded positions, bases = the handle's table array, `scalars` unused (the instance
    // table carries the pointers), one bucket window per instance; host_planes holds multi->K * 2 * (fold_m + 1) planes
    const msm_multi_t* multi = nullptr;
    const msm_bucket_sink_t* sink = nullptr;  // a chunk of a bigger MSM: its partial sums join the sink, no tail
    // recorded on the lane's stream behind the last kernel that reads the scalar vectors (the digit kernel; wide windows: the fused level-1
    // scatter) - from there on the caller may overwrite them while the MSM is still running
    hipEvent_t scalars_read = nullptr;
};
// What the stages of msm_run share: plan, geometry and the filled kernel parameter blocks.  Plain values; the lane's buffers are named where they are used.
template <class F>
struct msm_layout_t {
    msm_plan_t pl;
    bool wide;    // u32 digits, three-level sort
    bool fused;   // the level-1 partition reads the scalars itself
    bool ltail;   // the tail runs on the lazy arithmetic
    bool single_round, prefetch_ok;  // see msm_stage_accumulate
    uint32_t nwin, nbt;              // bucket windows of the tail (multi: one per instance), buckets in all
    size_t E_max, T0_max, T1_max;    // digit entries; bounds on the partial sums before / after the first reduce round
    const aff_mem_t<F>* vbase;       // what the sort's virtual indices are slots of (msm_radix_params_t)
    msm_tail_geom_t tg;
    msm_radix_params_t rp;
    msm_digit_params_t dp;
    // the radix partition: B1 level-1 bins per window, nbins in all, LBL key bits at the last level, nseg_last segments feeding it
    int LBL;
    uint32_t B1, nbins, nseg_last;
    size_t ncounts1, tiles1, tiles2_max;
};
// Validation, the plan, the bucket-side workspace and the geometry of every later stage.  Fills the pending record the host finish reads.
template <class F>
static msm_layout_t<F> msm_layout(lane_t& c, const msm_job_t<F>& j, msm_pending_t& pd) {
    const msm_multi_t* mu = j.multi;
    const size_t n = j.n;
    size_t n0 = j.bases1 ? j.n0 : n;
    if (n0 > n) n0 = n;
    msm_layout_t<F> L{};
    if (n >= ((size_t)1 << 31)) throw hip_failure{hipErrorInvalidValue, "msm: npoints must be < 2^31", __LINE__};
    const msm_plan_t pl = L.pl = msm_make_plan(n, mu ? j.table_bits : j.window_bits, j.tables, j.table_bits);
    L.wide = pl.c > 16;
    if (mu && (L.wide || pl.W != 1 || pl.c < 12 || (size_t)pl.J * mu->hn >= ((size_t)1 << 31) || n != mu->npad || n % SORT_TILE))
        throw hip_failure{hipErrorInvalidValue, "msm: geometry not eligible for a fused multi-instance run", __LINE__};
    if ((size_t)pl.Wd * n >= ((size_t)1 << 32)) throw hip_failure{hipErrorInvalidValue, "msm: windows * npoints must be < 2^32", __LINE__};
    if ((size_t)pl.J * n >= ((size_t)1 << 31)) throw hip_failure{hipErrorInvalidValue, "msm: tables * npoints must be < 2^31", __LINE__};
    const aff_mem_t<F>* vb1 = j.bases1 ? j.bases1 : j.bases;
    L.vbase = mu ? j.bases : (vb1 < j.bases ? vb1 : j.bases);
    if (!mu) {
        const size_t top0 = (size_t)(j.bases - L.vbase) + n0, top1 = (size_t)(vb1 - L.vbase) + (n - n0);
        if ((size_t)(pl.J - 1) * j.table_stride + (top0 > top1 ? top0 : top1) >= ((size_t)1 << 31))
            throw hip_failure{hipErrorInvalidValue, "msm: base slots must be addressable in 31 bits (tables * registered points < 2^31)", __LINE__};
    }
    const size_t E_max = L.E_max = (size_t)pl.Wd * n;
    const uint32_t nwin = L.nwin = mu ? mu->K : (uint32_t)pl.W;
    const uint32_t nbt = L.nbt = nwin * pl.nb;

    c.scan_tmp.ensure((scan_tmp_elems((size_t)nbt + 1)) * 4);
    c.boff.ensure(((size_t)nbt + 2) * 4);
    c.cnt_a.ensure(((size_t)nbt + 1) * 4);
    c.cnt_b.ensure(((size_t)nbt + 1) * 4);
    c.start_a.ensure(((size_t)nbt + 1) * 4);
    c.start_b.ensure(((size_t)nbt + 1) * 4);
    // thread-count bounds per level: T_(r+1) <= T_r / S2 + nbt + 1 (fixed point ~ nbt * 64/63), plus slack
    const size_t slack = (size_t)nbt / 32 + 64;
    L.T0_max = E_max / pl.S + nbt + 1 + slack;
    L.T1_max = L.T0_max / pl.S2 + nbt + 1 + slack;
    pd.lazy = L.ltail = msm_lazy_tail_on<F>();
    c.part_a.ensure(L.T0_max * msm_partial_bytes<F>());
    c.part_b.ensure(L.T1_max * msm_partial_bytes<F>());
    L.tg = msm_tail_geometry(pl, nwin, pd, mu ? (int)mu->K : 0);
    if (mu && (size_t)pd.nplanes > mu->plane_capacity) throw hip_failure{hipErrorInvalidValue, "msm: plane staging of the fused group too small", __LINE__};
    if (j.sink && (mu || j.sink->nbt != nbt)) throw hip_failure{hipErrorInvalidValue, "msm: bucket sink does not match the plan", __LINE__};
    c.planes.ensure((size_t)pd.nplanes * msm_partial_bytes<F>());

    // level-1 key of <= 7 bits: FUSED_G * 2^HB <= FUSED_THREADS
    L.fused = !mu && L.wide && tuning().fused && pl.c <= 22 && pl.Wd <= FUSED_MAX_ROWS;
    memcpy(L.dp.bias, pl.bias, sizeof L.dp.bias);
    L.dp.c = pl.c;
    L.dp.W = pl.Wd;
    L.dp.n = n;
    L.dp.montgomery = j.scalars_montgomery;
    // see msm_stage_accumulate; a fused multi-instance run never reads back either: its instances are small (<= 2^18 points each), so the
    // flattened-list fold takes whatever partial sums the accumulate grid leaves
    L.single_round = mu || (size_t)pl.Wd * n <= ((size_t)1 << 22);
    L.prefetch_ok = (size_t)pl.Wd * n <= ((size_t)1 << 22);  // one wave per SIMD: nothing else hides the gather

    msm_radix_params_t& rp = L.rp;
    rp.n = n;
    rp.c = pl.c;
    rp.W = pl.W;
    rp.J = pl.J;
    // virtual indices = slots relative to vbase (msm_radix_params_t): the lower of the two base ranges, or the handle's table array
    if (mu) {
        rp.inst = mu->d_inst;
        rp.ninst = mu->K;
        rp.vstride = (uint32_t)mu->hn;
    } else {
        rp.vn0 = (uint32_t)n0;
        rp.vr0 = (uint32_t)(j.bases - L.vbase);
        rp.vr1 = (uint32_t)(vb1 - L.vbase);
        rp.vstride = (uint32_t)j.table_stride;
    }
    const int K = pl.c - 1;           // bucket-index bits
    L.LBL = K < 7 ? K : 7;            // key bits of the last level
    rp.LB = L.wide ? 14 : L.LBL;      // bits left below the level-1 key
    rp.HB = K - rp.LB;
    rp.nb = pl.nb;
    rp.xcd = (uint32_t)tuning().xcd;
    rp.tiles_per_row = L.fused ? (uint32_t)((n + FUSED_TILE - 1) / FUSED_TILE) : (uint32_t)((n + SORT_TILE - 1) / SORT_TILE);
    rp.TPW = (uint32_t)pl.J * rp.tiles_per_row;
    L.B1 = 1u << rp.HB;
    L.nbins = nwin * L.B1;
    // single: W windows x B1 bins x TPW tiles; multi: the windows (instances) partition the J * npad / TILE tiles among themselves
    L.ncounts1 = (size_t)(mu ? L.B1 : L.nbins) * rp.TPW;
    L.tiles1 = (size_t)(mu ? 1 : pl.W) * rp.TPW;
    L.nseg_last = L.wide ? L.nbins << 7 : L.nbins;
    L.tiles2_max = E_max / SORT_TILE + L.nseg_last + 1;
    return L;
}
// 1. scalar read, unless the level-1 partition does it (L.fused): the stand-alone digit kernel writes the [rows][n] digit matrix.
template <class F>
static void msm_stage_digits(lane_t& c, const msm_layout_t<F>& L, const msm_job_t<F>& j, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    ph.begin("msm_digits");
    c.digits.ensure(L.E_max * (L.wide ? sizeof(uint32_t) : sizeof(uint16_t)));
    size_t blocks = (j.n + 255) / 256;
    if (j.multi) {
        hipLaunchKernelGGL(msm_digits_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, st, j.multi->d_inst, j.multi->K, c.digits.as<uint16_t>(), L.dp);
    } else {
        if (blocks > 256 * 16) blocks = 256 * 16;
        if (L.wide)
            hipLaunchKernelGGL((msm_digits_kernel<uint32_t>), dim3((unsigned)blocks), dim3(256), 0, st, j.scalars, c.digits.as<uint32_t>(), L.dp);
        else
            hipLaunchKernelGGL((msm_digits_kernel<uint16_t>), dim3((unsigned)blocks), dim3(256), 0, st, j.scalars, c.digits.as<uint16_t>(), L.dp);
    }
    ph.end();
    if (j.scalars_read) HIP_TRY(hipEventRecord(j.scalars_read, st));
}
// fn(std::integral_constant<int, c>) for the window widths the fused level-1 kernels exist for
template <class Fn>
static void msm_fused_width(int c, Fn&& fn) {
    switch (c) {
        case 17: return fn(std::integral_constant<int, 17>{});
        case 18: return fn(std::integral_constant<int, 18>{});
        case 19: return fn(std::integral_constant<int, 19>{});
        case 20: return fn(std::integral_constant<int, 20>{});
        case 21: return fn(std::integral_constant<int, 21>{});
        case 22: return fn(std::integral_constant<int, 22>{});
    }
}
// 1. + 2. wide windows: the scalar-read phase proper - a read-only pass over the scalars (32 B each) that leaves the level-1 histograms - then the
// level-1 scatter reads them again and writes (v1, rem1); the digits never exist in memory
template <class F>
static void msm_stage_level1_fused(lane_t& c, const msm_layout_t<F>& L, const msm_job_t<F>& j, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    const msm_plan_t& pl = L.pl;
    const uint32_t ntiles = L.rp.tiles_per_row, keys = (uint32_t)pl.Wd * L.B1;
    const uint32_t nchunks = (ntiles + FUSED_CHUNK - 1) / FUSED_CHUNK;
    const size_t ngroups = (size_t)keys * nchunks;
    c.counts.ensure((size_t)ntiles * keys * 4);
    c.offsets.ensure((size_t)ntiles * keys * 4);
    c.fchunk.ensure(2 * ngroups * 4);
    c.scan_tmp.ensure(scan_tmp_elems(ngroups > (size_t)L.nbt + 2 ? ngroups : (size_t)L.nbt + 2) * 4);
    uint32_t* counts1 = c.counts.as<uint32_t>();
    uint32_t* off1 = c.offsets.as<uint32_t>();
    uint32_t* csum = c.fchunk.as<uint32_t>();
    uint32_t* choff = csum + ngroups;
    ph.begin("msm_scalar_read");
    const size_t hist_lds = (size_t)keys * 4;
    // 1 024-thread workgroups with four private histogram copies (msm_sort.hip.h)
    msm_fused_width(pl.c, [&](auto cb) {
        hipLaunchKernelGGL((radix_hist1_wide_kernel<decltype(cb)::value>), dim3(ntiles), dim3(HISTW_THREADS), hist_lds * HISTW_COPIES, st, j.scalars, counts1, L.rp, L.dp);
    });
    ph.end();
    ph.begin("msm_sort_level1");
    const unsigned key_blocks = (keys + FUSED_THREADS - 1) / FUSED_THREADS;
    hipLaunchKernelGGL(fused_chunk_sums_kernel, dim3(nchunks, key_blocks), dim3(FUSED_THREADS), 0, st, (const uint32_t*)counts1, csum, ntiles, nchunks, keys, L.B1,
                       (uint32_t)pl.W, (uint32_t)pl.J);
    exclusive_scan_u32(st, csum, choff, ngroups, c.scan_tmp.as<uint32_t>());
    hipLaunchKernelGGL(fused_tile_offsets_kernel, dim3(nchunks, key_blocks), dim3(FUSED_THREADS), 0, st, (const uint32_t*)counts1, (const uint32_t*)choff,
                       (const uint32_t*)csum, off1, c.rbinstart.as<uint32_t>(), ntiles, nchunks, keys, L.B1, (uint32_t)pl.W, (uint32_t)pl.J);
    msm_fused_width(pl.c, [&](auto cb) {
        hipLaunchKernelGGL((radix_scatter1_fused_kernel<decltype(cb)::value>), dim3(ntiles), dim3(FUSED_THREADS), 0, st, j.scalars, (const uint32_t*)counts1,
                           (const uint32_t*)off1, c.rv1.as<uint32_t>(), c.rl1.as<uint16_t>(), L.rp, L.dp);
    });
    if (j.scalars_read) HIP_TRY(hipEventRecord(j.scalars_read, st));
    ph.end();
}
// 2. LDS-staged radix partition (msm_sort.hip.h), level 1: the workspace of the whole sort, then the entries grouped by the top key bits
// (v1, rem1) and the bin layout rbinstart
template <class F>
static void msm_stage_level1(lane_t& c, const msm_layout_t<F>& L, const msm_job_t<F>& j, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    c.counts.ensure(L.ncounts1 * 4);
    c.offsets.ensure(L.ncounts1 * 4);
    c.scan_tmp.ensure(scan_tmp_elems(L.ncounts1 > (size_t)L.nbt + 2 ? L.ncounts1 : (size_t)L.nbt + 2) * 4);
    c.rv1.ensure(L.E_max * 4);
    c.rl1.ensure(L.E_max * (L.wide ? 2 : 1));
    c.rcounts2.ensure(L.tiles2_max * 128 * 4);
    c.roff2.ensure(L.tiles2_max * 128 * 4);
    c.rbinstart.ensure(((size_t)L.nbins + 2) * 4);
    c.rntiles.ensure(((size_t)L.nseg_last + 2) * 4);
    c.rtstart.ensure(((size_t)L.nseg_last + 2) * 4);
    c.rbsize.ensure(((size_t)L.nbt + 3) * 4);
    c.sorted.ensure(L.E_max * 4);
    if (L.fused) return msm_stage_level1_fused(c, L, j, ph);
    uint32_t* counts1 = c.counts.as<uint32_t>();
    uint32_t* off1 = c.offsets.as<uint32_t>();
    ph.begin("msm_sort_level1");
    if (L.wide) {
        hipLaunchKernelGGL((radix_hist1_kernel<uint32_t>), dim3((unsigned)L.tiles1), dim3(SORT_THREADS), 0, st, c.digits.as<uint32_t>(), counts1, L.rp);
        exclusive_scan_u32(st, counts1, off1, L.ncounts1, c.scan_tmp.as<uint32_t>());
        hipLaunchKernelGGL((radix_scatter1_kernel<uint32_t, uint16_t>), dim3((unsigned)L.tiles1), dim3(SORT_THREADS), 0, st, c.digits.as<uint32_t>(),
                           counts1, off1, c.rv1.as<uint32_t>(), c.rl1.as<uint16_t>(), L.rp);
    } else {
        hipLaunchKernelGGL((radix_hist1_kernel<uint16_t>), dim3((unsigned)L.tiles1), dim3(SORT_THREADS), 0, st, c.digits.as<uint16_t>(), counts1, L.rp);
        exclusive_scan_u32(st, counts1, off1, L.ncounts1, c.scan_tmp.as<uint32_t>());
        hipLaunchKernelGGL((radix_scatter1_kernel<uint16_t, uint8_t>), dim3((unsigned)L.tiles1), dim3(SORT_THREADS), 0, st, c.digits.as<uint16_t>(),
                           counts1, off1, c.rv1.as<uint32_t>(), c.rl1.as<uint8_t>(), L.rp);
    }
    if (j.multi)
        hipLaunchKernelGGL(radix_bin_layout_multi_kernel, dim3((L.nbins + 1 + 255) / 256), dim3(256), 0, st, off1, counts1, L.ncounts1,
                           c.rbinstart.as<uint32_t>(), L.nbins, L.rp);
    else
        hipLaunchKernelGGL(radix_bin_layout_kernel, dim3((L.nbins + 1 + 255) / 256), dim3(256), 0, st, off1, counts1, L.ncounts1, c.rbinstart.as<uint32_t>(),
                           L.nbins, L.rp.TPW);
    ph.end();
}
// one further level: items grouped in `nseg` segments -> their tiles (rntiles, rtstart)
static void msm_tile_segments(lane_t& c, const uint32_t* seg_start, uint32_t nseg) {
    hipLaunchKernelGGL(radix_bin_tiles_kernel, dim3((nseg + 1 + 255) / 256), dim3(256), 0, c.stream, seg_start, c.rntiles.as<uint32_t>(), nseg);
    exclusive_scan_u32(c.stream, c.rntiles.as<uint32_t>(), c.rtstart.as<uint32_t>(), (size_t)nseg + 1, c.scan_tmp.as<uint32_t>());
}
// per (segment, key): exclusive prefix of the tile counts + group sizes; few big segments -> one workgroup per segment
static void msm_colscan(lane_t& c, uint32_t* sizes, uint32_t nsegs, int bits, uint32_t* dmax) {
    if (nsegs <= 4096)
        hipLaunchKernelGGL(radix_colscan2_seg_kernel, dim3(nsegs), dim3(1024), 0, c.stream, c.rcounts2.as<uint32_t>(), c.roff2.as<uint32_t>(),
                           c.rtstart.as<uint32_t>(), sizes, nsegs, bits, dmax);
    else
        hipLaunchKernelGGL(radix_colscan2_kernel, dim3(((nsegs << bits) + 1 + 255) / 256), dim3(256), 0, c.stream, c.rcounts2.as<uint32_t>(),
                           c.roff2.as<uint32_t>(), c.rtstart.as<uint32_t>(), sizes, nsegs, bits, dmax);
}
// 3.-4. the further levels: items (v_in, rem_in) grouped in `nseg` segments -> grouped by (segment, next key bits); wide windows take a middle
// level of 7 bits first.  Leaves the bucket-major `sorted` and the bucket offsets boff.
template <class F>
static void msm_stage_sort_rest(lane_t& c, const msm_layout_t<F>& L, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    const size_t E_max = L.E_max;
    const uint32_t nbt = L.nbt;
    uint32_t* bsize = c.rbsize.as<uint32_t>();
    uint32_t* d_max = bsize + nbt + 1;
    uint32_t* boffp = c.boff.as<uint32_t>();
    const uint32_t* seg_start = c.rbinstart.as<uint32_t>();
    uint32_t nseg = L.nbins;
    const uint32_t* v_in = c.rv1.as<uint32_t>();
    if (L.wide) {
        ph.begin("msm_sort_level2");
        const uint32_t ngroups = nseg << 7;
        const size_t tmax = E_max / SORT_TILE + nseg + 1;
        c.rv2.ensure(E_max * 4);
        c.rl2.ensure(E_max);
        c.rmid_size.ensure(((size_t)ngroups + 3) * 4);
        c.rmid_boff.ensure(((size_t)ngroups + 3) * 4);
        c.scan_tmp.ensure(scan_tmp_elems((size_t)ngroups + 2) * 4);
        uint32_t* msize = c.rmid_size.as<uint32_t>();
        uint32_t* mboff = c.rmid_boff.as<uint32_t>();
        msm_tile_segments(c, seg_start, nseg);
        hipLaunchKernelGGL((radix_hist2_kernel<uint16_t>), dim3((unsigned)tmax), dim3(SORT_THREADS), 0, st, c.rl1.as<uint16_t>(), seg_start,
                           c.rtstart.as<uint32_t>(), c.rcounts2.as<uint32_t>(), nseg, 7, 7);
        HIP_TRY(hipMemsetAsync(msize + ngroups + 1, 0, 4, st));
        msm_colscan(c, msize, nseg, 7, msize + ngroups + 1);
        exclusive_scan_u32(st, msize, mboff, (size_t)ngroups + 1, c.scan_tmp.as<uint32_t>());
        hipLaunchKernelGGL((radix_scatter2_kernel<uint16_t, uint8_t>), dim3((unsigned)tmax), dim3(SORT_THREADS), 0, st, v_in, c.rl1.as<uint16_t>(),
                           seg_start, c.rtstart.as<uint32_t>(), c.rcounts2.as<uint32_t>(), c.roff2.as<uint32_t>(), mboff, c.rv2.as<uint32_t>(),
                           c.rl2.as<uint8_t>(), nseg, 7, 7, (uint32_t)tuning().xcd);
        ph.end();
        seg_start = mboff;
        nseg = ngroups;
        v_in = c.rv2.as<uint32_t>();
    }
    ph.begin(L.wide ? "msm_sort_level3" : "msm_sort_level2");
    msm_tile_segments(c, seg_start, nseg);
    const uint8_t* rem_last = L.wide ? c.rl2.as<uint8_t>() : c.rl1.as<uint8_t>();
    hipLaunchKernelGGL((radix_hist2_kernel<uint8_t>), dim3((unsigned)L.tiles2_max), dim3(SORT_THREADS), 0, st, rem_last, seg_start,
                       c.rtstart.as<uint32_t>(), c.rcounts2.as<uint32_t>(), nseg, L.LBL, 0);
    HIP_TRY(hipMemsetAsync(d_max, 0, 4, st));
    msm_colscan(c, bsize, nseg, L.LBL, d_max);
    exclusive_scan_u32(st, bsize, boffp, (size_t)nbt + 1, c.scan_tmp.as<uint32_t>());
    hipLaunchKernelGGL((radix_scatter2_kernel<uint8_t, uint8_t>), dim3((unsigned)L.tiles2_max), dim3(SORT_THREADS), 0, st, v_in, rem_last, seg_start,
                       c.rtstart.as<uint32_t>(), c.rcounts2.as<uint32_t>(), c.roff2.as<uint32_t>(), boffp, c.sorted.as<uint32_t>(),
                       (uint8_t*)nullptr, nseg, L.LBL, 0, (uint32_t)tuning().xcd);
    ph.end();
}
// 5. accumulate; returns the number of reduce rounds the tail runs in front of the fold.
// A single-round MSM (<= 2^22 digit entries: at most 2^16 accumulate threads) leaves at most 2^16 + nbt partial sums
// whatever the scalars are, and the tail kernels walk them position by position (msm.hip.h 7a/7b): no reduce round.
// Bigger MSMs run a FIXED number of reduce rounds (round 4: ONE round that shrinks a bucket's partial sums 16x; rounds 2-3: two of 8x) before the fold reads
// them twice - what uniform scalars need anyway (the top digit row of a 253-bit scalar fills only 2^(253 mod c) buckets,
// thousands of entries each) - and the flattened-list fold takes whatever is left of a heavier bucket (all scalars
// equal at 2^24: 2 048 partial sums in one bucket, 32 additions per lane of its row and column).  Nothing is read back:
// an MSM of any size is one uninterrupted enqueue (round 2 sized the rounds by the largest bucket: a 4-byte copy and
// a stream synchronisation between sort and accumulate).
template <class F>
static int msm_stage_accumulate(lane_t& c, const msm_layout_t<F>& L, const msm_job_t<F>& j, msm_phases_t& ph) {
    hipStream_t st = c.stream;
    const msm_multi_t* mu = j.multi;
    const uint32_t nbt = L.nbt;
    uint32_t* boffp = c.boff.as<uint32_t>();
    int rounds = 0;
    ph.begin("msm_accumulate");
    // a bucket of s entries is touched by at most (s - 1) / S + 2 segment threads
    const int env_rounds = tuning().reduce_rounds;
    if (!L.single_round) rounds = env_rounds < 0 ? 0 : (env_rounds > 8 ? 8 : env_rounds);
    // fused groups: optional reduce rounds (tuning fuse_reduce).  They bound what one fold workgroup can meet when an instance's
    // scalars are all equal (a 2^18-pair instance then leaves ~70 000 partial sums in ONE bucket: 1 100 dependent additions per
    // lane of its row) at the price of one more pass over the partial sums of well-behaved instances.
    if (mu && tuning().fuse_reduce > 0) rounds = tuning().fuse_reduce > 4 ? 4 : tuning().fuse_reduce;
    if (mu && tuning().fuse_reduce < 0) rounds = mu->K >= 8 ? 1 : 0;
    hipLaunchKernelGGL(msm_alloc_seg_kernel, dim3((nbt + 1 + 255) / 256), dim3(256), 0, st, boffp, c.cnt_a.as<uint32_t>(), nbt, L.pl.S);
    exclusive_scan_u32(st, c.cnt_a.as<uint32_t>(), c.start_a.as<uint32_t>(), (size_t)nbt + 1, c.scan_tmp.as<uint32_t>());
    msm_launch_accumulate<F>(c, L.pl, L.vbase, boffp, nbt, (L.E_max + L.pl.S - 1) / L.pl.S, L.single_round && L.prefetch_ok, L.ltail);
    ph.end();
    return rounds;
}
template <class T>
struct msm_field_tag {
    using type = T;
};
// fn(msm_field_tag<T>) for the arithmetic T the tail of an MSM over F runs on: fqz_t when a G1 accumulate kernel left raw lazy partial sums
// (`lazy`: tuning lazy_tail), else F's exact arithmetic
template <class F, class Fn>
static void msm_on_tail_field(bool lazy, Fn&& fn) {
    if constexpr (sizeof(F) == sizeof(fq_t)) {
        if (lazy) return fn(msm_field_tag<fqz_t>{});
    }
    fn(msm_field_tag<F>{});
}
// Device side of one MSM on lane `c`.  Everything is enqueued on the lane's stream, ending with the copy of the bit-plane sums into
// j.host_planes; the caller synchronises the stream and runs msm_collect / msm_accum_t::finish.  The steps, by number:
// 1. msm_stage_digits (or fused into 2.), 2. msm_stage_level1, 3.-4. msm_stage_sort_rest, 5. msm_stage_accumulate, 6.-9. msm_reduce_and_tail.
template <class F>
static msm_pending_t msm_run(lane_t& c, const msm_job_t<F>& j) {
    msm_pending_t pd;
    pd.planes = j.host_planes;
    if (j.n == 0) return pd;  // no planes: the sum is the point at infinity
    msm_phases_t ph{c, j.profile, msm_trace_level(), j.n};
    const msm_layout_t<F> L = msm_layout(c, j, pd);
    if (!L.fused) msm_stage_digits(c, L, j, ph);
    msm_stage_level1(c, L, j, ph);
    msm_stage_sort_rest(c, L, ph);
    const int rounds = msm_stage_accumulate(c, L, j, ph);
    // 6.-9. reduce rounds, then the bucket merge (a chunk of a bigger MSM) or fold -> bit-plane sums -> (host) Horner
    msm_on_tail_field<F>(L.ltail, [&](auto t) {
        msm_reduce_and_tail<typename decltype(t)::type>(c, L.pl, L.tg, L.nwin, L.nbt, rounds, L.T0_max, L.T1_max, j.sink, pd, j.host_planes, ph);
    });
    return pd;
}
// The tail of a chunked MSM: fold + bit planes over the bucket sink (every bucket holds L partial sums, one per lane).  Of the job it reads what the chunks'
// plan came from - n (the largest chunk), window_bits, tables, table_bits - and host_planes.
template <class F>
static msm_pending_t msm_tail_from_sink(lane_t& c, const msm_job_t<F>& j, const msm_bucket_sink_t& sink) {
    msm_pending_t pd;
    pd.planes = j.host_planes;
    const msm_plan_t pl = msm_make_plan(j.n, j.window_bits, j.tables, j.table_bits);
    const uint32_t nwin = (uint32_t)pl.W, nbt = nwin * pl.nb;
    if (nbt != sink.nbt) throw hip_failure{hipErrorInvalidValue, "msm: bucket sink does not match the plan", __LINE__};
    const msm_tail_geom_t tg = msm_tail_geometry(pl, nwin, pd, 0);
    c.start_a.ensure(((size_t)nbt + 1) * 4);
    c.cnt_a.ensure(((size_t)nbt + 1) * 4);
    hipLaunchKernelGGL(msm_sink_lists_kernel, dim3((nbt + 1 + 255) / 256), dim3(256), 0, c.stream, c.start_a.as<uint32_t>(), c.cnt_a.as<uint32_t>(), nbt, sink.L);
    pd.lazy = msm_lazy_tail_on<F>();  // the sink holds what the chunks' merges left: raw lazy points then
    c.phase_begin("msm_bucket_reduce");
    msm_on_tail_field<F>(pd.lazy, [&](auto t) {
        using T = typename decltype(t)::type;
        msm_tail_launch<T>(c, pl, tg, nwin, nbt, (const xyzz_mem_t<T>*)sink.acc, c.start_a.as<uint32_t>(), c.cnt_a.as<uint32_t>(), pd, j.host_planes);
    });
    c.phase_end();
    return pd;
}
// synchronous single MSM: run, wait, finish on the host into `out` (Jacobian memory image); the planes are staged in the lane's pinned block
template <class F>
static void msm_run_sync(lane_t& c, const msm_job_t<F>& j, void* out) {
    // A lane borrowed from the calling thread's scope: MSMs the scope enqueued on it (in-stream, or with no further lane free) keep their bit planes in
    // `pin` from offset 0 until the scope's flush has read them - this call stages at offset 0 too (and ensure() may move the block): deliver them first.
    if (c.in_scope && c.pin_used) scope_flush();
    c.pin.ensure(msm_plane_bytes<F>());
    msm_job_t<F> staged = j;
    staged.host_planes = c.pin.p;
    const msm_pending_t pd = msm_run<F>(c, staged);
    HIP_TRY(hipStreamSynchronize(c.stream));
    const double t0 = host_now_ms();
    msm_accum_t<F>* acc = new msm_accum_t<F>();
    std::unique_ptr<msm_accum_t<F>> hold(acc);
    msm_collect<F>(*acc, pd);
    acc->finish(out);
    c.phase_host("msm_host_finish", host_now_ms() - t0);  // the Horner chain over the bit planes, on the calling thread
}

template <class F>
static void convert_bases(lane_t& c, const uint8_t* d_in, size_t stride, size_t n, aff_mem_t<F>* d_out, hipStream_t st = nullptr, bool for_msm = false) {
    if (!n) return;
    const int form406 = for_msm && msm_lazy_on<F>() ? 1 : 0;
    hipLaunchKernelGGL((convert_bases_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st ? st : c.stream, d_in, stride, n, d_out, form406);
    HIP_TRY(hipGetLastError());
}
// the last step of a G1 registration: every slot of every table, exact internal form -> form406
static void bases_to_lazy_form(lane_t& c, g1_aff_mem_t* d, size_t slots) {
    if (!slots || !msm_lazy_on<fq_t>()) return;
    hipLaunchKernelGGL(g1_bases_to_form406_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, c.stream, d, slots);
    HIP_TRY(hipGetLastError());
}
#ifndef SV_NO_G2
static void bases_to_lazy_form(lane_t& c, aff_mem_t<fq2_t>* d, size_t slots) {
    if (!slots || !msm_lazy_on<fq2_t>()) return;
    hipLaunchKernelGGL(g2_bases_to_form406_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, c.stream, d, slots);
    HIP_TRY(hipGetLastError());
}
#endif

// Precomputed base tables of a registered vector: table j = 2^(table_bits * j) * P_i, from table j - 1 (msm.hip.h).  Long
// vectors give every thread a run of points that share one inversion; a run of 1 keeps small vectors parallel.
template <class F>
static void precompute_tables_run(lane_t& c, aff_mem_t<F>* d, size_t n, int tables, int table_bits) {
    if (tables <= 1 || !n) return;
    int run = (int)(n >> 16);
    run = run < 1 ? 1 : (run > PRE_RUN ? PRE_RUN : run);
    const size_t slab = n < PRE_SLAB ? n : PRE_SLAB;
    c.gen_pts.ensure(4 * slab * sizeof(typename F::mem_t));
    for (int j = 1; j < tables; j++)
        for (size_t lo = 0; lo < n; lo += PRE_SLAB) {
            const size_t cnt = n - lo < PRE_SLAB ? n - lo : PRE_SLAB;
            const size_t threads = (cnt + run - 1) / run;
            hipLaunchKernelGGL((precompute_table_kernel<F>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c.stream, d + (size_t)(j - 1) * n + lo,
                               d + (size_t)j * n + lo, cnt, table_bits, run, (typename F::mem_t*)c.gen_pts.p);
        }
    HIP_TRY(hipGetLastError());
}
