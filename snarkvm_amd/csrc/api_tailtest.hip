// api_tailtest.hip - test hook for the tail of the variable-base MSM (snarkvm_hip_devtest_msm_tail): the reduce round, the bucket merge, the fold and the
// bit-plane kernels of msm.hip.h 6.-7b launched ONCE over caller-chosen partial-sum lists, in the order and with the arguments msm_run.hip.h::msm_reduce_and_tail /
// msm_tail_launch give them, every output copied back as an exact projective point.  The lists are built on the host with the exact arithmetic (general ZZ / ZZZ,
// optionally another representative of the same point) and converted to the arithmetic under test (fq_t, fqz_t, fq2_t).  Every output buffer is filled with 0xff
// before the launch: an output no workgroup writes comes back marked as such, never as a plausible point.
// A translation unit of its own (as api_msmtest.hip): the units that own the MSM entry points and the tail_*.hip units compile exactly as before; the fold and
// bit-plane kernels are referenced through their external handles (msm.hip.h SV_TAIL_KERNELS), the small reduce / merge kernels are instantiated here.
#include "msm_run.hip.h"
#include "testrng.hip.h"

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

namespace {

enum { TT_REDUCE = 0, TT_MERGE, TT_FOLD, TT_SPARSE };
struct tt_geom_t {
    int m, hb, W, nb, S2, L, slot, fold_threads, plane_threads, hex, quads, run_fix;
};
struct tt_args_t {
    int stage;
    tt_geom_t g;
    const uint8_t* points;
    size_t npoints;
    const int32_t* terms;
    const uint64_t* seeds;
    size_t nentries;
    const uint32_t *start, *cnt;
    size_t nbt;
    uint32_t *out, *status, *flags;
    size_t nout;
    uint32_t* aux;
};
[[noreturn]] void tt_bad(const char* what, int line) { throw hip_failure{hipErrorInvalidValue, what, line}; }

template <class E>
E tt_scale(uint64_t seed);  // a non-zero field element derived from the seed
template <>
fq_t tt_scale<fq_t>(uint64_t seed) {
    fq_t l = fq_t::zero();
    splitmix64_t next{seed};
    for (int i = 0; i < 12; i++) l.v[i] = (uint32_t)(next() & LIMB_MASK);
    l.v[0] |= 1;
    return l;
}
template <>
fq2_t tt_scale<fq2_t>(uint64_t seed) {
    return {tt_scale<fq_t>(seed), tt_scale<fq_t>(~seed)};
}
// exact point -> the memory image of the arithmetic T; the point at infinity as the all-zero image (a zero-initialised sink slot, an empty partial sum)
template <class T, class E>
void tt_put(xyzz_mem_t<T>* dst, const xyzz_t<E>& a) {
    if (a.is_inf()) {
        memset(dst, 0, sizeof *dst);
        return;
    }
    if constexpr (std::is_same<T, fqz_t>::value)
        store_xyzz<fqz_t>(dst, xyzz_t<fqz_t>{{fql_t::from_exact(a.x)}, {fql_t::from_exact(a.y)}, {fql_t::from_exact(a.zz)}, {fql_t::from_exact(a.zzz)}});
    else
        store_xyzz<T>(dst, a);
}
template <class T, class E>
xyzz_t<E> tt_get(const xyzz_mem_t<T>* src) {
    const xyzz_t<T> p = load_xyzz<T>(src);
    if constexpr (std::is_same<T, fqz_t>::value) {
        if (p.is_inf()) return xyzz_t<E>::inf();
        return {p.x.to_exact(), p.y.to_exact(), p.zz.to_exact(), p.zzz.to_exact()};
    } else {
        return p;
    }
}
bool tt_is_fill(const void* p, size_t bytes) {
    for (size_t i = 0; i < bytes; i++)
        if (((const uint8_t*)p)[i] != 0xff) return false;
    return true;
}
int tt_log2(uint32_t v) {
    int l = 0;
    while ((1u << l) < v) l++;
    return l;
}

// T: the arithmetic of the kernels, E: the exact field of the group, STRIDE: bytes of one affine point of `points`
template <class T, class E, size_t STRIDE>
void tt_run(lane_t& c, const tt_args_t& a) {
    typedef xyzz_mem_t<T> mem_t;
    constexpr bool G2 = std::is_same<E, fq2_t>::value;
    constexpr size_t CW = sizeof(typename E::mem_t) / 4;  // words per coordinate
    const tt_geom_t& g = a.g;
    const size_t nbt = a.nbt, nacc = a.stage == TT_MERGE ? nbt * (size_t)g.L : 0, nent = a.nentries + nacc;
    hipStream_t st = c.stream;
    // ---- the entries ----
    std::vector<aff_t<E>> pool(a.npoints);
    for (size_t i = 0; i < a.npoints; i++) {
        const uint32_t* src = (const uint32_t*)(a.points + STRIDE * i);
        pool[i] = {E::from_raw_words(src), E::from_raw_words(src + CW)};
        if (pool[i].is_inf()) tt_bad("devtest_msm_tail: a pool point at infinity", __LINE__);
    }
    std::vector<mem_t> ent(nent ? nent : 1);
    for (size_t e = 0; e < nent; e++) {
        xyzz_t<E> p = xyzz_t<E>::inf();
        for (int j = 0; j < 3; j++) {
            const int32_t t = a.terms[3 * e + j];
            if (!t) continue;
            const size_t idx = (size_t)(t < 0 ? -(int64_t)t : (int64_t)t) - 1;
            if (idx >= a.npoints) tt_bad("devtest_msm_tail: a term outside the pool", __LINE__);
            p.add_affine(pool[idx], t < 0);
        }
        if (a.seeds[e] && !p.is_inf()) {
            const E l = tt_scale<E>(a.seeds[e]), l2 = l.sqr(), l3 = l2 * l;
            p = {p.x * l2, p.y * l3, p.zz * l2, p.zzz * l3};
        }
        tt_put<T, E>(&ent[e], p);
    }
    c.part_a.ensure((a.nentries + 1) * sizeof(mem_t));
    c.start_a.ensure((nbt + 1) * 4);
    c.cnt_a.ensure((nbt + 1) * 4);
    if (a.nentries) HIP_TRY(hipMemcpyAsync(c.part_a.p, ent.data(), a.nentries * sizeof(mem_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.start_a.p, a.start, (nbt + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.cnt_a.p, a.cnt, nbt * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c.cnt_a.as<uint32_t>() + nbt, 0, 4, st));
    const mem_t* sums = c.part_a.as<mem_t>();
    const uint32_t *start = c.start_a.as<uint32_t>(), *cnt = c.cnt_a.as<uint32_t>();
    std::vector<mem_t> got(a.nout);
    std::vector<uint32_t> flag_copy(a.nout, 0);
    if (a.stage == TT_REDUCE) {  // msm_reduce_and_tail, one round
        c.cnt_b.ensure((nbt + 1) * 4);
        c.start_b.ensure((nbt + 1) * 4);
        c.scan_tmp.ensure(scan_tmp_elems(nbt + 1) * 4);
        c.part_b.ensure(a.nout * sizeof(mem_t));
        HIP_TRY(hipMemsetAsync(c.part_b.p, 0xff, a.nout * sizeof(mem_t), st));
        HIP_TRY(hipMemsetAsync(c.start_b.p, 0xff, (nbt + 1) * 4, st));
        hipLaunchKernelGGL(msm_alloc_kernel, dim3((unsigned)((nbt + 1 + 255) / 256)), dim3(256), 0, st, cnt, c.cnt_b.as<uint32_t>(), (uint32_t)nbt, (uint32_t)g.S2);
        exclusive_scan_u32(st, c.cnt_b.as<uint32_t>(), c.start_b.as<uint32_t>(), nbt + 1, c.scan_tmp.as<uint32_t>());
        hipLaunchKernelGGL((msm_reduce_kernel<T>), dim3((unsigned)((a.nout + 255) / 256)), dim3(256), 0, st, sums, start, cnt, (const uint32_t*)c.start_b.as<uint32_t>(),
                           c.part_b.as<mem_t>(), (uint32_t)nbt, (uint32_t)g.S2);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(a.aux, c.start_b.p, (nbt + 1) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(got.data(), c.part_b.p, a.nout * sizeof(mem_t), hipMemcpyDeviceToHost, st));
    } else if (a.stage == TT_MERGE) {
        c.part_b.ensure(nacc * sizeof(mem_t));
        HIP_TRY(hipMemcpyAsync(c.part_b.p, ent.data() + a.nentries, nacc * sizeof(mem_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((msm_bucket_merge_kernel<T>), dim3((unsigned)((nbt + 255) / 256)), dim3(256), 0, st, sums, start, cnt, c.part_b.as<mem_t>(), (uint32_t)nbt,
                           (uint32_t)g.L, (uint32_t)g.slot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(got.data(), c.part_b.p, nacc * sizeof(mem_t), hipMemcpyDeviceToHost, st));
    } else {  // msm_tail_launch
        const bool fold = a.stage == TT_FOLD;
        const int nbits = fold ? g.m + 1 : tt_log2((uint32_t)g.nb) + 1;
        const size_t nslots = fold ? (size_t)g.W << (g.m + 1) : 0, nplanes = (size_t)(fold ? 2 * g.W : g.W) * nbits;
        c.fold_sums.ensure((nslots + 1) * sizeof(mem_t));
        c.planes.ensure(nplanes * sizeof(mem_t));
        c.tail_flags.ensure((nslots + nplanes) * 4);
        HIP_TRY(hipMemsetAsync(c.fold_sums.p, 0xff, (nslots + 1) * sizeof(mem_t), st));
        HIP_TRY(hipMemsetAsync(c.planes.p, 0xff, nplanes * sizeof(mem_t), st));
        HIP_TRY(hipMemsetAsync(c.tail_flags.p, 0xff, (nslots + nplanes) * 4, st));
        uint32_t* fold_flags = G2 ? c.tail_flags.as<uint32_t>() : nullptr;
        uint32_t* plane_flags = G2 ? fold_flags + nslots : nullptr;
        mem_t* fs = c.fold_sums.as<mem_t>();
        mem_t* planes = c.planes.as<mem_t>();
        const dim3 plane_grid((unsigned)nbits, (unsigned)(fold ? 2 * g.W : g.W));
        if (fold) {
            const dim3 fold_grid((1u << g.m) + (1u << g.hb), (unsigned)g.W);
            hipLaunchKernelGGL((msm_fold_kernel<T>), fold_grid, dim3((unsigned)g.fold_threads), 0, st, sums, start, cnt, fs, g.m, g.hb, g.hex, (g.quads >> 1) & 1, fold_flags);
            if constexpr (TAIL_FLAGGED<T>::value)
                if (g.run_fix) hipLaunchKernelGGL((msm_fold_fix_kernel<T>), fold_grid, dim3(64), 0, st, sums, start, cnt, fs, g.m, g.hb, (const uint32_t*)fold_flags);
            hipLaunchKernelGGL((msm_bitplane_kernel<T, true>), plane_grid, dim3((unsigned)g.plane_threads), 0, st, (const mem_t*)fs, (const uint32_t*)nullptr,
                               (const uint32_t*)nullptr, planes, (uint32_t)1 << (g.m + g.hb), g.m, g.hb, g.hex, g.quads & 1, plane_flags);
            if constexpr (TAIL_FLAGGED<T>::value)
                if (g.run_fix)
                    hipLaunchKernelGGL((msm_bitplane_fix_kernel<T, true>), plane_grid, dim3(64), 0, st, (const mem_t*)fs, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                                       planes, (uint32_t)1 << (g.m + g.hb), g.m, g.hb, (const uint32_t*)plane_flags);
        } else {
            hipLaunchKernelGGL((msm_bitplane_kernel<T, false>), plane_grid, dim3((unsigned)g.plane_threads), 0, st, sums, start, cnt, planes, (uint32_t)g.nb, 0, 0, g.hex, 0,
                               plane_flags);
            if constexpr (TAIL_FLAGGED<T>::value)
                if (g.run_fix)
                    hipLaunchKernelGGL((msm_bitplane_fix_kernel<T, false>), plane_grid, dim3(64), 0, st, sums, start, cnt, planes, (uint32_t)g.nb, 0, 0, (const uint32_t*)plane_flags);
        }
        HIP_TRY(hipGetLastError());
        if (nslots) HIP_TRY(hipMemcpyAsync(got.data(), fs, nslots * sizeof(mem_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(got.data() + nslots, planes, nplanes * sizeof(mem_t), hipMemcpyDeviceToHost, st));
        if (G2) HIP_TRY(hipMemcpyAsync(flag_copy.data(), c.tail_flags.p, (nslots + nplanes) * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // ---- the outputs as exact projective points ----
    for (size_t i = 0; i < a.nout; i++) {
        uint32_t* dst = a.out + 3 * CW * i;
        a.flags[i] = flag_copy[i];
        if (a.stage != TT_MERGE && tt_is_fill(&got[i], sizeof(mem_t))) {
            a.status[i] = 1;
            memset(dst, 0xff, 3 * CW * 4);
            continue;
        }
        a.status[i] = (a.stage == TT_MERGE && memcmp(&got[i], &ent[a.nentries + i], sizeof(mem_t)) == 0) ? 2u : 0u;
        const jac_t<E> j = tt_get<T, E>(&got[i]).to_jacobian();
        j.x.to_raw_words(dst);
        j.y.to_raw_words(dst + CW);
        j.z.to_raw_words(dst + 2 * CW);
    }
}

}  // namespace

extern "C" {

RustError snarkvm_hip_devtest_msm_tail(int arith, int stage, const int32_t* geom, const void* points, size_t npoints, const int32_t* terms, const uint64_t* seeds,
                                       size_t nentries, const uint32_t* start, const uint32_t* cnt, size_t nbt, void* out, uint32_t* status, uint32_t* flags, size_t nout,
                                       uint32_t* aux) {
    API_BEGIN
    if (arith < 0 || arith > 2 || stage < TT_REDUCE || stage > TT_SPARSE) tt_bad("devtest_msm_tail: arith must be 0 .. 2, stage 0 .. 3", __LINE__);
#ifdef SV_NO_G2
    if (arith == 2) throw hip_failure{hipErrorNotSupported, "this development build was compiled without G2 (SV_NO_G2)", __LINE__};
#endif
    if (!geom || !points || !terms || !seeds || !start || !cnt || !out || !status || !flags || (stage == TT_REDUCE && !aux))
        tt_bad("devtest_msm_tail: null argument", __LINE__);
    tt_args_t a;
    a.stage = stage;
    a.g = {geom[0], geom[1], geom[2], geom[3], geom[4], geom[5], geom[6], geom[7], geom[8], geom[9], geom[10], geom[11]};
    const tt_geom_t& g = a.g;
    auto threads_ok = [](int t) { return t == 64 || t == 128 || t == 256; };
    if (npoints == 0 || npoints > 4096 || nbt == 0 || nbt > ((size_t)1 << 17) || nentries > ((size_t)1 << 20)) tt_bad("devtest_msm_tail: sizes out of range", __LINE__);
    if ((g.hex != 0 && g.hex != 1) || g.quads < 0 || g.quads > 3 || (g.run_fix != 0 && g.run_fix != 1) || (arith != 2 && (g.hex || g.run_fix)))
        tt_bad("devtest_msm_tail: hex, quads or run_fix out of range (hex and run_fix are G2 switches)", __LINE__);
    size_t want_out = 0;
    bool contiguous = false;
    if (stage == TT_REDUCE) {
        if (g.S2 < 2 || g.S2 > 64) tt_bad("devtest_msm_tail: S2 must be 2 .. 64", __LINE__);
        size_t T = 0;
        for (size_t k = 0; k < nbt; k++) T += ((size_t)cnt[k] + g.S2 - 1) / g.S2;
        if (nout < T || nout > T + 4096 || nout == 0) tt_bad("devtest_msm_tail: nout must cover the round's partial sums (and at most 4096 more)", __LINE__);
        want_out = nout;
    } else if (stage == TT_MERGE) {
        if (g.L < 1 || g.L > 8 || g.slot < 0 || g.slot >= g.L) tt_bad("devtest_msm_tail: L must be 1 .. 8, slot < L", __LINE__);
        want_out = nbt * (size_t)g.L;
    } else if (stage == TT_FOLD) {
        if (g.m < 1 || g.hb < 1 || g.hb > g.m || g.hb > 11 || g.m > 11 || g.W < 1 || g.W > 64) tt_bad("devtest_msm_tail: fold geometry out of range (1 <= hb <= m <= 11)", __LINE__);
        if (!threads_ok(g.fold_threads) || !threads_ok(g.plane_threads)) tt_bad("devtest_msm_tail: threads must be 64, 128 or 256", __LINE__);
        if (((g.quads & 2) && g.fold_threads == 64) || ((g.quads & 1) && g.plane_threads == 64)) tt_bad("devtest_msm_tail: no quad-strided loop with 64 threads", __LINE__);
        if (nbt != ((size_t)g.W << (g.m + g.hb))) tt_bad("devtest_msm_tail: nbt must be W * 2^(m + hb)", __LINE__);
        want_out = ((size_t)g.W << (g.m + 1)) + 2 * (size_t)g.W * (g.m + 1);
        contiguous = true;
    } else {
        if (g.nb < 2 || g.nb > 1024 || (g.nb & (g.nb - 1)) || g.W < 1 || g.W > 64) tt_bad("devtest_msm_tail: nb must be a power of two, 2 .. 1024", __LINE__);
        if (!threads_ok(g.plane_threads) || g.quads) tt_bad("devtest_msm_tail: threads must be 64, 128 or 256, and the unfolded planes have no quad-strided loop", __LINE__);
        if (nbt != (size_t)g.W * g.nb) tt_bad("devtest_msm_tail: nbt must be W * nb", __LINE__);
        int nbits = 1;
        while ((1 << (nbits - 1)) < g.nb) nbits++;
        want_out = (size_t)g.W * nbits;
        contiguous = true;
    }
    if (nout != want_out) tt_bad("devtest_msm_tail: nout does not match the stage's outputs", __LINE__);
    for (size_t k = 0; k < nbt; k++) {
        if ((size_t)start[k] + cnt[k] > nentries) tt_bad("devtest_msm_tail: a list overruns the entries", __LINE__);
        if (contiguous && start[k + 1] != start[k] + cnt[k]) tt_bad("devtest_msm_tail: the fold and the bit planes walk lists laid out bucket after bucket", __LINE__);
    }
    if (contiguous && (start[0] != 0 || start[nbt] != nentries)) tt_bad("devtest_msm_tail: the lists must cover the entries", __LINE__);
    a.points = (const uint8_t*)points;
    a.npoints = npoints;
    a.terms = terms;
    a.seeds = seeds;
    a.nentries = nentries;
    a.start = start;
    a.cnt = cnt;
    a.nbt = nbt;
    a.out = (uint32_t*)out;
    a.status = status;
    a.flags = flags;
    a.nout = nout;
    a.aux = aux;
    if (arith == 0) tt_run<fq_t, fq_t, 104>(c, a);
    if (arith == 1) tt_run<fqz_t, fq_t, 104>(c, a);
#ifndef SV_NO_G2
    if (arith == 2) tt_run<fq2_t, fq2_t, 200>(c, a);
#endif
    API_END
}

}  // extern "C"
