// api_g2.hip - the G2 (Fq2) entry points of the C ABI: the MSM engine, table precomputation and point encoding instantiated
// over fq2_t, behind the front end shared with G1 (msm_registered.hip.h).  A separate translation unit only because these instantiations
// are half of the compile time: build.py compiles the units in parallel.
#include "msm_registered.hip.h"
#include "serde.hip.h"

// this unit launches the scans (the G2 MSMs)
static void tu_set_kernel_attributes() {
    HIP_TRY(hipFuncSetAttribute((const void*)scan_one_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SCAN_ONE_MAX * 4)));
}

extern "C" {

void snarkvm_hip_free_bases_g2(snarkvm_hip_bases_g2_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}

#ifdef SV_NO_G2  // development builds only (python -m snarkvm_amd.build --fast): skips the Fq2 kernel instantiations; every entry point refuses
static RustError no_g2() { return from_failure(hip_failure{hipErrorNotSupported, "this development build was compiled without G2 (SV_NO_G2)", __LINE__}); }
RustError snarkvm_hip_msm_g2(void*, const void*, size_t, const void*, size_t) { return no_g2(); }
RustError snarkvm_hip_register_bases_g2(snarkvm_hip_bases_g2_t**, const void*, size_t, size_t, int, int) { return no_g2(); }
RustError snarkvm_hip_msm_g2_registered(void*, const snarkvm_hip_bases_g2_t*, size_t, size_t, const void*, int, int) { return no_g2(); }
RustError snarkvm_hip_msm_g2_registered_batch(void*, const snarkvm_hip_bases_g2_t*, size_t, const size_t*, const size_t*, const void* const*, int, int) { return no_g2(); }
RustError snarkvm_hip_g2_deserialize(void*, const void*, size_t, int) { return no_g2(); }
RustError snarkvm_hip_g2_deserialize_compressed(void*, const void*, size_t, int) { return no_g2(); }
RustError snarkvm_hip_g2_serialize(void*, const void*, size_t, size_t) { return no_g2(); }
RustError snarkvm_hip_g2_serialize_compressed(void*, const void*, size_t, size_t) { return no_g2(); }
RustError snarkvm_hip_devtest_g2_tail_repeat(const void*, size_t, int, int, int, int, int, int, int, uint32_t*) { return no_g2(); }
#else

RustError snarkvm_hip_msm_g2(void* out, const void* points, size_t npoints, const void* scalars, size_t ffi_affine_sz) {
    API_TRY
    if (!out) throw hip_failure{hipErrorInvalidValue, "msm_g2: null output", __LINE__};
    g_rt.configure();
    if (npoints == 0) {
        write_infinity<fq2_t>(out);
    } else {
        if (!points || !scalars) throw hip_failure{hipErrorInvalidValue, "msm_g2: null argument", __LINE__};
        msm_host_chunked<fq2_t>(out, points, npoints, scalars, ffi_affine_sz);
    }
    API_CATCH
}

// ---- registered G2 bases (extension): same engine over fq2_t, precomputed tables remove most of the Horner chain of a
// one-shot G2 MSM
RustError snarkvm_hip_register_bases_g2(snarkvm_hip_bases_g2_t** handle, const void* points, size_t npoints, size_t ffi_affine_sz, int tables,
                                        int window_bits) {
    API_TRY
    if (!handle || (npoints && !points)) throw hip_failure{hipErrorInvalidValue, "register_bases_g2: null argument", __LINE__};
    if (ffi_affine_sz < 200 || (ffi_affine_sz & 7)) throw hip_failure{hipErrorInvalidValue, "register_bases_g2: bad stride", __LINE__};
    check_tables(tables, window_bits, "register_bases_g2");
    *handle = bases_build<fq2_t>(npoints, tables, window_bits ? window_bits : 256 / tables,
                                 [&](lane_t& c, aff_mem_t<fq2_t>* table0) { bases_fill_from_host<fq2_t>(c, points, npoints, ffi_affine_sz, table0); });
    API_CATCH
}
// One G2 MSM over a registered range (msm_registered.hip.h::msm_registered_single; an empty one is answered on return, also inside a scope)
RustError snarkvm_hip_msm_g2_registered(void* out, const snarkvm_hip_bases_g2_t* h, size_t offset, size_t npoints, const void* scalars,
                                        int scalars_on_device, int window_bits) {
    API_TRY
    if (!h || offset + npoints > h->n) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered: range exceeds the registered bases", __LINE__};
    if (!msm_window_bits_ok(window_bits)) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered: window_bits must be 0 or 2..23", __LINE__};
    if (!out || (npoints && !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered: null argument", __LINE__};
    msm_req_t one;
    one.off0 = offset, one.n0 = npoints, one.scalars = scalars, one.out = out;
    msm_registered_single<fq2_t>(*h, one, scalars_on_device, 0, window_bits, false);
    API_CATCH
}
// A batch of independent G2 MSMs over one registered vector (BASELINE configs[4]: one per proof), fanned out like the G1 batch.
RustError snarkvm_hip_msm_g2_registered_batch(void* outs, const snarkvm_hip_bases_g2_t* h, size_t count, const size_t* offsets, const size_t* npoints,
                                              const void* const* scalars, int scalars_on_device, int window_bits) {
    API_TRY
    if (!h) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered_batch: null handle", __LINE__};
    if (!msm_window_bits_ok(window_bits)) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered_batch: window_bits must be 0 or 2..23", __LINE__};
    if (count && (!outs || !offsets || !npoints || !scalars)) throw hip_failure{hipErrorInvalidValue, "msm_g2_registered_batch: null argument", __LINE__};
    std::vector<msm_req_t> req = msm_requests<fq2_t>(outs, count, offsets, npoints, nullptr, nullptr, scalars);
    msm_batch_dispatch<fq2_t>(*h, req, scalars_on_device, 0, window_bits);
    API_CATCH
}

static RustError g2_deserialize_impl(void* out_affine, const void* bytes, size_t n, int compressed, int validate) {
    API_BEGIN
    if (n) {
        if (!out_affine || !bytes) throw hip_failure{hipErrorInvalidValue, "g2_deserialize: null argument", __LINE__};
        const size_t psz = compressed ? 96 : 192;
        c.bases_tmp.ensure(n * psz);
        c.poly[0].ensure(n * 200);
        c.serde_status.ensure(4);
        HIP_TRY(hipMemcpyAsync(c.bases_tmp.p, bytes, n * psz, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemsetAsync(c.serde_status.p, 0, 4, c.stream));
        hipLaunchKernelGGL(g2_deserialize_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, c.bases_tmp.as<uint8_t>(), n, compressed, validate,
                           c.poly[0].as<uint8_t>(), c.serde_status.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        uint32_t st = 0;
        HIP_TRY(hipMemcpyAsync(&st, c.serde_status.p, 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(out_affine, c.poly[0].p, n * 200, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        serde_throw_on_status(st, "g2_deserialize");
    }
    API_END
}
static RustError g2_serialize_impl(void* out_bytes, const void* affine, size_t n, size_t ffi_affine_sz, int compressed) {
    API_BEGIN
    if (n) {
        if (!out_bytes || !affine) throw hip_failure{hipErrorInvalidValue, "g2_serialize: null argument", __LINE__};
        if (ffi_affine_sz < 200 || (ffi_affine_sz & 7)) throw hip_failure{hipErrorInvalidValue, "g2_serialize: bad stride", __LINE__};
        c.bases_tmp.ensure(n * ffi_affine_sz);
        const size_t psz = compressed ? 96 : 192;
        c.poly[0].ensure(n * psz);
        HIP_TRY(hipMemcpyAsync(c.bases_tmp.p, affine, n * ffi_affine_sz, hipMemcpyHostToDevice, c.stream));
        hipLaunchKernelGGL(g2_serialize_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream, c.bases_tmp.as<uint8_t>(), ffi_affine_sz, n,
                           compressed, c.poly[0].as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_bytes, c.poly[0].p, n * psz, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    API_END
}

RustError snarkvm_hip_g2_deserialize(void* out_affine, const void* bytes, size_t n, int validate) { return g2_deserialize_impl(out_affine, bytes, n, 0, validate); }
RustError snarkvm_hip_g2_deserialize_compressed(void* out_affine, const void* bytes, size_t n, int validate) {
    return g2_deserialize_impl(out_affine, bytes, n, 1, validate);
}
RustError snarkvm_hip_g2_serialize(void* out_bytes, const void* affine, size_t n, size_t ffi_affine_sz) { return g2_serialize_impl(out_bytes, affine, n, ffi_affine_sz, 0); }
RustError snarkvm_hip_g2_serialize_compressed(void* out_bytes, const void* affine, size_t n, size_t ffi_affine_sz) {
    return g2_serialize_impl(out_bytes, affine, n, ffi_affine_sz, 1);
}

// The G2 fold and bit-plane kernels launched `iters` times over ONE fixed set of per-bucket partial-sum lists (2^(m + hb) buckets of one window; 0, 1 or 2
// entries per bucket - the sparse shape of a small MSM over window tables - built from +- points[k]): every launch must leave the same group elements.
// A difference is a race or a lost register, whatever the points are.  threads: per fold workgroup (64, 128, 256);
// plane_threads likewise; hex / quads: the kernels' switches.  report[0] = fold launches that differ from the first, report[1] = differing fold slots in
// total, report[2] = bit-plane launches that differ from the first, report[3] = differing planes in total, report[4 .. 7] = the first differing fold slots, report[8], [9] = fold slots / planes of the first launch the fast
// kernels flagged for the fix kernels (equal x coordinates met on the way).
RustError snarkvm_hip_devtest_g2_tail_repeat(const void* points, size_t npoints, int m, int hb, int threads, int plane_threads, int hex, int quads, int iters,
                                             uint32_t* report) {
    API_BEGIN
    if (!points || npoints < 2 || !report || m < 1 || hb < 1 || hb > m || m + hb > 16 || iters < 2 || (threads != 64 && threads != 128 && threads != 256) ||
        (plane_threads != 64 && plane_threads != 128 && plane_threads != 256))
        throw hip_failure{hipErrorInvalidValue, "devtest_g2_tail_repeat: bad arguments", __LINE__};
    typedef xyzz_mem_t<fq2_t> mem_t;
    const uint32_t nb = 1u << (m + hb);
    std::vector<uint32_t> cnt(nb), start(nb);
    uint32_t E = 0;
    for (uint32_t k = 0; k < nb; k++) {
        const uint32_t h = (k * 2654435761u) >> 28;
        cnt[k] = h == 0 ? 2 : h == 1 ? 0 : 1;
        start[k] = E;
        E += cnt[k];
    }
    std::vector<mem_t> sums(E);
    for (uint32_t k = 0; k < nb; k++)
        for (uint32_t q = start[k]; q < start[k] + cnt[k]; q++) {
            const uint32_t q0 = start[k];  // both entries of a two-entry bucket are the same signed point: neighbours in every list, P + P in the first level that adds them
            const uint32_t* src = (const uint32_t*)((const uint8_t*)points + 200 * (size_t)((q0 * 7u + 3u) % npoints));
            xyzz_t<fq2_t> a = xyzz_t<fq2_t>::inf();
            a.add_affine({fq2_t::from_raw_words(src), fq2_t::from_raw_words(src + 24)}, ((q0 >> 3) & 1) != 0);
            store_xyzz<fq2_t>(&sums[q], a);
        }
    const size_t nslots = (size_t)1 << (m + 1), nbits = (size_t)m + 1, nplanes = 2 * nbits;
    c.part_a.ensure(E * sizeof(mem_t));
    c.cnt_a.ensure(nb * 4);
    c.start_a.ensure(nb * 4);
    c.fold_sums.ensure(2 * nslots * sizeof(mem_t));  // [0]: the first launch's output (the bit planes read it), [1]: the launch under test
    c.planes.ensure(nplanes * sizeof(mem_t));
    c.tail_flags.ensure((nslots + nplanes) * 4);
    std::vector<uint32_t> flag_copy(nslots + nplanes, 0);
    HIP_TRY(hipMemcpyAsync(c.part_a.p, sums.data(), E * sizeof(mem_t), hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipMemcpyAsync(c.cnt_a.p, cnt.data(), nb * 4, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipMemcpyAsync(c.start_a.p, start.data(), nb * 4, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipMemsetAsync(c.fold_sums.p, 0, 2 * nslots * sizeof(mem_t), c.stream));
    HIP_TRY(hipMemsetAsync(c.tail_flags.p, 0, (nslots + nplanes) * 4, c.stream));  // the buffer outlives an MSM: a slot no workgroup writes must not count with an earlier call's flag
    std::vector<uint8_t> first(nslots * sizeof(mem_t)), got(nslots * sizeof(mem_t)), p_first(nplanes * sizeof(mem_t)), p_got(nplanes * sizeof(mem_t));
    for (int i = 0; i < 10; i++) report[i] = 0;
    int nfirst = 0;
    auto same_point = [](const xyzz_t<fq2_t>& a, const xyzz_t<fq2_t>& b) {  // as group elements (the coordinates of a point at infinity are arbitrary)
        if (a.is_inf() || b.is_inf()) return a.is_inf() == b.is_inf();
        return a.x * b.zz == b.x * a.zz && a.y * b.zzz == b.y * a.zzz;
    };
    for (int it = 0; it < iters; it++) {
        mem_t* out = c.fold_sums.as<mem_t>() + (it ? nslots : 0);
        uint32_t* fold_flags = c.tail_flags.as<uint32_t>();
        uint32_t* plane_flags = fold_flags + nslots;
        const dim3 fold_grid((1u << m) + (1u << hb), 1u), plane_grid((unsigned)nbits, 2u);
        hipLaunchKernelGGL((msm_fold_kernel<fq2_t>), fold_grid, dim3((unsigned)threads), 0, c.stream, (const mem_t*)c.part_a.as<mem_t>(),
                           (const uint32_t*)c.start_a.as<uint32_t>(), (const uint32_t*)c.cnt_a.as<uint32_t>(), out, m, hb, hex, quads & 2 ? 1 : 0, fold_flags);
        hipLaunchKernelGGL((msm_fold_fix_kernel<fq2_t>), fold_grid, dim3(64), 0, c.stream, (const mem_t*)c.part_a.as<mem_t>(), (const uint32_t*)c.start_a.as<uint32_t>(),
                           (const uint32_t*)c.cnt_a.as<uint32_t>(), out, m, hb, (const uint32_t*)fold_flags);
        hipLaunchKernelGGL((msm_bitplane_kernel<fq2_t, true>), plane_grid, dim3((unsigned)plane_threads), 0, c.stream, (const mem_t*)c.fold_sums.as<mem_t>(),
                           (const uint32_t*)nullptr, (const uint32_t*)nullptr, c.planes.as<mem_t>(), nb, m, hb, hex, quads & 1, plane_flags);
        hipLaunchKernelGGL((msm_bitplane_fix_kernel<fq2_t, true>), plane_grid, dim3(64), 0, c.stream, (const mem_t*)c.fold_sums.as<mem_t>(), (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, c.planes.as<mem_t>(), nb, m, hb, (const uint32_t*)plane_flags);
        if (!it) HIP_TRY(hipMemcpyAsync(flag_copy.data(), fold_flags, (nslots + nplanes) * 4, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(it ? got.data() : first.data(), out, nslots * sizeof(mem_t), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(it ? p_got.data() : p_first.data(), c.planes.p, nplanes * sizeof(mem_t), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (!it) continue;
        uint32_t bad = 0;
        for (size_t sl = 0; sl + 1 < nslots; sl++)  // (the last slot is never written)
            if (!same_point(load_xyzz<fq2_t>((const mem_t*)&first[sl * sizeof(mem_t)]), load_xyzz<fq2_t>((const mem_t*)&got[sl * sizeof(mem_t)]))) {
                bad++;
                if (nfirst < 4) report[4 + nfirst++] = (uint32_t)sl;
            }
        report[0] += bad ? 1 : 0;
        report[1] += bad;
        bad = 0;
        for (size_t pl = 0; pl < nplanes; pl++)
            if (!same_point(load_xyzz<fq2_t>((const mem_t*)&p_first[pl * sizeof(mem_t)]), load_xyzz<fq2_t>((const mem_t*)&p_got[pl * sizeof(mem_t)]))) bad++;
        report[2] += bad ? 1 : 0;
        report[3] += bad;
    }
    report[8] = report[9] = 0;  // outputs of the first launch the fast kernels flagged (fold slots, planes): the fix kernels' share of the work
    for (size_t sl = 0; sl + 1 < nslots; sl++) report[8] += flag_copy[sl] ? 1 : 0;  // (the slots no workgroup writes were cleared above)
    for (size_t pl = 0; pl < nplanes; pl++) report[9] += flag_copy[nslots + pl] ? 1 : 0;
    API_END
}

#endif  // SV_NO_G2

}  // extern "C"
