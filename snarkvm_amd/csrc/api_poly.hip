// api_poly.hip - the polynomial entry points of the C ABI over Fr vectors (poly.hip.h): the vector passes, the division by X - z (Horner) and
// by a vanishing polynomial, batch inversion, powers, Lagrange coefficients, fr_lincomb, fr_open_fold, the reductions and the support pass, each
// with its host twin and geometry hook.  The frame they share: fr_call.hip.h.
#include "fr_call.hip.h"

#include <array>
#include <map>

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

// the butterflies of fr_block_sum / fr_block_support over `vals` (one per thread): lanes l and l ^ off meet, then the waves' values
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

// The two routes of a suffix Horner sweep over n coefficients (fr_horner_sweep).
// route 1: the three-launch scan (C coefficients per thread, `blocks` workgroups of HORNER2_B); route 0: the chunk recursion (C = POLY_CHUNK,
// `blocks` workgroups of 256 at its level 0).
struct fr_horner_geometry_t {
    int route;
    uint32_t C;
    size_t blocks;
};
static fr_horner_geometry_t fr_horner_geometry(size_t n, bool want_quotient) {
    if (want_quotient && n >= 2048 && n <= ((size_t)1 << 20) && tuning().horner2) {
        // quotient wanted, a proof-sized polynomial: the three-launch form with a scan inside every workgroup (poly.hip.h); C coefficients per thread keep
        // <= 256 workgroups.  (Beyond 2^20 coefficients a thread would fold 32+ of them serially on a quarter of the chip's lanes - round 3 measured that
        // shape at 2^24: 1.69 vs 1.04 ms - and the chunk recursion, 2^19 threads at its first level, is the better form.)
        uint32_t C = 8;
        while (((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B > 256) C *= 2;
        return {1, C, ((n + C - 1) / C + HORNER2_B - 1) / HORNER2_B};
    }
    const size_t T = (n + POLY_CHUNK - 1) / POLY_CHUNK;
    return {0, (uint32_t)POLY_CHUNK, (T + 255) / 256};
}
// the sizes of the levels of the chunk recursion: n, then the chunk values of the level below until one is left (always at least two levels:
// the chunk values of level 0 exist even for a single coefficient)
static std::vector<size_t> fr_horner_levels(size_t n, size_t chunk) {
    std::vector<size_t> sizes{n};
    do sizes.push_back((sizes.back() + chunk - 1) / chunk);
    while (sizes.back() > 1);
    return sizes;
}

// One suffix Horner sweep, h_i = sum_{k >= i} a_k m^(k - i), over `count` vectors of n coefficients (blockIdx.y) on the lane's stream, for the plain
// division and the opening fold alike: the workspace in the lane's poly[4], the level table and the launches - the constructor lays out and
// enqueues the multipliers or tables, up() one sweep up, down() the sweep down behind it.  Level 0 is walked through the caller's span policy
// (poly.hip.h), the levels above it - chunk values - through the plain policy in place.
//   route 1: tab | hs[count][blocks 256] | bv[count][blocks] | kept[keep]
//   route 0: mult[top + 1] | cv[count][levels 1 .. top - 1] | kept[keep]
// kept: the caller's `keep` elements.  Route 0 puts the single value of the top level - h_0 - of vector y of the sweep up(walk, slot) at
// kept[slot count + y]; the rest is the caller's own.
struct fr_horner_sweep {
    lane_t& c;
    const fr_horner_geometry_t g;
    const size_t n, count;
    const fr_mem_t m;
    std::vector<size_t> sizes, off;  // route 0: level k has sizes[k] values, those of 1 <= k < top at cv + off[k]
    int top = 0;
    size_t total = 0;
    fr_mem_t *head = nullptr, *hs = nullptr, *bv = nullptr, *cv = nullptr, *kept = nullptr;

    fr_horner_sweep(lane_t& c, const fr_horner_geometry_t& g, size_t n, const fr_mem_t& m, size_t count, size_t keep) : c(c), g(g), n(n), count(count), m(m) {
        if (g.route == 1) {
            const size_t hs_n = count * g.blocks * HORNER2_B, bv_n = count * g.blocks;
            c.poly[4].ensure(sizeof(fr_mem_t) * (HORNER2_TAB + hs_n + bv_n + keep));
            head = c.poly[4].as<fr_mem_t>(), hs = head + HORNER2_TAB, bv = hs + hs_n, kept = bv + bv_n;
            hipLaunchKernelGGL(fr_horner2_tables_kernel, dim3(1), dim3(HORNER2_B), 0, c.stream, m, head, g.C);
            return;
        }
        sizes = fr_horner_levels(n, POLY_CHUNK);
        top = (int)sizes.size() - 1;
        off.assign(sizes.size(), 0);
        for (int k = 1; k < top; k++) off[k] = total, total += sizes[k];
        c.poly[4].ensure(sizeof(fr_mem_t) * ((size_t)top + 1 + count * total + keep));
        head = c.poly[4].as<fr_mem_t>(), cv = head + top + 1, kept = cv + count * total;
        hipLaunchKernelGGL(fr_horner_multipliers_kernel, dim3(1), dim3(1), 0, c.stream, m, head, top + 1);
    }
    // level k >= 1 of vector 0 and the distance to the next vector's; the plain policy over it, in place
    fr_mem_t* level(int k, size_t slot) const { return k == top ? kept + slot * count : cv + off[k]; }
    size_t stride(int k) const { return k == top ? 1 : total; }
    fr_span_plain_t in_place(int k, size_t slot) const { return {level(k, slot), level(k, slot), stride(k), stride(k), 0}; }
    dim3 grid(int k) const { return dim3((unsigned)((sizes[k + 1] + 255) / 256), (unsigned)count); }

    template <class S>
    void up_level(int k, const S& walk, size_t slot) {
        hipLaunchKernelGGL((fr_horner_up_kernel<S>), grid(k), dim3(256), 0, c.stream, walk, sizes[k], (const fr_mem_t*)(head + k), level(k + 1, slot), sizes[k + 1], stride(k + 1));
    }
    template <class S>
    void down_level(int k, const S& walk, fr_mem_t* first) {
        hipLaunchKernelGGL((fr_horner_down_kernel<S>), grid(k), dim3(256), 0, c.stream, walk, sizes[k], (const fr_mem_t*)(head + k), (const fr_mem_t*)level(k + 1, 0),
                           sizes[k + 1], stride(k + 1), first);
    }
    template <class S>
    void up(const S& walk, size_t slot = 0) {
        if (g.route == 1) {
            hipLaunchKernelGGL((fr_horner2_up_kernel<S>), dim3((unsigned)g.blocks, (unsigned)count), dim3(HORNER2_B), 0, c.stream, walk, n, m, (const fr_mem_t*)head, hs, bv,
                               g.C, g.blocks * HORNER2_B, g.blocks);
            return;
        }
        up_level(0, walk, slot);
        for (int k = 1; k < top; k++) up_level(k, in_place(k, slot), slot);
    }
    // behind up(walk, 0): every level's chunk values become its suffix sums in place (the one value of the top level is its own), then level 0
    // through the policy; first[y] = h_0 of vector y
    template <class S>
    void down(const S& walk, fr_mem_t* first) {
        if (g.route == 1) {
            hipLaunchKernelGGL((fr_horner2_down_kernel<S>), dim3((unsigned)g.blocks, (unsigned)count), dim3(HORNER2_B), 0, c.stream, walk, n, m, (const fr_mem_t*)head,
                               (const fr_mem_t*)hs, (const fr_mem_t*)bv, g.C, g.blocks * HORNER2_B, g.blocks, first);
            return;
        }
        down_above();
        down_level(0, walk, first);
    }
    void down_above() {  // route 0, the levels above level 0 alone
        for (int k = top - 1; k >= 1; k--) down_level(k, in_place(k, 0), nullptr);
    }
};

extern "C" {

// ---- prover-round polynomial kernels (poly.hip.h) ---------------------------------------------------
static RustError fr_vec_op_impl(int op, void* out, const void* a, const void* b, const void* c3, const void* scalar, size_t n, int on_device, size_t count,
                                size_t stride) {
    API_BEGIN_DEV(device_for(a, (on_device && n) ? 1 : 0))
    if (op < 0 || op > FR_OP_RSUB_SCALAR) throw hip_failure{hipErrorInvalidValue, "fr_vec_op: unknown op", __LINE__};
    check_strided(n, count, stride, on_device);
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

// quotient and remainder of `count` vectors (`stride` elements apart, like their quotients) by X - z: d_out[i - 1] = h_i, d_first[y] = h_0;
// `d_out` may be null (only h_0 wanted)
static void fr_divide_by_linear_run(lane_t& c, const fr_mem_t* d_in, size_t n, const fr_mem_t& z, fr_mem_t* d_out, fr_mem_t* d_first, size_t count, size_t stride) {
    const auto value_from = [&](const fr_mem_t* src, size_t src_stride) {
        for (size_t y = 0; y < count; y++) HIP_TRY(hipMemcpyAsync(d_first + y, src + y * src_stride, sizeof(fr_mem_t), hipMemcpyDeviceToDevice, c.stream));
    };
    if (n == 1) {
        // a lone coefficient is its own h_0: one level and no chunk values, where a sweep always has two
        c.poly[4].ensure(sizeof(fr_mem_t) * 3);
        hipLaunchKernelGGL(fr_horner_multipliers_kernel, dim3(1), dim3(1), 0, c.stream, z, c.poly[4].as<fr_mem_t>(), 1);
        value_from(d_in, stride);
    } else {
        const fr_horner_geometry_t g = fr_horner_geometry(n, d_out != nullptr);
        const fr_span_plain_t walk{d_in, d_out, stride, stride, 1};
        fr_horner_sweep sweep(c, g, n, z, count, g.route ? 0 : count);
        sweep.up(walk);
        if (d_out) {
            sweep.down(walk, d_first);
        } else {
            // only h_0: the value of the top level.  The levels above level 0 still take their way down, as they always have here (the fold's
            // value-only path never did): launches nobody reads, kept so that this call's launch sequence stays what it was
            sweep.down_above();
            value_from(sweep.kept, 1);
        }
    }
    HIP_TRY(hipGetLastError());
}

static RustError fr_divide_by_linear_impl(void* quotient, void* remainder, const void* poly, size_t n, const void* point, int on_device, size_t count,
                                          size_t stride) {
    API_BEGIN_DEV(device_for(poly, (on_device && n) ? 1 : 0))
    if (!point || (n && !poly)) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_linear: missing operand", __LINE__};
    check_strided(n, count, stride, on_device);
    if (on_device && n > 1) {  // header: different workgroups own adjacent coefficient ranges - an in-place division would race
        const size_t span = (count - 1) * stride + n;
        if (fr_spans_overlap(quotient, span, poly, span)) throw hip_failure{hipErrorInvalidValue, "fr_divide_by_linear: quotient overlaps poly (device operands must not alias)", __LINE__};
    }
    if (n == 0) {
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t) * count);
    } else {
        const fr_mem_t z = fr_mem_from_host(point);
        const fr_mem_t* din = fr_stage_in(c, 0, poly, n, on_device);
        fr_mem_t* dq = (quotient && n > 1) ? fr_stage_out(c, 1, quotient, n - 1, on_device) : nullptr;
        c.poly[2].ensure(sizeof(fr_mem_t) * count);
        fr_mem_t* drem = c.poly[2].as<fr_mem_t>();
        fr_divide_by_linear_run(c, din, n, z, dq, drem, count, stride);
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

RustError snarkvm_hip_fr_lagrange_coefficients(void* out, uint32_t lg, const void* tau, int on_device) {
    API_BEGIN_DEV(device_for(out, (on_device && out) ? 1 : 0))
    if (lg > 30) throw hip_failure{hipErrorInvalidValue, "fr_lagrange_coefficients: lg_domain_size > 30", __LINE__};
    if (!out || !tau) throw hip_failure{hipErrorInvalidValue, "fr_lagrange_coefficients: missing operand", __LINE__};
    const size_t n = (size_t)1 << lg;
    // scalar set-up with the same arithmetic compiled for the host (domain.rs:118-147, 258-264)
    const fr_t omega = fr_domain_generator(lg);
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
    check_strided(len, count, stride, on_device);
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
// a non-empty operand of a combination: the caller's index, its length, whether it IS the output (fr_lincomb alone allows that)
struct fr_lincomb_entry_t {
    size_t k, len;
    bool aliased;
};
// One launch table for fr_lincomb_plan and fr_open_plan: the sum so far first - `acc` (n_acc elements, coefficient one, src -1), nullptr in a
// launch that has none to take in - then the entries from `at` up to `end`, as many as the table holds; `at` moves on.
static fr_lincomb_launch_t fr_lincomb_table(const void* acc, size_t n_acc, const std::vector<fr_lincomb_entry_t>& live, size_t& at, size_t end, const void* const* polys,
                                            const void* coeffs) {
    fr_lincomb_launch_t L{};
    int m = 0;
    if (acc) {
        L.t.p[0] = (const fr_mem_t*)acc, L.t.len[0] = n_acc, L.src[0] = -1;
        for (int l = 0; l < 9; l++) L.t.c[0][l] = FrP::ONE[l];
        m = 1;
    }
    for (; m < FR_LINCOMB_CHUNK && at < end; m++, at++) {
        const fr_lincomb_entry_t& e = live[at];
        const fr_mem_t c_mem = fr_mem_from_host((const uint8_t*)coeffs + sizeof(fr_mem_t) * e.k);
        const fr_t c = fr_t::load(&c_mem).from_mem_mont();
        L.t.p[m] = (const fr_mem_t*)polys[e.k], L.t.len[m] = e.len, L.src[m] = (int64_t)e.k;
        for (int l = 0; l < 9; l++) L.t.c[m][l] = c.v[l];
    }
    L.t.count = m;
    return L;
}
// nullptr, or why the call is refused (hipErrorInvalidValue).  Nothing has been touched either way.
static const char* fr_lincomb_plan(const void* out, size_t n_out, size_t count, const void* const* polys, const size_t* lens, const void* coeffs,
                                   std::vector<fr_lincomb_launch_t>& plan) {
    if (!out || (count && (!polys || !lens || !coeffs))) return "missing argument";
    using entry_t = fr_lincomb_entry_t;
    std::vector<entry_t> live;
    size_t aliased = 0;
    for (size_t k = 0; k < count; k++) {
        const size_t len = lens[k];
        if (len > n_out) return "an operand is longer than n_out";
        if (!len) continue;
        if (!polys[k]) return "null operand of non-zero length";
        // out may BE an operand (same start): a thread reads index i of every operand before it writes out[i].  Any other overlap is refused.
        if (polys[k] != out && fr_spans_overlap(out, n_out, polys[k], len)) return "out overlaps an operand";
        live.push_back({k, len, polys[k] == out});
        aliased += polys[k] == out;
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
    do plan.push_back(fr_lincomb_table(at ? out : nullptr, n_out, live, at, live.size(), polys, coeffs));  // every launch but the first: out is the sum so far
    while (at < live.size());
    return nullptr;
}
RustError snarkvm_hip_fr_lincomb(void* out, size_t n_out, size_t count, const void* const* polys, const size_t* lens, const void* coeffs, int on_device) {
    if (n_out == 0) return ok();
    std::vector<fr_lincomb_launch_t> plan;
    if (const char* why = fr_lincomb_plan(out, n_out, count, polys, lens, coeffs, plan)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_lincomb: ") + why);
    API_BEGIN_DEV(device_for(out, on_device ? 1 : 0))
    fr_mem_t* dout = (fr_mem_t*)out;
    fr_host_pack_t pack(c);
    if (on_device) {
        for (size_t k = 0; k < count; k++)
            if (lens[k]) fr_same_device(c, polys[k], "fr_lincomb: an operand lives on another device than out");
    } else {  // out and, behind it, every operand
        size_t total = n_out;
        for (size_t k = 0; k < count; k++) total += lens[k];
        pack.begin(0, total);
        dout = pack.out(out, n_out);
        std::vector<const fr_mem_t*> staged(count, nullptr);
        for (size_t k = 0; k < count; k++) staged[k] = pack.in(polys[k], lens[k]);
        for (fr_lincomb_launch_t& L : plan)
            for (int m = 0; m < L.t.count; m++) L.t.p[m] = L.src[m] < 0 ? dout : staged[(size_t)L.src[m]];
    }
    for (const fr_lincomb_launch_t& L : plan) hipLaunchKernelGGL(fr_lincomb_kernel, dim3(fr_grid(n_out)), dim3(256), 0, c.stream, dout, n_out, L.t);
    HIP_TRY(hipGetLastError());
    pack.download();
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

// ---- opening fold: a combination, its quotient by X - point and its value (poly.hip.h: fr_span_fold_t under fr_horner_sweep) -------------
// What the device call and its host replay share: validation, operand order, the split into launches and the choice of the route.
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  An empty plan: the
// combination is zero.  The LAST launch of the plan is the fused sweep, the ones before it are plain fr_lincomb_kernel launches.  With a
// quotient every launch after the first takes the quotient buffer - the sum so far - back in as its first term (src -1, coefficient one);
// without one every launch is an up sweep that stands alone, and the values of the launches are added.
static const char* fr_open_plan(const void* quotient, size_t n, size_t count, const void* const* polys, const size_t* lens, const void* coeffs, const void* point,
                                std::vector<fr_lincomb_launch_t>& plan) {
    if (!point) return "missing point";
    if (count && (!polys || !lens)) return "missing operand list";
    if (count && !coeffs) return "missing coeffs";
    using entry_t = fr_lincomb_entry_t;
    std::vector<entry_t> live;
    for (size_t k = 0; k < count; k++) {
        const size_t len = lens[k];
        if (len > n) return "an operand is longer than n";
        if (!len) continue;
        if (!polys[k]) return "null operand of non-zero length";
        // the quotient buffer is the pass's only workspace: no operand may touch it, not even start where it starts
        if (fr_spans_overlap(quotient, n, polys[k], len)) return "quotient overlaps an operand";
        live.push_back({k, len, false});
    }
    if (live.empty()) return nullptr;
    std::stable_sort(live.begin(), live.end(), [](const entry_t& a, const entry_t& b) { return a.len > b.len; });
    size_t at = 0;
    // one table: the sum so far first (every launch into a quotient buffer but the first), then the members from `at` up to `end`
    const auto table = [&](size_t end) { plan.push_back(fr_lincomb_table(at ? quotient : nullptr, n, live, at, end, polys, coeffs)); };
    // with a quotient the fused sweep takes FR_OPEN_FUSE terms at most (poly.hip.h: one), the sum of the other members among them: those go
    // through plain accumulating launches first
    const size_t lead = quotient && live.size() > (size_t)FR_OPEN_FUSE ? live.size() - (FR_OPEN_FUSE - 1) : 0;
    while (at < lead) table(lead);
    do table(live.size());  // the fused launch (it may hold the sum alone); without a quotient one table after the other
    while (at < live.size());
    return nullptr;
}
// enqueues the pass on the lane's stream: the leading accumulating launches, then one fr_horner_sweep over the fold's span policy; -> where the
// value h_0 will be (device memory, the lane's poly[4]: the sweep's kept elements, a top value per table and the result behind them)
static const fr_mem_t* fr_open_run(lane_t& c, fr_mem_t* dq, size_t n, const fr_mem_t& z, const std::vector<fr_lincomb_launch_t>& plan) {
    hipStream_t st = c.stream;
    const fr_horner_geometry_t g = fr_horner_geometry(n, dq != nullptr);
    // a list longer than one table, quotient wanted: the leading tables are plain accumulating passes into the quotient buffer
    if (dq)
        for (size_t j = 0; j + 1 < plan.size(); j++) hipLaunchKernelGGL(fr_lincomb_kernel, dim3(fr_grid(n)), dim3(256), 0, st, dq, n, plan[j].t);
    // the value alone (always route 0): by linearity one up sweep per table, the top values - kept[0 .. nl) - added in list order
    const size_t nl = dq ? 1 : plan.size(), tops = g.route ? 0 : nl;
    fr_horner_sweep sweep(c, g, n, z, 1, tops + 1);
    fr_mem_t* res = sweep.kept + tops;
    if (dq) {
        // level 0 of the way down turns the combination, parked in the quotient buffer on the way up, into the quotient
        const fr_span_fold_t walk{dq, plan.back().t};
        sweep.up(walk);
        sweep.down(walk, res);
    } else {
        for (size_t j = 0; j < nl; j++) sweep.up(fr_span_fold_t{nullptr, plan[j].t}, j);
        if (nl > 1) hipLaunchKernelGGL(fr_open_sum_kernel, dim3(1), dim3(1), 0, st, (const fr_mem_t*)sweep.kept, (uint32_t)nl, res);
    }
    HIP_TRY(hipGetLastError());
    return dq || nl > 1 ? res : sweep.kept;
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
    fr_host_pack_t pack(c);
    if (on_device) {
        for (size_t k = 0; k < count; k++)
            if (lens[k]) fr_same_device(c, polys[k], "fr_open_fold: an operand lives on another device than the quotient (or the first operand)");
    } else {  // the quotient and, behind it, every operand
        size_t total = quotient ? n : 0;
        for (size_t k = 0; k < count; k++) total += lens[k];
        pack.begin(0, total);
        if (quotient) dq = pack.out(quotient, n);
        std::vector<const fr_mem_t*> staged(count, nullptr);
        for (size_t k = 0; k < count; k++) staged[k] = pack.in(polys[k], lens[k]);
        for (fr_lincomb_launch_t& L : plan)
            for (int m = 0; m < L.t.count; m++) L.t.p[m] = L.src[m] < 0 ? dq : staged[(size_t)L.src[m]];
    }
    if (plan.empty()) {  // device quotient of the zero combination
        HIP_TRY(hipMemsetAsync(dq, 0, sizeof(fr_mem_t) * n, c.stream));
        if (remainder) memset(remainder, 0, sizeof(fr_mem_t));
    } else {
        const fr_mem_t* dres = fr_open_run(c, dq, n, fr_mem_from_host(point), plan);
        pack.download();
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
    const fr_horner_geometry_t g = fr_horner_geometry(n ? n : 1, true);
    out5[0] = (uint32_t)g.route, out5[1] = g.C, out5[2] = (uint32_t)g.blocks, out5[3] = FR_LINCOMB_CHUNK, out5[4] = FR_OPEN_FUSE;
    return 0;
}
// The same call on host memory with the CPU in the kernels' place, over a GIVEN geometry: the same plan, every launch a loop over its threads
// through the kernels' own span policies and scaffold routines (poly.hip.h), a workgroup's LDS exchanges as loops over its threads.
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
    const fr_span_fold_t walk{q, plan.back().t};
    if (route == 1) {
        const uint32_t B = HORNER2_B;
        std::vector<fr_mem_t> tab(HORNER2_TAB), hs((size_t)blocks * B), bv(blocks);  // through memory, as on the device
        for (uint32_t t = 0; t < B; t++) fr_horner2_tables_thread(m, tab.data(), C, t);
        std::vector<fr_t> v(B), sh;  // a workgroup's values, thread by thread, and what it put into LDS before the barrier
        const auto behind = [&](uint32_t s) { return sh[s]; };
        for (uint32_t b = 0; b < blocks; b++) {  // fr_horner2_up_kernel
            for (uint32_t t = 0; t < B; t++) {
                const fr_horner_span_t sp = fr_horner_span((size_t)b * B + t, C, n);
                v[t] = walk.up(m, sp.lo, sp.hi);
            }
            for (int j = 0; j < 8; j++) {
                sh = v;
                for (uint32_t t = 0; t < B; t++) v[t] = fr_horner_scan_step(tab.data(), j, t, sh[t], behind);
            }
            for (uint32_t t = 0; t < B; t++) v[t].store(&hs[(size_t)b * B + t]);
            v[0].store(&bv[b]);
        }
        for (uint32_t b = 0; b < blocks; b++) {  // fr_horner2_down_kernel
            for (uint32_t t = 0; t < B; t++) v[t] = fr_horner_carry_term(tab.data(), bv.data(), b, t, blocks);
            for (uint32_t off = B / 2; off >= 1; off >>= 1) {
                sh = v;
                for (uint32_t t = 0; t < B; t++) v[t] = fr_horner_carry_step(off, t, sh[t], behind);
            }
            const fr_t carry = v[0];
            for (uint32_t t = 0; t < B; t++) {
                const fr_horner_span_t sp = fr_horner_span((size_t)b * B + t, C, n);
                if (sp.empty()) continue;
                const fr_t h = walk.down(m, fr_horner_thread_carry(tab.data(), hs.data(), b, t, carry), sp.lo, sp.hi);
                if (sp.lo == 0) h.store(&res);
            }
        }
    } else {
        const std::vector<size_t> sizes = fr_horner_levels(n, C);
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
        std::vector<std::vector<fr_mem_t>> cv(top + 1);  // level k >= 1: the chunk values of level k - 1, cv[top] the single top value
        for (int k = 1; k <= top; k++) cv[k].resize(sizes[k]);
        const auto in_place = [&](int k) { return fr_span_plain_t{cv[k].data(), cv[k].data(), 0, 0, 0}; };
        // one level of a sweep: the threads of fr_horner_up_kernel / fr_horner_down_kernel
        const auto up_level = [&](int k, const auto& w) {
            for (size_t t = 0; t < sizes[k + 1]; t++) {
                const fr_horner_span_t sp = fr_horner_span(t, C, sizes[k]);
                w.up(mult[k], sp.lo, sp.hi).store(&cv[k + 1][t]);
            }
        };
        const auto down_level = [&](int k, const auto& w) {
            for (size_t t = 0; t < sizes[k + 1]; t++) {
                const fr_horner_span_t sp = fr_horner_span(t, C, sizes[k]);
                const fr_t h = w.down(mult[k], fr_horner_chunk_carry(cv[k + 1].data(), t, sizes[k + 1]), sp.lo, sp.hi);
                if (k == 0 && t == 0) h.store(&res);
            }
        };
        const auto up = [&](const fr_span_fold_t& w) {
            up_level(0, w);
            for (int k = 1; k < top; k++) up_level(k, in_place(k));
            return fr_t::load(&cv[top][0]);
        };
        if (!q) {
            fr_t s = fr_t::zero();
            for (size_t j = 0; j < plan.size(); j++) {
                const fr_t v = up(fr_span_fold_t{nullptr, plan[j].t});
                if (plan.size() == 1)
                    v.store(&res);
                else
                    s = s + v;
            }
            if (plan.size() > 1) s.store(&res);
        } else {
            up(walk);
            for (int k = top - 1; k >= 1; k--) down_level(k, in_place(k));
            down_level(0, walk);
        }
    }
    if (remainder) memcpy(remainder, &res, sizeof res);
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

// ---- evaluation of many polynomials, each at its point (poly.hip.h: fr_evaluate_kernel) -----------------------------------------
static constexpr size_t FR_EVALUATE_MAX_LEN = (size_t)1 << 29;
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  n_max: the longest member.
static const char* fr_evaluate_check(const void* results, size_t count, const void* const* polys, const size_t* lens, const void* points, size_t& n_max) {
    if (!results || !polys || !lens || !points) return "missing argument";
    if (count > 65535) return "more than 65535 members";
    n_max = 0;
    for (size_t k = 0; k < count; k++) {
        if (lens[k] > FR_EVALUATE_MAX_LEN) return "a member is longer than 2^29";
        if (lens[k] && !polys[k]) return "null member of non-zero length";
        n_max = std::max(n_max, lens[k]);
    }
    return nullptr;
}
// What the device call and its host replay share: the distinct points (recognised by their bytes) with their powers for T threads per member, the
// members grouped by point (stable: the caller's order inside a group) and cut into launches of at most FR_EVALUATE_MEMBERS members and
// FR_EVALUATE_POINTS points.  The point is converted to the true internal form HERE, once per distinct point (poly.hip.h: the pass's one fix-up).
static std::vector<fr_evaluate_t> fr_evaluate_plan(size_t count, const void* const* polys, const size_t* lens, const void* points, size_t T) {
    std::vector<std::array<uint8_t, sizeof(fr_mem_t)>> distinct;
    std::vector<std::vector<size_t>> members;  // per distinct point, in the order of first appearance
    {
        std::map<std::array<uint8_t, sizeof(fr_mem_t)>, size_t> seen;
        for (size_t k = 0; k < count; k++) {
            std::array<uint8_t, sizeof(fr_mem_t)> key;
            memcpy(key.data(), (const uint8_t*)points + sizeof(fr_mem_t) * k, sizeof(fr_mem_t));
            const auto it = seen.emplace(key, distinct.size());
            if (it.second) distinct.push_back(key), members.emplace_back();
            members[it.first->second].push_back(k);
        }
    }
    std::vector<fr_evaluate_t> plan;
    int np = FR_EVALUATE_POINTS;  // points of the last table; a full one opens the next
    for (size_t q = 0; q < distinct.size(); q++) {
        fr_evaluate_point_t P;
        {
            const fr_mem_t z_mem = fr_mem_from_host(distinct[q].data());
            fr_t s = fr_t::load(&z_mem).from_mem_mont();
            const fr_t Z = s.pow_u64(T);
            for (int i = 0; i < FR_EVALUATE_BITS; i++, s = s.sqr())
                for (int l = 0; l < 9; l++) P.pw[i][l] = s.v[l];
            fr_t Zg = fr_t::one();
            for (int g = 0; g <= FR_EVALUATE_G; g++, Zg = Zg * Z)
                for (int l = 0; l < 9; l++) P.Z[g][l] = Zg.v[l];
        }
        bool placed = false;  // is P in the last table of the plan?
        for (size_t k : members[q]) {
            if (plan.empty() || plan.back().count == (uint32_t)FR_EVALUATE_MEMBERS || (!placed && np == FR_EVALUATE_POINTS)) plan.emplace_back(), np = 0, placed = false;
            fr_evaluate_t& t = plan.back();
            if (!placed) t.pt[np++] = P, t.points = (uint32_t)np, placed = true;
            const uint32_t m = t.count++;
            t.p[m] = (const fr_mem_t*)polys[k], t.len[m] = (uint32_t)lens[k], t.point[m] = (uint16_t)(np - 1), t.row[m] = (uint16_t)k;
        }
    }
    return plan;
}
RustError snarkvm_hip_fr_evaluate(void* results, size_t count, const void* const* polys, const size_t* lens, const void* points, int on_device) {
    if (count == 0) return ok();
    size_t n_max = 0;
    if (const char* why = fr_evaluate_check(results, count, polys, lens, points, n_max)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_evaluate: ") + why);
    if (n_max == 0) {
        memset(results, 0, sizeof(fr_mem_t) * count);
        return ok();
    }
    const void* first = nullptr;
    for (size_t k = 0; k < count && !first; k++)
        if (lens[k]) first = polys[k];
    API_BEGIN_DEV(device_for(first, on_device ? 1 : 0))
    const unsigned blocks = fr_reduce_blocks(n_max);
    std::vector<fr_evaluate_t> plan = fr_evaluate_plan(count, polys, lens, points, (size_t)blocks * FR_REDUCE_B);
    fr_host_pack_t pack(c);
    if (on_device) {
        for (size_t k = 0; k < count; k++)
            if (lens[k]) fr_same_device(c, polys[k], "fr_evaluate: members live on different devices");
    } else {  // every distinct buffer once, at the longest length it is read with
        std::map<const void*, size_t> longest;
        for (size_t k = 0; k < count; k++)
            if (lens[k]) longest[polys[k]] = std::max(longest[polys[k]], lens[k]);
        size_t total = 0;
        for (const auto& e : longest) total += e.second;
        pack.begin(0, total);
        std::map<const void*, const fr_mem_t*> staged;
        for (const auto& e : longest) staged[e.first] = pack.in(e.first, e.second);
        for (fr_evaluate_t& t : plan)
            for (uint32_t m = 0; m < t.count; m++)
                if (t.len[m]) t.p[m] = staged[t.p[m]];
    }
    // workspace: count x blocks partials, then the count results, then the table of powers of one launch (every launch fills it anew: the stream is in order)
    const size_t tab_n = fr_evaluate_table_size(FR_REDUCE_B, blocks);
    c.poly[4].ensure(sizeof(fr_mem_t) * (count * ((size_t)blocks + 1) + tab_n));
    fr_mem_t* parts = c.poly[4].as<fr_mem_t>();
    fr_mem_t* dres = parts + count * (size_t)blocks;
    fr_mem_t* tab = dres + count;
    for (const fr_evaluate_t& t : plan) {
        if (tab_n) hipLaunchKernelGGL(fr_evaluate_powers_kernel, dim3((FR_REDUCE_B + blocks + FR_REDUCE_B - 1) / FR_REDUCE_B, t.points), dim3(FR_REDUCE_B), 0, c.stream, tab, (uint32_t)FR_REDUCE_B, (uint32_t)blocks, t);
        hipLaunchKernelGGL(fr_evaluate_kernel, dim3(blocks, t.count), dim3(FR_REDUCE_B), 0, c.stream, parts, (const fr_mem_t*)tab, t);
    }
    hipLaunchKernelGGL(fr_reduce_final_kernel, dim3(1, (unsigned)count), dim3(FR_REDUCE_B), 0, c.stream, (int)FR_REDUCE_SUM, (const fr_mem_t*)parts, (size_t)blocks, dres);
    HIP_TRY(hipGetLastError());
    // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the values are there on return
    c.host_result(results, dres, sizeof(fr_mem_t) * count, on_device != 0);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernels' place, over a GIVEN geometry (blocks workgroups of `threads` threads, threads = 64, 128
// or 256, blocks x threads <= 2^FR_EVALUATE_BITS): the same plan, per launch the table of powers entry by entry through fr_evaluate_table_entry, every thread
// through fr_evaluate_thread, the workgroup's tree level by level, thread 0's fr_evaluate_block, the partials through memory, the last launch as in
// snarkvm_hip_selftest_fr_reduce.  0, or -1 when the arguments or the
// geometry are refused.
int snarkvm_hip_selftest_fr_evaluate(void* results, size_t count, const void* const* polys, const size_t* lens, const void* points, uint32_t blocks, uint32_t threads) {
    if (!fr_reduce_geometry_ok(blocks, threads) || (uint64_t)blocks * threads > (uint64_t)1 << FR_EVALUATE_BITS) return -1;
    if (count == 0) return 0;
    size_t n_max = 0;
    if (fr_evaluate_check(results, count, polys, lens, points, n_max)) return -1;
    const auto add = [](const fr_t& x, const fr_t& y) { return x + y; };
    std::vector<fr_mem_t> parts(count * (size_t)blocks), tab(fr_evaluate_table_size(threads, blocks));
    for (const fr_evaluate_t& t : fr_evaluate_plan(count, polys, lens, points, (size_t)blocks * threads)) {
        if (!tab.empty())  // fr_evaluate_powers_kernel
            for (uint32_t q = 0; q < t.points; q++)
                for (uint32_t e = 0; e < threads + blocks; e++) fr_evaluate_table_entry(t.pt[q], e, threads).store(&tab[(size_t)q * (threads + blocks) + e]);
        for (uint32_t y = 0; y < t.count; y++)
            for (uint32_t x = 0; x < blocks; x++) {
                std::vector<fr_t> vals(threads);
                for (uint32_t tid = 0; tid < threads; tid++) vals[tid] = fr_evaluate_thread(t, tab.data(), y, x, tid, threads, blocks);
                fr_evaluate_block(t, tab.data(), y, x, threads, blocks, fr_block_tree_host(vals, fr_t::zero(), add)).store(&parts[(size_t)t.row[y] * blocks + x]);
            }
    }
    fr_mem_t* res = (fr_mem_t*)results;
    for (size_t k = 0; k < count; k++) {
        std::vector<fr_t> vals(FR_REDUCE_B);
        for (uint32_t tid = 0; tid < (uint32_t)FR_REDUCE_B; tid++) vals[tid] = fr_reduce_thread<FR_REDUCE_SUM>(parts.data() + k * (size_t)blocks, nullptr, blocks, tid, FR_REDUCE_B);
        fr_mem_t r;
        fr_reduce_finish(FR_REDUCE_SUM, fr_block_tree_host(vals, fr_t::zero(), add)).store(&r);
        memcpy(&res[k], &r, sizeof r);
    }
    return 0;
}
// what snarkvm_hip_fr_evaluate launches for a longest member of n_max: out8 = {workgroups per member, threads per workgroup, the cap on workgroups,
// coefficients per Montgomery reduction, members per launch, distinct points per launch, how z^t is formed (FR_EVALUATE_POW), the bits of a thread index}
int snarkvm_hip_selftest_fr_evaluate_geometry(size_t n_max, uint32_t* out) {
    if (!out) return -1;
    out[0] = fr_reduce_blocks(n_max), out[1] = FR_REDUCE_B, out[2] = FR_REDUCE_BLOCKS_MAX, out[3] = FR_EVALUATE_G;
    out[4] = FR_EVALUATE_MEMBERS, out[5] = FR_EVALUATE_POINTS, out[6] = FR_EVALUATE_POW, out[7] = FR_EVALUATE_BITS;
    return 0;
}

}  // extern "C"
