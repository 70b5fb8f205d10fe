// api_varuna.hip - the Varuna entry points of the C ABI (poly.hip.h): round 3's selector fold, round 1's witness and assignment evaluations, round 2's rowcheck
// fold, the sparse matrix-vector product over a registered matrix, round 4's matrix-sumcheck evaluations over a registered arithmetization, and
// the circuit index (arithmetize, register_csr), each with its host twin and geometry hook.  The frame they share: fr_call.hip.h.
#include "fr_call.hip.h"

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

// a registered matrix: per device ONE block holding vals | segment table | fix-up table | col_idx
struct snarkvm_hip_fr_matrix : fr_replicas_t<uint8_t> {
    size_t rows = 0, cols = 0, nnz = 0, nseg = 0, nfix = 0, nparts = 0;
    uint32_t seg = 0, width = 0;
    size_t off_segs = 0, off_fix = 0, off_col = 0, bytes = 0;
    // the parts of one device's block `b`
    const fr_mem_t* vals(const uint8_t* b) const { return (const fr_mem_t*)b; }
    const fr_spmv_seg_t* segs(const uint8_t* b) const { return (const fr_spmv_seg_t*)(b + off_segs); }
    const fr_spmv_fix_t* fix(const uint8_t* b) const { return (const fr_spmv_fix_t*)(b + off_fix); }
    const uint32_t* col(const uint8_t* b) const { return (const uint32_t*)(b + off_col); }
};
// a registered arithmetization: per device ONE block holding row | col | row_col_val, k elements each
struct snarkvm_hip_fr_arith : fr_replicas_t<fr_mem_t> {
    size_t k = 0;
};
template <int W>
static void fr_spmv_launch(lane_t& c, const snarkvm_hip_fr_matrix& h, const uint8_t* blk, const fr_mem_t* dx, size_t stride_x, fr_mem_t* dy, size_t stride_y, size_t n_out,
                           size_t count, fr_mem_t* parts) {
    const size_t per_block = FR_SPMV_B / W;
    if (h.nseg)
        hipLaunchKernelGGL(fr_spmv_seg_kernel<W>, dim3((unsigned)((h.nseg + per_block - 1) / per_block), (unsigned)count), dim3(FR_SPMV_B), 0, c.stream, h.segs(blk), h.nseg,
                           h.vals(blk), h.col(blk), dx, stride_x, dy, stride_y, parts, h.nparts);
    const size_t groups = h.nfix + (n_out - h.rows);
    if (groups)
        hipLaunchKernelGGL(fr_spmv_fix_kernel<W>, dim3((unsigned)((groups + per_block - 1) / per_block), (unsigned)count), dim3(FR_SPMV_B), 0, c.stream, h.fix(blk), h.nfix,
                           (const fr_mem_t*)parts, h.nparts, dy, stride_y, h.rows, n_out);
}
// the rowcheck's instantiation for what a plan wants (FR_ROWCHECK_FOLD, _CHECK or both): f(std::integral_constant<int, mode>)
template <class F>
static auto fr_rowcheck_dispatch(int mode, F f) {
    if (mode == FR_ROWCHECK_FOLD) return f(std::integral_constant<int, FR_ROWCHECK_FOLD>{});
    if (mode == FR_ROWCHECK_CHECK) return f(std::integral_constant<int, FR_ROWCHECK_CHECK>{});
    return f(std::integral_constant<int, FR_ROWCHECK_FOLD | FR_ROWCHECK_CHECK>{});
}

extern "C" {

// ---- selector fold: Varuna round 3 (poly.hip.h: fr_selector_fold_kernel) ---------------------------------------------------
// What the device call and its host replay share: validation, the member tables and the split into launches.  src[m]: the caller's index
// of table entry m (its pointers are bound later: to the caller's memory, or to the staged copies).
static constexpr size_t FR_SELECTOR_LEN_MAX =(size_t)1 << 29, FR_SELECTOR_TARGET_MAX = (size_t)1 << 28;
struct fr_selector_launch_t {
    fr_selector_t t;
    size_t src[FR_SELECTOR_CHUNK];
};
struct fr_selector_plan_t {
    std::vector<fr_selector_launch_t> launches;
    bool want_h = false, want_xg = false, want_sums = false;
    uint32_t h_len = 0, N = 0, span = 0, threads = 0;  // span: the indices of xg the fold itself writes (the tile kernel the rest)
};
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  A plan without
// launches: nothing is wanted.
static const char* fr_selector_plan(const void* h_out, size_t h_len, const void* xg_out, size_t target_size, const void* sums, size_t count, const void* const* polys,
                                    const size_t* lens, const size_t* src_sizes, const void* multipliers, fr_selector_plan_t& plan) {
    if (count > 65535) return "more than 65535 members";
    if (count && (!polys || !lens || !src_sizes || !multipliers)) return "missing argument";
    if (h_out && h_len > FR_SELECTOR_LEN_MAX) return "h_len above 2^29";
    if (xg_out && (target_size == 0 || target_size > FR_SELECTOR_TARGET_MAX)) return "target_size is 0 or above 2^28";
    size_t need = 0, period = 1;
    for (size_t k = 0; k < count; k++) {
        const size_t n = src_sizes[k], L = lens[k];
        if (!n) return "an empty source domain";
        if (L > FR_SELECTOR_LEN_MAX) return "a member longer than 2^29";
        if (L && !polys[k]) return "null member of non-zero length";
        if (xg_out && target_size % n) return "a source domain does not divide target_size";
        if (L > n && L - n > need) need = L - n;
        if (xg_out && L) period = period / fr_gcd(period, n) * n;  // every n_k divides target_size: so does the period
    }
    if (h_out && h_len < need) return "h_len is shorter than the longest quotient";
    {  // no output may overlap an operand or another output
        std::vector<fr_range_t> rs;
        if (h_out && h_len) rs.push_back({(const uint8_t*)h_out, sizeof(fr_mem_t) * h_len, true});
        if (xg_out) rs.push_back({(const uint8_t*)xg_out, sizeof(fr_mem_t) * target_size, true});
        if (sums && count) rs.push_back({(const uint8_t*)sums, sizeof(fr_mem_t) * count, true});
        for (size_t k = 0; k < count; k++)
            if (lens[k]) rs.push_back({(const uint8_t*)polys[k], sizeof(fr_mem_t) * lens[k], false});
        if (fr_output_overlaps(std::move(rs))) return "an output overlaps an operand or another output";
    }
    plan.want_h = h_out && h_len, plan.want_xg = xg_out != nullptr, plan.want_sums = sums && count;
    if (!plan.want_h && !plan.want_xg && !plan.want_sums) return nullptr;
    plan.h_len = plan.want_h ? (uint32_t)h_len : 0;
    plan.N = plan.want_xg ? (uint32_t)target_size : 0;
    plan.span = plan.want_xg ? (FR_SELECTOR_TILE ? (uint32_t)period : plan.N) : 0;
    plan.threads = plan.h_len > plan.span ? plan.h_len : plan.span;
    if (!plan.threads) plan.threads = 1;
    std::vector<size_t> live;  // an empty member contributes nothing: it stays only where its sum (zero) is to be written
    for (size_t k = 0; k < count; k++)
        if (lens[k] || plan.want_sums) live.push_back(k);
    size_t at = 0;
    do {  // no member at all: one launch that writes the zeros
        fr_selector_launch_t L{};
        int m = 0;
        L.t.accumulate = at != 0;
        for (; m < FR_SELECTOR_CHUNK && at < live.size(); m++, at++) {
            const size_t k = live[at];
            const fr_mem_t mu_mem = fr_mem_from_host((const uint8_t*)multipliers + sizeof(fr_mem_t) * k);
            const fr_t mu = fr_t::load(&mu_mem).from_mem_mont(), ns = fr_from_u64((uint64_t)src_sizes[k]);
            L.src[m] = k;
            L.t.len[m] = (uint32_t)lens[k];
            L.t.n[m] = src_sizes[k] > ((size_t)1 << 30) ? (1u << 30) : (uint32_t)src_sizes[k];
            for (int l = 0; l < 9; l++) L.t.mu[m][l] = mu.v[l], L.t.ns[m][l] = ns.v[l];
        }
        L.t.count = m;
        plan.launches.push_back(L);
    } while (at < live.size());
    return nullptr;
}
// pointers of the tables: member k at polys[k], its sum at sums + k (nullptr: no sums)
static void fr_selector_bind(fr_selector_plan_t& plan, const fr_mem_t* const* polys, fr_mem_t* sums) {
    for (fr_selector_launch_t& L : plan.launches)
        for (int m = 0; m < L.t.count; m++) L.t.p[m] = polys[L.src[m]], L.t.sum[m] = sums ? sums + L.src[m] : nullptr;
}
RustError snarkvm_hip_fr_selector_fold(void* h_out, size_t h_len, void* xg_out, size_t target_size, void* sums, size_t count, const void* const* polys,
                                       const size_t* lens, const size_t* src_sizes, const void* multipliers, int on_device) {
    fr_selector_plan_t plan;
    if (const char* why = fr_selector_plan(h_out, h_len, xg_out, target_size, sums, count, polys, lens, src_sizes, multipliers, plan))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_selector_fold: ") + why);
    if (plan.launches.empty()) return ok();
    const void* first = plan.want_h ? h_out : (plan.want_xg ? xg_out : sums);
    API_BEGIN_DEV(device_for(first, on_device ? 1 : 0))
    fr_mem_t *dh = plan.want_h ? (fr_mem_t*)h_out : nullptr, *dxg = plan.want_xg ? (fr_mem_t*)xg_out : nullptr, *dsums = plan.want_sums ? (fr_mem_t*)sums : nullptr;
    std::vector<const fr_mem_t*> members(count, nullptr);
    fr_host_pack_t pack(c);
    if (on_device) {
        const char* why = "fr_selector_fold: the outputs and members live on different devices";
        fr_same_device(c, dh, why), fr_same_device(c, dxg, why), fr_same_device(c, dsums, why);
        for (size_t k = 0; k < count; k++) {
            if (lens[k]) fr_same_device(c, polys[k], why);
            members[k] = (const fr_mem_t*)polys[k];
        }
    } else {  // the outputs and, behind them, every member
        size_t total = (size_t)plan.h_len + plan.N + (plan.want_sums ? count : 0);
        for (size_t k = 0; k < count; k++) total += lens[k];
        pack.begin(0, total);
        if (plan.want_h) dh = pack.out(h_out, plan.h_len);
        if (plan.want_xg) dxg = pack.out(xg_out, plan.N);
        if (plan.want_sums) dsums = pack.out(sums, count);
        for (size_t k = 0; k < count; k++) members[k] = pack.in(polys[k], lens[k]);
    }
    fr_selector_bind(plan, members.data(), dsums);
    for (const fr_selector_launch_t& L : plan.launches)
        hipLaunchKernelGGL(fr_selector_fold_kernel, dim3(fr_grid(plan.threads)), dim3(256), 0, c.stream, dh, plan.h_len, dxg, plan.span, plan.threads, L.t);
    if (plan.span < plan.N) hipLaunchKernelGGL(fr_tile_kernel, dim3(fr_grid(plan.N - plan.span)), dim3(256), 0, c.stream, dxg, plan.span, plan.N);
    HIP_TRY(hipGetLastError());
    pack.download();
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernels' place: the same plan, every launch a loop over i through the kernel's own
// per-index routine, then the tiling.  0, or -1 when the plan refuses the arguments.
int snarkvm_hip_selftest_fr_selector_fold(void* h_out, size_t h_len, void* xg_out, size_t target_size, void* sums, size_t count, const void* const* polys,
                                          const size_t* lens, const size_t* src_sizes, const void* multipliers) {
    fr_selector_plan_t plan;
    if (fr_selector_plan(h_out, h_len, xg_out, target_size, sums, count, polys, lens, src_sizes, multipliers, plan)) return -1;
    if (plan.launches.empty()) return 0;
    fr_mem_t *h = plan.want_h ? (fr_mem_t*)h_out : nullptr, *xg = plan.want_xg ? (fr_mem_t*)xg_out : nullptr;
    fr_selector_bind(plan, (const fr_mem_t* const*)polys, plan.want_sums ? (fr_mem_t*)sums : nullptr);
    for (const fr_selector_launch_t& L : plan.launches)
        for (uint32_t i = 0; i < plan.threads; i++) fr_selector_at(L.t, h, plan.h_len, xg, plan.span, i);
    for (uint32_t i = plan.span; i < plan.N; i++) fr_tile_at(xg, plan.span, i);
    return 0;
}

// ---- round 1: the evaluations of w on the variable domain (poly.hip.h: fr_witness_evals_kernel) ------------------------------------------
static constexpr size_t FR_ROUND12_N_MAX = (size_t)1 << 28;
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.
static const char* fr_witness_check(const void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size) {
    if (input_size == 0) return "input_size is 0";
    if (n % input_size) return "input_size does not divide n";
    if (n > FR_ROUND12_N_MAX) return "n above 2^28";
    if (w_len > n - input_size) return "w is longer than n - input_size";
    if (n && (!out || !x_evals)) return "null vector of non-zero length";
    if (w_len && !w) return "null witness of non-zero length";
    if ((out != x_evals && fr_spans_overlap(out, n, x_evals, n)) || fr_spans_overlap(out, n, w, w_len)) return "out overlaps an operand (only out == x_evals is allowed)";
    return nullptr;
}
RustError snarkvm_hip_fr_witness_evals(void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size, int on_device) {
    if (const char* why = fr_witness_check(out, n, w, w_len, x_evals, input_size)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_witness_evals: ") + why);
    if (n == 0) return ok();
    API_BEGIN_DEV(device_for(out, on_device ? 1 : 0))
    if (on_device) {
        const char* why = "fr_witness_evals: the operands live on different devices";
        fr_same_device(c, x_evals, why);
        if (w_len) fr_same_device(c, w, why);
    }
    const fr_mem_t* dw = fr_stage_in(c, 0, w_len ? w : nullptr, w_len, on_device);
    const fr_mem_t* dx = fr_stage_in(c, 1, x_evals, n, on_device);
    fr_mem_t* dout = fr_stage_out(c, 3, out, n, on_device);
    hipLaunchKernelGGL(fr_witness_evals_kernel, dim3(fr_grid(n)), dim3(256), 0, c.stream, dout, (uint32_t)n, dw, (uint32_t)w_len, dx, (uint32_t)(n / input_size));
    HIP_TRY(hipGetLastError());
    fr_finish_out(c, dout, out, n, on_device);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernel's place, through the kernel's own per-index routine.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_witness_evals(void* out, size_t n, const void* w, size_t w_len, const void* x_evals, size_t input_size) {
    if (fr_witness_check(out, n, w, w_len, x_evals, input_size)) return -1;
    for (size_t k = 0; k < n; k++) fr_witness_at((fr_mem_t*)out, (const fr_mem_t*)w, (uint32_t)w_len, (const fr_mem_t*)x_evals, (uint32_t)(n / input_size), (uint32_t)k);
    return 0;
}
// Round 1 in lock step: the evaluations of z for every instance of a circuit (poly.hip.h: fr_assignment_evals_kernel); the refusals are
// fr_call.hip.h's fr_assignment_check, the host twin lives in api_selftest.hip.
RustError snarkvm_hip_fr_assignment_evals(void* out, size_t n, const void* vars, size_t num_vars, size_t input_size, size_t count, size_t stride_out, size_t stride_vars,
                                          int on_device) {
    if (const char* why = fr_assignment_check(out, n, vars, num_vars, input_size, count, stride_out, stride_vars))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_assignment_evals: ") + why);
    if (count == 0 || n == 0) return ok();
    if (count == 1) stride_out = stride_vars = 0;
    API_BEGIN_DEV(device_for(out, on_device ? 1 : 0))
    const fr_mem_t* dv = (const fr_mem_t*)vars;
    fr_mem_t* dout = (fr_mem_t*)out;
    size_t so = stride_out;
    if (on_device) {
        fr_same_device(c, vars, "fr_assignment_evals: vars lives on another device than out");
    } else {
        // host operands: the rows as they lie (members and the gaps between them), out packed member after member and downloaded member by member
        dv = fr_stage_in(c, 0, vars, (count - 1) * stride_vars + num_vars, 0);
        dout = fr_stage_out(c, 1, out, count * n, 0);
        so = n;
    }
    hipLaunchKernelGGL(fr_assignment_evals_kernel, dim3(fr_grid(n, FR_ASSIGNMENT_BLOCK), (unsigned)count), dim3(FR_ASSIGNMENT_BLOCK), 0, c.stream, dout, (uint32_t)n, dv,
                       (uint32_t)num_vars, (uint32_t)input_size, (uint32_t)(n / input_size), so, stride_vars);
    HIP_TRY(hipGetLastError());
    if (!on_device)
        for (size_t m = 0; m < count; m++) HIP_TRY(hipMemcpyAsync((fr_mem_t*)out + m * stride_out, dout + m * n, sizeof(fr_mem_t) * n, hipMemcpyDeviceToHost, c.stream));
    fr_call_done(c, on_device);
    API_END
}

// ---- round 2: the rowcheck fold (poly.hip.h: fr_rowcheck_fold_kernel) ------------------------------------------------------------------------
// What the device call and its host replay share: validation, the member tables and the split into launches.  Launch j holds the members
// first .. first + t.count - 1 of the caller's order (its pointers are bound later: to the caller's memory, or to the staged copies).
struct fr_rowcheck_launch_t {
    fr_rowcheck_t t;
    size_t first;
};
struct fr_rowcheck_plan_t {
    std::vector<fr_rowcheck_launch_t> launches;
    int mode = 0;  // FR_ROWCHECK_FOLD | FR_ROWCHECK_CHECK: what is wanted
};
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  Nothing has been touched either way.  A plan without launches:
// no kernel is needed (n == 0, or nothing is wanted).
static const char* fr_rowcheck_plan(const void* out, const uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c,
                                    const void* multipliers, fr_rowcheck_plan_t& plan) {
    if (n > FR_ROUND12_N_MAX) return "n above 2^28";
    if (count > 65535) return "more than 65535 members";
    if (count && (!a || !b || !c || (out && !multipliers))) return "missing argument";
    if (n)
        for (size_t k = 0; k < count; k++) {
            if (!a[k] || !b[k] || !c[k]) return "null member";
            if (fr_spans_overlap(out, n, a[k], n) || fr_spans_overlap(out, n, b[k], n) || fr_spans_overlap(out, n, c[k], n)) return "out overlaps a member";
        }
    plan.mode = (out ? FR_ROWCHECK_FOLD : 0) | (violations && count ? FR_ROWCHECK_CHECK : 0);
    if (!n || !plan.mode) return nullptr;
    size_t at = 0;
    do {  // no member at all: one launch that writes the zeros
        fr_rowcheck_launch_t L{};
        L.first = at, L.t.accumulate = at != 0;
        int m = 0;
        for (; m < FR_ROWCHECK_CHUNK && at < count; m++, at++) {
            if (!out) continue;
            const fr_mem_t mu_mem = fr_mem_from_host((const uint8_t*)multipliers + sizeof(fr_mem_t) * at);
            const fr_t mu = fr_t::load(&mu_mem).from_mem_mont(), mu_fix = mu.from_mem_mont(), neg = mu.neg();
            for (int l = 0; l < 9; l++) L.t.mu[m][l] = mu_fix.v[l], L.t.nmu[m][l] = neg.v[l];
        }
        L.t.count = m;
        plan.launches.push_back(L);
    } while (at < count);
    return nullptr;
}
// pointers of the tables: member k's vectors at a[k], b[k], c[k]
static void fr_rowcheck_bind(fr_rowcheck_plan_t& plan, const fr_mem_t* const* a, const fr_mem_t* const* b, const fr_mem_t* const* c) {
    for (fr_rowcheck_launch_t& L : plan.launches)
        for (int m = 0; m < L.t.count; m++) L.t.a[m] = a[L.first + m], L.t.b[m] = b[L.first + m], L.t.c[m] = c[L.first + m];
}
RustError snarkvm_hip_fr_rowcheck_fold(void* out, uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c3,
                                       const void* multipliers, int on_device) {
    fr_rowcheck_plan_t plan;
    if (const char* why = fr_rowcheck_plan(out, violations, n, count, a, b, c3, multipliers, plan)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_rowcheck_fold: ") + why);
    if (plan.launches.empty()) {
        if (violations && count) memset(violations, 0, sizeof(uint64_t) * count);  // n == 0: nothing is violated
        return ok();
    }
    API_BEGIN_DEV(device_for(out ? out : a[0], on_device ? 1 : 0))
    fr_mem_t* dout = (fr_mem_t*)out;
    std::vector<const fr_mem_t*> members[3];
    const void* const* given[3] = {a, b, c3};
    for (auto& v : members) v.assign(count, nullptr);
    fr_host_pack_t pack(c);
    if (on_device) {
        const char* why = "fr_rowcheck_fold: out and the members live on different devices";
        for (int j = 0; j < 3; j++)
            for (size_t k = 0; k < count; k++) fr_same_device(c, given[j][k], why), members[j][k] = (const fr_mem_t*)given[j][k];
    } else {  // out and, behind it, every member vector
        pack.begin(0, n * ((out ? 1 : 0) + 3 * count));
        if (out) dout = pack.out(out, n);
        for (int j = 0; j < 3; j++)
            for (size_t k = 0; k < count; k++) members[j][k] = pack.in(given[j][k], n);
    }
    fr_rowcheck_bind(plan, members[0].data(), members[1].data(), members[2].data());
    unsigned long long* dviol = nullptr;
    if (plan.mode & FR_ROWCHECK_CHECK) {  // workspace: one 64-bit counter per member
        c.poly[4].ensure(sizeof(unsigned long long) * count);
        dviol = c.poly[4].as<unsigned long long>();
        HIP_TRY(hipMemsetAsync(dviol, 0, sizeof(unsigned long long) * count, c.stream));
    }
    const dim3 grid(fr_grid(n)), block(256);
    for (const fr_rowcheck_launch_t& L : plan.launches) {
        unsigned long long* v = dviol ? dviol + L.first : nullptr;
        fr_rowcheck_dispatch(plan.mode, [&](auto M) { hipLaunchKernelGGL(fr_rowcheck_fold_kernel<decltype(M)::value>, grid, block, 0, c.stream, dout, v, (uint32_t)n, L.t); });
    }
    HIP_TRY(hipGetLastError());
    pack.download();
    // device operands inside a scope: delivered by snarkvm_hip_scope_end; host operands: the call waits below, the counts are there on return
    if (dviol) c.host_result(violations, dviol, sizeof(uint64_t) * count, on_device != 0);
    fr_call_done(c, on_device);
    API_END
}
// The same call on host memory with the CPU in the kernel's place: the same plan, every launch a loop over i through the kernel's own
// per-index routine, the bits it returns counted per member.  0, or -1 when the plan refuses the arguments.
int snarkvm_hip_selftest_fr_rowcheck_fold(void* out, uint64_t* violations, size_t n, size_t count, const void* const* a, const void* const* b, const void* const* c3,
                                          const void* multipliers) {
    fr_rowcheck_plan_t plan;
    if (fr_rowcheck_plan(out, violations, n, count, a, b, c3, multipliers, plan)) return -1;
    const bool check = violations && count;
    if (check) memset(violations, 0, sizeof(uint64_t) * count);
    if (plan.launches.empty()) return 0;
    fr_rowcheck_bind(plan, (const fr_mem_t* const*)a, (const fr_mem_t* const*)b, (const fr_mem_t* const*)c3);
    for (const fr_rowcheck_launch_t& L : plan.launches)
        for (size_t i = 0; i < n; i++) {
            uint32_t bad = fr_rowcheck_dispatch(plan.mode, [&](auto M) { return fr_rowcheck_at<decltype(M)::value>(L.t, (fr_mem_t*)out, (uint32_t)i); });
            for (int m = 0; bad; m++, bad >>= 1) violations[L.first + m] += bad & 1;
        }
    return 0;
}
// the members per launch and per Montgomery reduction the library was built with
int snarkvm_hip_selftest_fr_rowcheck_geometry(uint32_t* out2) {
    if (!out2) return -1;
    out2[0] = FR_ROWCHECK_CHUNK, out2[1] = FR_ROWCHECK_G;
    return 0;
}

// ---- sparse matrix times vector over a registered matrix (poly.hip.h: fr_spmv_seg_kernel, fr_spmv_fix_kernel) ----------------------
static constexpr size_t FR_SPMV_DIM_MAX = (size_t)1 << NTT_LG_MAX;  // rows, cols, n_out: the SRS maximum the transforms stop at
// nullptr, or why the CSR arrays are refused (hipErrorInvalidValue).  Needs no device and touches nothing: after it no index the kernels will
// ever see can point outside x (cols elements), vals or col_idx.
static const char* fr_spmv_matrix_check(size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals) {
    if (rows > FR_SPMV_DIM_MAX || cols > FR_SPMV_DIM_MAX) return "more than 2^28 rows or columns";
    if (!row_ptr) return "null row_ptr";
    if (row_ptr[0] != 0) return "row_ptr[0] != 0";
    for (size_t r = 0; r < rows; r++)
        if (row_ptr[r + 1] < row_ptr[r]) return "row_ptr decreases";
    const uint64_t nnz = row_ptr[rows];
    if (nnz > 0xFFFFFFFFull) return "more than 2^32 - 1 entries";
    if (nnz && (!col_idx || !vals)) return "null col_idx or vals of a matrix with entries";
    for (uint64_t k = 0; k < nnz; k++)
        if (col_idx[k] >= cols) return "a column index is not below cols";
    return nullptr;
}
// the work layout of a checked matrix for segments of at most `seg` entries -> number of partial-sum slots
static size_t fr_spmv_layout(size_t rows, const uint64_t* row_ptr, uint32_t seg, std::vector<fr_spmv_seg_t>& segs, std::vector<fr_spmv_fix_t>& fix) {
    size_t nparts = 0;
    for (size_t r = 0; r < rows; r++) {
        const uint64_t first = row_ptr[r], len = row_ptr[r + 1] - first;
        const uint64_t pieces = (len + seg - 1) / seg;
        if (pieces != 1) fix.push_back({(uint32_t)r, (uint32_t)nparts, (uint32_t)pieces, 0});
        for (uint64_t p = 0; p < pieces; p++) {
            const uint64_t at = p * seg;
            segs.push_back({(uint32_t)r, (uint32_t)(first + at), (uint32_t)(len - at < seg ? len - at : seg), pieces == 1 ? FR_SPMV_SOLE : (uint32_t)(nparts + p)});
        }
        if (pieces > 1) nparts += pieces;
    }
    return nparts;
}
RustError snarkvm_hip_fr_matrix_register(snarkvm_hip_fr_matrix_t** handle, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_matrix_register: null handle");
    *handle = nullptr;
    if (const char* why = fr_spmv_matrix_check(rows, cols, row_ptr, col_idx, vals)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_matrix_register: ") + why);
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_matrix> h(new snarkvm_hip_fr_matrix());
    std::vector<fr_spmv_seg_t> segs;
    std::vector<fr_spmv_fix_t> fix;
    h->rows = rows, h->cols = cols, h->nnz = (size_t)row_ptr[rows], h->seg = FR_SPMV_SEG;
    h->nparts = fr_spmv_layout(rows, row_ptr, h->seg, segs, fix);
    h->nseg = segs.size(), h->nfix = fix.size();
    h->width = fr_spmv_width(h->nnz, h->nseg);
    h->off_segs = sizeof(fr_mem_t) * h->nnz;
    h->off_fix = h->off_segs + sizeof(fr_spmv_seg_t) * h->nseg;
    h->off_col = h->off_fix + sizeof(fr_spmv_fix_t) * h->nfix;
    h->bytes = h->off_col + sizeof(uint32_t) * h->nnz;
    h->fill_all(h->bytes, [&](lane_t& c, uint8_t* d) {  // every device uploads its own replica
        if (h->nnz) HIP_TRY(hipMemcpyAsync(d, vals, sizeof(fr_mem_t) * h->nnz, hipMemcpyHostToDevice, c.stream));
        if (h->nseg) HIP_TRY(hipMemcpyAsync(d + h->off_segs, segs.data(), sizeof(fr_spmv_seg_t) * h->nseg, hipMemcpyHostToDevice, c.stream));
        if (h->nfix) HIP_TRY(hipMemcpyAsync(d + h->off_fix, fix.data(), sizeof(fr_spmv_fix_t) * h->nfix, hipMemcpyHostToDevice, c.stream));
        if (h->nnz) HIP_TRY(hipMemcpyAsync(d + h->off_col, col_idx, sizeof(uint32_t) * h->nnz, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
    *handle = h.release();
    API_CATCH
}
void snarkvm_hip_fr_matrix_free(snarkvm_hip_fr_matrix_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}
// nullptr, or why the product is refused (hipErrorInvalidValue); needs no device
static const char* fr_spmv_check(const void* y, size_t n_out, const snarkvm_hip_fr_matrix* h, const void* x, size_t count, size_t stride_x, size_t stride_y, int on_device) {
    if (!h) return "null handle";
    if (n_out < h->rows) return "n_out is less than the number of rows";
    if (n_out > FR_SPMV_DIM_MAX) return "n_out > 2^28";
    if (count > 65535) return "more than 65535 batch members";
    if (count > 1 && ((stride_x && stride_x < h->cols) || stride_y < n_out)) return "a stride is shorter than its vector";
    // count < 2^16 members of at most 2^40 elements apart: no span below can wrap, in elements or in bytes
    if (count > 1 && (stride_x > ((size_t)1 << 40) || stride_y > ((size_t)1 << 40))) return "a stride of more than 2^40 elements";
    if (!y || (!x && h->nnz)) return "null operand";
    if (on_device) {
        const size_t span_x = h->cols ? (count - 1) * stride_x + h->cols : 0, span_y = (count - 1) * stride_y + n_out;
        if (fr_spans_overlap(x, span_x, y, span_y)) return "y overlaps x (rows are owned by different waves: an in-place product races)";
    }
    return nullptr;
}
RustError snarkvm_hip_fr_spmv(void* y, size_t n_out, const snarkvm_hip_fr_matrix_t* h, const void* x, size_t count, size_t stride_x, size_t stride_y, int on_device) {
    if (h && (count == 0 || (n_out == 0 && h->rows == 0))) return ok();
    if (const char* why = fr_spmv_check(y, n_out, h, x, count, stride_x, stride_y, on_device)) return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_spmv: ") + why);
    if (count == 1) stride_x = stride_y = 0;
    API_BEGIN_DEV(device_for(y, on_device ? 1 : 0))
    const uint8_t* blk = h->on(c, "fr_spmv: the matrix has no replica on this device");
    const fr_mem_t* dx = (const fr_mem_t*)x;
    fr_mem_t* dy = (fr_mem_t*)y;
    size_t sx = stride_x, sy = stride_y;
    if (on_device) {
        fr_same_device(c, x, "fr_spmv: x lives on another device than y");
    } else {
        // host operands: x as it lies (members and the gaps between them), y packed member after member and downloaded member by member
        dx = fr_stage_in(c, 0, x, h->cols ? (count - 1) * stride_x + h->cols : 0, 0);
        dy = fr_stage_out(c, 1, y, count * n_out, 0);
        sy = n_out;
    }
    c.poly[4].ensure(sizeof(fr_mem_t) * (count * h->nparts ? count * h->nparts : 1));
    fr_mem_t* parts = c.poly[4].as<fr_mem_t>();
    switch (h->width) {
        case 4: fr_spmv_launch<4>(c, *h, blk, dx, sx, dy, sy, n_out, count, parts); break;
        case 8: fr_spmv_launch<8>(c, *h, blk, dx, sx, dy, sy, n_out, count, parts); break;
        case 16: fr_spmv_launch<16>(c, *h, blk, dx, sx, dy, sy, n_out, count, parts); break;
        default: fr_spmv_launch<64>(c, *h, blk, dx, sx, dy, sy, n_out, count, parts); break;
    }
    HIP_TRY(hipGetLastError());
    if (!on_device)
        for (size_t m = 0; m < count; m++) HIP_TRY(hipMemcpyAsync((fr_mem_t*)y + m * stride_y, dy + m * n_out, sizeof(fr_mem_t) * n_out, hipMemcpyDeviceToHost, c.stream));
    fr_call_done(c, on_device);
    API_END
}
// The product on host memory with the CPU in the kernels' place, for a GIVEN segment size and lane-group width: the same validation and layout,
// every lane of every segment through fr_spmv_lane, the butterfly level by level over the lanes it exchanges between, the partials, the fix-up
// launch with its own lanes and butterfly, the zero tail.  0, or -1 when refused.
static fr_t fr_spmv_tree_host(std::vector<fr_t>& lanes) {
    const size_t w = lanes.size();
    for (size_t off = w / 2; off >= 1; off >>= 1) {
        std::vector<fr_t> next(w);
        for (size_t l = 0; l < w; l++) next[l] = lanes[l] + lanes[l ^ off];
        lanes.swap(next);
    }
    return lanes[0];
}
int snarkvm_hip_selftest_fr_spmv(void* y, size_t n_out, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, const void* x,
                                 uint32_t seg, uint32_t width) {
    if (fr_spmv_matrix_check(rows, cols, row_ptr, col_idx, vals)) return -1;
    if (seg < 1 || (width != 4 && width != 8 && width != 16 && width != 64)) return -1;
    if (n_out < rows || n_out > FR_SPMV_DIM_MAX || (n_out && !y) || (row_ptr[rows] && !x)) return -1;
    std::vector<fr_spmv_seg_t> segs;
    std::vector<fr_spmv_fix_t> fix;
    const size_t nparts = fr_spmv_layout(rows, row_ptr, seg, segs, fix);
    std::vector<fr_mem_t> parts(nparts ? nparts : 1);
    fr_mem_t* py = (fr_mem_t*)y;
    std::vector<fr_t> lanes(width);
    for (const fr_spmv_seg_t& s : segs) {
        lanes.resize(width);
        for (uint32_t l = 0; l < width; l++) lanes[l] = fr_spmv_lane((const fr_mem_t*)vals + s.first, col_idx + s.first, (const fr_mem_t*)x, s.count, l, width);
        const fr_t v = fr_spmv_tree_host(lanes);
        if (s.part == FR_SPMV_SOLE)
            fr_spmv_finish(v).store(&py[s.row]);
        else
            v.store(&parts[s.part]);
    }
    for (const fr_spmv_fix_t& f : fix) {
        lanes.resize(width);
        for (uint32_t l = 0; l < width; l++) lanes[l] = fr_reduce_thread<FR_REDUCE_SUM>(parts.data() + f.first, nullptr, f.count, l, width);
        fr_spmv_finish(fr_spmv_tree_host(lanes)).store(&py[f.row]);
    }
    for (size_t r = rows; r < n_out; r++) fr_t::zero().store(&py[r]);
    return 0;
}
// what registration lays out for a matrix of `rows` rows and nnz entries spread evenly (the first nnz % rows rows one entry longer): out4 = {segment
// size S, lane-group width, threads per workgroup, segments}
int snarkvm_hip_selftest_fr_spmv_geometry(size_t rows, size_t nnz, uint32_t* out4) {
    if (!out4 || nnz > 0xFFFFFFFFull || rows > FR_SPMV_DIM_MAX || (nnz && !rows)) return -1;
    const size_t S = FR_SPMV_SEG, lo = rows ? nnz / rows : 0, longer = rows ? nnz % rows : 0;
    const size_t nseg = longer * ((lo + 1 + S - 1) / S) + (rows - longer) * ((lo + S - 1) / S);
    out4[0] = (uint32_t)S, out4[1] = fr_spmv_width(nnz, nseg), out4[2] = FR_SPMV_B, out4[3] = (uint32_t)nseg;
    return 0;
}

// ---- Varuna round 4: matrix-sumcheck evaluations over a registered arithmetization (poly.hip.h: fr_sumcheck_evals_kernel) -----------
static constexpr size_t FR_ARITH_K_MAX = (size_t)1 << NTT_LG_MAX;
RustError snarkvm_hip_fr_arith_register(snarkvm_hip_fr_arith_t** handle, size_t k, const void* row, const void* col, const void* row_col_val) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: null handle");
    *handle = nullptr;
    if (k > FR_ARITH_K_MAX) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: more than 2^28 elements");
    if (k && (!row || !col || !row_col_val)) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register: null array of a non-empty arithmetization");
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_arith> h(new snarkvm_hip_fr_arith());
    h->k = k;
    const size_t bytes = sizeof(fr_mem_t) * k;
    h->fill_all(3 * bytes, [&](lane_t& c, fr_mem_t* d) {  // every device uploads its own replica
        if (!k) return;
        HIP_TRY(hipMemcpyAsync(d, row, bytes, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(d + k, col, bytes, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(d + 2 * k, row_col_val, bytes, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
    *handle = h.release();
    API_CATCH
}
void snarkvm_hip_fr_arith_free(snarkvm_hip_fr_arith_t* h) {
    if (!h) return;
    h->free_all();
    delete h;
}
// one wanted output of a call: member, which of a / b / f, the caller's pointer, elements
struct fr_sumcheck_out_t {
    size_t m;
    int which;
    uint8_t* p;
    size_t k;
};
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device.  outs: every non-NULL output of a member with k > 0.
static const char* fr_sumcheck_check(const snarkvm_hip_fr_arith_t* const* ariths, size_t count, void* const* a, void* const* b, void* const* f, const void* alpha,
                                     const void* beta, const void* scales, std::vector<fr_sumcheck_out_t>& outs) {
    if (count > (size_t)FR_SUMCHECK_MEMBERS) return "more than 16 members";
    if (!ariths) return "null list of handles";
    for (size_t m = 0; m < count; m++)
        if (!ariths[m]) return "null handle in the list";
    if (!alpha || !beta || !scales) return "null alpha, beta or scales";
    void* const* lists[3] = {a, b, f};
    for (size_t m = 0; m < count; m++)
        for (int w = 0; w < 3; w++)
            if (ariths[m]->k && lists[w] && lists[w][m]) outs.push_back({m, w, (uint8_t*)lists[w][m], ariths[m]->k});
    std::vector<fr_range_t> rs;
    for (const fr_sumcheck_out_t& o : outs) rs.push_back({o.p, sizeof(fr_mem_t) * o.k, true});
    return fr_output_overlaps(std::move(rs)) ? "two outputs overlap" : nullptr;
}
RustError snarkvm_hip_fr_matrix_sumcheck_evals(const snarkvm_hip_fr_arith_t* const* ariths, size_t count, void* const* a_evals, void* const* b_evals, void* const* f_evals,
                                               const void* alpha, const void* beta, const void* scales, int on_device) {
    if (count == 0) return ok();
    std::vector<fr_sumcheck_out_t> outs;
    if (const char* why = fr_sumcheck_check(ariths, count, a_evals, b_evals, f_evals, alpha, beta, scales, outs))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_matrix_sumcheck_evals: ") + why);
    if (outs.empty()) return ok();  // every k_m == 0, or nothing wanted
    API_BEGIN_DEV(device_for(outs[0].p, on_device ? 1 : 0))
    if (on_device)
        for (const fr_sumcheck_out_t& o : outs) fr_same_device(c, o.p, "fr_matrix_sumcheck_evals: the outputs live on different devices");
    fr_sumcheck_t tab{};
    size_t threads = 0, total = 0;
    for (const fr_sumcheck_out_t& o : outs) {
        const snarkvm_hip_fr_arith& h = *ariths[o.m];
        const fr_mem_t* d = h.on(c, "fr_matrix_sumcheck_evals: a handle has no replica on this device");
        fr_sumcheck_member_t& mb = tab.m[o.m];
        mb.row = d, mb.col = d + h.k, mb.rcv = d + 2 * h.k;
        mb.k = h.k, mb.T = fr_sumcheck_threads(h.k);
        if (mb.T > threads) threads = mb.T;
        total += o.k;
    }
    fr_host_pack_t pack(c);
    if (!on_device) pack.begin(0, total);  // the wanted outputs, nothing else
    for (const fr_sumcheck_out_t& o : outs) {
        fr_sumcheck_member_t& mb = tab.m[o.m];
        (o.which == 0 ? mb.a : (o.which == 1 ? mb.b : mb.f)) = on_device ? (fr_mem_t*)o.p : pack.out(o.p, o.k);
    }
    const uint8_t* sc = (const uint8_t*)scales;
    const fr_mem_t sc3[3] = {fr_mem_from_host(sc), fr_mem_from_host(sc + sizeof(fr_mem_t)), fr_mem_from_host(sc + 2 * sizeof(fr_mem_t))};
    tab.cs = fr_sumcheck_consts(fr_mem_from_host(alpha), fr_mem_from_host(beta), sc3);
    hipLaunchKernelGGL(fr_sumcheck_evals_kernel, dim3((unsigned)((threads + FR_SUMCHECK_B - 1) / FR_SUMCHECK_B), (unsigned)count), dim3(FR_SUMCHECK_B), 0, c.stream, tab);
    HIP_TRY(hipGetLastError());
    pack.download();
    fr_call_done(c, on_device);
    API_END
}
// One member on host memory with the CPU in the kernel's place over blocks x threads threads: the same constants, every thread through
// fr_sumcheck_thread.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_sumcheck(void* a, void* b, void* f, const void* row, const void* col, const void* rcv, size_t k, const void* alpha, const void* beta,
                                     const void* scales, uint32_t blocks, uint32_t threads) {
    if (k > FR_ARITH_K_MAX || (k && (!row || !col || !rcv)) || !alpha || !beta || !scales || blocks < 1 || threads < 1) return -1;
    const uint8_t* sc = (const uint8_t*)scales;
    const fr_mem_t sc3[3] = {fr_mem_from_host(sc), fr_mem_from_host(sc + sizeof(fr_mem_t)), fr_mem_from_host(sc + 2 * sizeof(fr_mem_t))};
    const fr_sumcheck_consts_t cs = fr_sumcheck_consts(fr_mem_from_host(alpha), fr_mem_from_host(beta), sc3);
    fr_sumcheck_member_t mb{(const fr_mem_t*)row, (const fr_mem_t*)col, (const fr_mem_t*)rcv, (fr_mem_t*)a, (fr_mem_t*)b, (fr_mem_t*)f, k, (size_t)blocks * threads};
    for (size_t t = 0; t < mb.T && t < k; t++) fr_sumcheck_thread(mb, cs, t);
    return 0;
}
// what snarkvm_hip_fr_matrix_sumcheck_evals launches for a member of k elements: out4 = {threads, threads per workgroup, workgroups, elements per thread}
int snarkvm_hip_selftest_fr_sumcheck_geometry(size_t k, uint32_t* out4) {
    if (!out4 || k > FR_ARITH_K_MAX) return -1;
    const size_t T = fr_sumcheck_threads(k);
    out4[0] = (uint32_t)T, out4[1] = FR_SUMCHECK_B, out4[2] = (uint32_t)((T + FR_SUMCHECK_B - 1) / FR_SUMCHECK_B), out4[3] = (uint32_t)fr_sumcheck_share(k);
    return 0;
}

// ---- the circuit index: the arithmetization of a CSR matrix on K (poly.hip.h: fr_arithmetize_kernel) ---------------------------------
// nullptr, or why the call is refused (hipErrorInvalidValue); needs no device and touches nothing.  host_csr: the CSR arrays can be read here -
// after it no index the kernel will ever see points outside row_ptr, col_idx, vals or a table.  Device CSR: the contents are the caller's contract.
static const char* fr_arith_check(void* const* outs, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, uint32_t lg_constraint,
                                  uint32_t lg_variable, uint32_t lg_input, bool host_csr) {
    if (lg_constraint > (uint32_t)NTT_LG_MAX || lg_variable > (uint32_t)NTT_LG_MAX || lg_input > (uint32_t)NTT_LG_MAX) return "a domain of more than 2^28 elements";
    if (lg_input >= lg_variable) return "other.size() must be smaller than self.size() (lg_input >= lg_variable)";
    if (k > FR_ARITH_K_MAX) return "more than 2^28 elements";
    if (rows > ((size_t)1 << lg_constraint)) return "more rows than the constraint domain has elements";
    if (!row_ptr) return "null row_ptr";
    size_t span_vals = 1;  // device CSR: nnz cannot be read here - the first element of vals is checked, the rest is the caller's contract
    if (host_csr) {
        if (row_ptr[0] != 0) return "row_ptr[0] != 0";
        for (size_t r = 0; r < rows; r++)
            if (row_ptr[r + 1] < row_ptr[r]) return "row_ptr decreases";
        const uint64_t nnz = row_ptr[rows];
        if (nnz > 0xFFFFFFFFull) return "more than 2^32 - 1 entries";
        if (nnz && (!col_idx || !vals)) return "null col_idx or vals of a matrix with entries";
        if (k < nnz) return "k is less than the number of entries";
        for (uint64_t e = 0; e < nnz; e++)
            if (col_idx[e] >> lg_variable) return "a column index is not below the variable domain size";
        span_vals = (size_t)nnz;
    }
    for (int i = 0; i < 4; i++) {
        if (fr_spans_overlap(outs[i], k, vals, span_vals)) return "an output overlaps vals";
        for (int j = i + 1; j < 4; j++)
            if (fr_spans_overlap(outs[i], k, outs[j], k)) return "two outputs overlap";
    }
    return nullptr;
}
static fr_mem_t fr_domain_generator_mem(uint32_t lg) {  // fr_domain_generator, memory form
    fr_mem_t m;
    fr_domain_generator(lg).to_mem_mont().store(&m);
    return m;
}
// everything of a kernel argument but the pointers
static fr_arith_t fr_arith_args(size_t k, size_t rows, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, uint32_t s_r, uint32_t s_c) {
    fr_arith_t a{};
    fr_t::one().to_mem_mont().store(&a.one);
    const fr_t fix2 = fr_t::one().from_mem_mont().from_mem_mont();
    for (int l = 0; l < 9; l++) a.fix2[l] = fix2.v[l];
    a.k = (uint32_t)k, a.rows = (uint32_t)rows;
    a.s_r = s_r, a.mask_r = (1u << lg_constraint) - 1, a.s_c = s_c, a.mask_c = (1u << lg_variable) - 1;
    a.input_size = 1u << lg_input, a.period = 1u << (lg_variable - lg_input);
    return a;
}
// the tables and the pass, enqueued on the lane's stream; every pointer is device memory of the lane's device.  Tables: c.poly[4].
static void fr_arith_run(lane_t& c, fr_mem_t* const* outs, size_t k, size_t rows, const uint64_t* d_row_ptr, const uint32_t* d_col, const fr_mem_t* d_vals,
                         uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input) {
    const uint32_t s_r = fr_arith_split(lg_constraint), s_c = FR_ARITH_FULL_TABLE ? lg_variable : fr_arith_split(lg_variable);
    const size_t n_r = ((size_t)1 << s_r) + ((size_t)1 << (lg_constraint - s_r)), n_c = ((size_t)1 << s_c) + ((size_t)1 << (lg_variable - s_c));
    c.poly[4].ensure(sizeof(fr_mem_t) * (n_r + n_c));
    fr_mem_t* t = c.poly[4].as<fr_mem_t>();
    fr_arith_t a = fr_arith_args(k, rows, lg_constraint, lg_variable, lg_input, s_r, s_c);
    a.row = outs[0], a.col = outs[1], a.row_col = outs[2], a.rcv = outs[3];
    a.row_ptr = d_row_ptr, a.col_idx = d_col, a.vals = d_vals;
    a.r_lo = t, a.r_hi = t + ((size_t)1 << s_r), a.c_lo = t + n_r, a.c_hi = t + n_r + ((size_t)1 << s_c);
    hipLaunchKernelGGL(fr_arith_tables_kernel, dim3((unsigned)((n_r + 255) / 256)), dim3(256), 0, c.stream, t, t + ((size_t)1 << s_r), fr_domain_generator_mem(lg_constraint), s_r,
                       (uint32_t)n_r);
#if FR_ARITH_FULL_TABLE  // measurement variant: w_C^x for every x of the variable domain, as fr_lagrange_coefficients forms them
    hipLaunchKernelGGL(fr_fill_kernel, dim3(fr_grid((size_t)1 << lg_variable)), dim3(256), 0, c.stream, t + n_r, (size_t)1 << lg_variable, a.one);
    fr_distribute_powers_run(c, t + n_r, (size_t)1 << lg_variable, fr_domain_generator_mem(lg_variable), a.one);
#else
    hipLaunchKernelGGL(fr_arith_tables_kernel, dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0, c.stream, t + n_r, t + n_r + ((size_t)1 << s_c),
                       fr_domain_generator_mem(lg_variable), s_c, (uint32_t)n_c);
#endif
    hipLaunchKernelGGL(fr_arithmetize_kernel, dim3(fr_grid(k)), dim3(256), 0, c.stream, a);
    HIP_TRY(hipGetLastError());
}
// the host CSR arrays as device pointers in c.poly[0 .. 2]
static void fr_arith_stage_csr(lane_t& c, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals, const uint64_t*& d_row_ptr, const uint32_t*& d_col,
                               const fr_mem_t*& d_vals) {
    const size_t nnz = (size_t)row_ptr[rows];
    c.poly[0].ensure(sizeof(uint64_t) * (rows + 1) + (FR_ARITH_ROW_INDEX ? sizeof(uint32_t) * nnz : 0));
    c.poly[1].ensure(sizeof(uint32_t) * (nnz ? nnz : 1));
    HIP_TRY(hipMemcpyAsync(c.poly[0].p, row_ptr, sizeof(uint64_t) * (rows + 1), hipMemcpyHostToDevice, c.stream));
#if FR_ARITH_ROW_INDEX  // measurement variant: the row of every entry, expanded here and laid behind row_ptr (the copy is synchronous: pageable memory)
    {
        std::vector<uint32_t> row_of(nnz);
        for (size_t r = 0; r < rows; r++)
            for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) row_of[e] = (uint32_t)r;
        if (nnz) HIP_TRY(hipMemcpy(c.poly[0].as<uint64_t>() + rows + 1, row_of.data(), sizeof(uint32_t) * nnz, hipMemcpyHostToDevice));
    }
#endif
    if (nnz) HIP_TRY(hipMemcpyAsync(c.poly[1].p, col_idx, sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, c.stream));
    d_row_ptr = c.poly[0].as<uint64_t>(), d_col = c.poly[1].as<uint32_t>();
    d_vals = fr_stage_in(c, 2, nnz ? vals : nullptr, nnz, 0);
}
RustError snarkvm_hip_fr_arithmetize(void* row, void* col, void* row_col, void* row_col_val, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                                     const void* vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, int on_device) {
    void* const outs[4] = {row, col, row_col, row_col_val};
    if (const char* why = fr_arith_check(outs, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, !on_device))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_arithmetize: ") + why);
    void* first = row ? row : (col ? col : (row_col ? row_col : row_col_val));
    if (k == 0 || !first) return ok();
    API_BEGIN_DEV(device_for(first, on_device ? 1 : 0))
    fr_mem_t* d_outs[4] = {(fr_mem_t*)row, (fr_mem_t*)col, (fr_mem_t*)row_col, (fr_mem_t*)row_col_val};
    const uint64_t* d_row_ptr = row_ptr;
    const uint32_t* d_col = col_idx;
    const fr_mem_t* d_vals = (const fr_mem_t*)vals;
    fr_host_pack_t pack(c);
    if (on_device) {
        const char* why = "fr_arithmetize: the operands live on different devices";
        for (int i = 0; i < 4; i++) fr_same_device(c, outs[i], why);
        fr_same_device(c, row_ptr, why);
        fr_same_device(c, col_idx, why);
        fr_same_device(c, vals, why);
    } else {  // the CSR arrays in three lane buffers, the wanted outputs in a fourth
        fr_arith_stage_csr(c, rows, row_ptr, col_idx, vals, d_row_ptr, d_col, d_vals);
        size_t wanted = 0;
        for (int i = 0; i < 4; i++) wanted += outs[i] ? 1 : 0;
        pack.begin(3, wanted * k);
        for (int i = 0; i < 4; i++)
            if (outs[i]) d_outs[i] = pack.out(outs[i], k);
    }
    fr_arith_run(c, d_outs, k, rows, d_row_ptr, d_col, d_vals, lg_constraint, lg_variable, lg_input);
    pack.download();
    fr_call_done(c, on_device);
    API_END
}
RustError snarkvm_hip_fr_arith_register_csr(snarkvm_hip_fr_arith_t** handle, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx, const void* vals,
                                            uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input) {
    if (!handle) return fail((int)hipErrorInvalidValue, "snarkvm_hip: fr_arith_register_csr: null handle");
    *handle = nullptr;
    void* const none[4] = {nullptr, nullptr, nullptr, nullptr};
    if (const char* why = fr_arith_check(none, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, true))
        return fail((int)hipErrorInvalidValue, std::string("snarkvm_hip: fr_arith_register_csr: ") + why);
    API_TRY
    std::unique_ptr<snarkvm_hip_fr_arith> h(new snarkvm_hip_fr_arith());
    h->k = k;
    h->fill_all(3 * sizeof(fr_mem_t) * k, [&](lane_t& c, fr_mem_t* d) {  // every device computes its own replica from the CSR arrays
        if (!k) return;
        const uint64_t* d_row_ptr;
        const uint32_t* d_col;
        const fr_mem_t* d_vals;
        fr_arith_stage_csr(c, rows, row_ptr, col_idx, vals, d_row_ptr, d_col, d_vals);
        fr_mem_t* const outs[4] = {d, d + k, nullptr, d + 2 * k};
        fr_arith_run(c, outs, k, rows, d_row_ptr, d_col, d_vals, lg_constraint, lg_variable, lg_input);
        HIP_TRY(hipStreamSynchronize(c.stream));
    });
    *handle = h.release();
    API_CATCH
}
// snarkvm_hip_fr_arithmetize on host memory with the CPU in the kernel's place, for a GIVEN table split (split_bits low bits per domain, cut to the
// domain's lg) and `threads` threads: the same validation, the tables through fr_arith_table_at, thread t over e = t, t + threads, ... through
// fr_arith_at.  0, or -1 when refused.
int snarkvm_hip_selftest_fr_arithmetize(void* row, void* col, void* row_col, void* row_col_val, size_t k, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx,
                                        const void* vals, uint32_t lg_constraint, uint32_t lg_variable, uint32_t lg_input, uint32_t split_bits, uint32_t threads) {
    void* const outs[4] = {row, col, row_col, row_col_val};
    if (FR_ARITH_FULL_TABLE || FR_ARITH_ROW_INDEX) return -1;  // a measurement variant has no twin
    if (threads < 1 || fr_arith_check(outs, k, rows, row_ptr, col_idx, vals, lg_constraint, lg_variable, lg_input, true)) return -1;
    const uint32_t s_r = split_bits < lg_constraint ? split_bits : lg_constraint, s_c = split_bits < lg_variable ? split_bits : lg_variable;
    const size_t n_r = ((size_t)1 << s_r) + ((size_t)1 << (lg_constraint - s_r)), n_c = ((size_t)1 << s_c) + ((size_t)1 << (lg_variable - s_c));
    std::vector<fr_mem_t> tab(n_r + n_c);
    const fr_mem_t w_r = fr_domain_generator_mem(lg_constraint), w_c = fr_domain_generator_mem(lg_variable);
    for (size_t t = 0; t < n_r; t++) fr_arith_table_at(tab.data(), tab.data() + ((size_t)1 << s_r), fr_t::load(&w_r).from_mem_mont(), s_r, (uint32_t)t);
    for (size_t t = 0; t < n_c; t++) fr_arith_table_at(tab.data() + n_r, tab.data() + n_r + ((size_t)1 << s_c), fr_t::load(&w_c).from_mem_mont(), s_c, (uint32_t)t);
    fr_arith_t a = fr_arith_args(k, rows, lg_constraint, lg_variable, lg_input, s_r, s_c);
    a.row = (fr_mem_t*)row, a.col = (fr_mem_t*)col, a.row_col = (fr_mem_t*)row_col, a.rcv = (fr_mem_t*)row_col_val;
    a.row_ptr = row_ptr, a.col_idx = col_idx, a.vals = (const fr_mem_t*)vals;
    a.r_lo = tab.data(), a.r_hi = tab.data() + ((size_t)1 << s_r), a.c_lo = tab.data() + n_r, a.c_hi = tab.data() + n_r + ((size_t)1 << s_c);
    const uint32_t nnz = (uint32_t)row_ptr[rows];
    for (size_t t = 0; t < threads && t < k; t++)
        for (size_t e = t; e < k; e += threads) fr_arith_at(a, nnz, (uint32_t)e);
    return 0;
}
// what snarkvm_hip_fr_arithmetize launches for k elements, and the table split of a domain of 2^lg elements: out4 = {workgroups, threads per
// workgroup, the cap on workgroups, split bits s}
int snarkvm_hip_selftest_fr_arithmetize_geometry(size_t k, uint32_t lg, uint32_t* out4) {
    if (!out4 || k > FR_ARITH_K_MAX || lg > (uint32_t)NTT_LG_MAX) return -1;
    out4[0] = fr_grid(k), out4[1] = 256, out4[2] = 8192, out4[3] = fr_arith_split(lg);
    return 0;
}

}  // extern "C"
