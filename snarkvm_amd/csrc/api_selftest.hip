// api_selftest.hip - the test hooks that need no MSM entry point: the field operations on the host and in a kernel (snarkvm_hip_selftest_field /
// snarkvm_hip_devtest_field), the MSM planner, the naive G1 sum, the lazily reduced G1 arithmetic, the host-side finish of an MSM, and the lane-pair and
// sixteen-lane Fq2 arithmetic of the G2 kernels on simulated lanes, and the host twin of the assignment gather of Varuna's round 1 (the refusals it shares
// with the entry point: fr_call.hip.h).  All but devtest_field run on the host alone.  A translation unit of its own (as api_msmtest.hip): the units that own
// the MSM entry points compile without them.  python -m snarkvm_amd.build --fast (SV_NO_G2) leaves the two G2 hooks as the refusal at the end of this file.
#include "msm_run.hip.h"
#include "g1_generator.hip.h"
#include "testrng.hip.h"
#include "fr_call.hip.h"  // fr_assignment_check, fr_grid

static void tu_set_kernel_attributes() {}  // no kernel of this unit needs an attribute

// the field operation of snarkvm_hip_selftest_field (host) and snarkvm_hip_devtest_field (kernel); C++ linkage
template <class F>
SV_HD void field_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    // operands are memory-form Montgomery residues: convert to internal, operate, convert back
    F x = F::unpack(a).from_mem_mont();
    F y = F::unpack(b).from_mem_mont();
    F r;
    switch (op) {
        case 0: r = x + y; break;
        case 1: r = x - y; break;
        case 2: r = x * y; break;
        case 3: r = x.sqr(); break;
        case 4: r = x.inverse(); break;
        case 5: r = x.neg(); break;
        case 6: r = F::unpack(a).int_to_mont(); break;                  // from_bigint: integer -> Montgomery
        case 7: (x.mont_to_int()).pack(out); return;                    // to_bigint: Montgomery -> integer
        case 9: r = F::diff_of_products(x, y, y, x + y); break;  // x*y - y*(x+y) with one reduction
        case 8: {  // lazy-arithmetic chain used by the NTT butterflies (Fr only): ((a + b) - b + 2r) * b == a * b
            if (F::N != 9) { r = x * y; break; }
            uint32_t kp[F::N];
            F::mod_shl(kp, 1);
            F t = F::add_lazy(x, y);         // < 2r
            t = F::sub_lazy(t, y, kp);       // < 4r
            r = t.mul_lazy(y).reduce_lazy();
            break;
        }
        default: r = F::zero();
    }
    r.to_mem_mont().pack(out);
}
static __global__ void devtest_field_kernel(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (field == 0)
        field_op<fr_t>(op, a + 8 * i, b + 8 * i, out + 8 * i);
    else
        field_op<fq_t>(op, a + 12 * i, b + 12 * i, out + 12 * i);
}
extern "C" {
int snarkvm_hip_selftest_field(int field, int op, const void* a, const void* b, void* out, size_t n) {
    const uint32_t* A = (const uint32_t*)a;
    const uint32_t* B = (const uint32_t*)(b ? b : a);
    uint32_t* O = (uint32_t*)out;
    for (size_t i = 0; i < n; i++) {
        if (field == 0)
            field_op<fr_t>(op, A + 8 * i, B + 8 * i, O + 8 * i);
        else if (field == 1)
            field_op<fq_t>(op, A + 12 * i, B + 12 * i, O + 12 * i);
        else
            return 1;
    }
    return 0;
}
RustError snarkvm_hip_devtest_field(int field, int op, const void* a, const void* b, void* out, size_t n) {
    API_BEGIN
    if (field < 0 || field > 1) throw hip_failure{hipErrorInvalidValue, "devtest_field: field must be 0 or 1", __LINE__};
    const size_t bytes = n * (field == 0 ? 32 : 48);
    c.poly[0].ensure(bytes + 16);
    c.poly[1].ensure(bytes + 16);
    c.poly[2].ensure(bytes + 16);
    HIP_TRY(hipMemcpyAsync(c.poly[0].p, a, bytes, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipMemcpyAsync(c.poly[1].p, b ? b : a, bytes, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(devtest_field_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, field, op, c.poly[0].as<uint32_t>(),
                       c.poly[1].as<uint32_t>(), c.poly[2].as<uint32_t>(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c.poly[2].p, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    API_END
}
// The MSM planner on the host (no device needed): out = {c, W, J, Wd, nb, nbt, S, S2, L, wide}.  Returns 0.
int snarkvm_hip_selftest_msm_plan(size_t n, int window_bits, int tables, int table_bits, uint32_t* out) {
    const msm_plan_t p = msm_make_plan(n, window_bits, tables, table_bits);
    const uint32_t v[10] = {(uint32_t)p.c, (uint32_t)p.W, (uint32_t)p.J, (uint32_t)p.Wd, p.nb, p.nbt, p.S, p.S2, p.L, p.c > 16 ? 1u : 0u};
    for (int i = 0; i < 10; i++) out[i] = v[i];
    // bias must place one 2^(c-1) per digit row below MSM_BIAS_BITS
    uint32_t chk[10] = {0};
    for (int w = 0; w < p.Wd; w++) {
        const int bit = p.c - 1 + p.c * w;
        if (bit >= MSM_BIAS_BITS) return 1;
        chk[bit / 32] |= 1u << (bit % 32);
    }
    for (int i = 0; i < 10; i++)
        if (chk[i] != p.bias[i]) return 2;
    return 0;
}
// naive sum_i scalar_i * P_i on the host with the device point arithmetic (scalars: 256-bit, 32 B each)
int snarkvm_hip_selftest_g1_msm_naive(const void* points, size_t npoints, size_t stride, const void* scalars, void* out) {
    const uint8_t* P = (const uint8_t*)points;
    const uint32_t* S = (const uint32_t*)scalars;
    g1_xyzz_t total = g1_xyzz_t::inf();
    for (size_t i = 0; i < npoints; i++) {
        const uint32_t* src = (const uint32_t*)(P + i * stride);
        g1_aff_t a;
        if (src[24] & 0xff)
            a = g1_aff_t::inf();
        else
            a = {fq_t::unpack(src).from_mem_mont(), fq_t::unpack(src + 12).from_mem_mont()};
        g1_xyzz_t acc = g1_xyzz_t::inf();
        for (int bit = 255; bit >= 0; bit--) {
            acc = acc.dbl();
            if ((S[8 * i + bit / 32] >> (bit % 32)) & 1) acc.add_affine(a);
        }
        // route half of the additions through the xyzz+xyzz law and the negation path
        if (i & 1) {
            g1_xyzz_t neg = acc;
            neg.y = neg.y.neg();
            g1_xyzz_t t2 = total;
            t2.add(acc);
            t2.add(neg);  // + acc - acc
            t2.add(acc);
            total = t2;
        } else {
            total.add(acc);
        }
    }
    const g1_jac_t j = total.to_jacobian();
    uint32_t* o = (uint32_t*)out;
    j.x.to_mem_mont().pack(o);
    j.y.to_mem_mont().pack(o + 12);
    j.z.to_mem_mont().pack(o + 24);
    return 0;
}
// The lazily reduced accumulate arithmetic (ffl.hip.h) against the exact one (ff.hip.h / ec.hip.h) on the host, no device needed:
// a chain of `iters` mixed additions of +-k G (k from a SplitMix64 stream over a pool of 64 multiples of the generator, so that
// P + P, P + (-P) and additions to infinity all occur), every coordinate of the accumulator compared after every step; also the
// field routines on values at the edges of their documented ranges.  Returns 0, or the (1-based) step of the first mismatch.
int snarkvm_hip_selftest_fq_lazy(uint64_t seed, int iters) {
    const g1_aff_t g = g1_generator();
    // pool[k] = (k + 1) G, affine, exact internal form
    std::vector<g1_aff_t> pool;
    g1_xyzz_t run = g1_xyzz_t::inf();
    for (int k = 0; k < 64; k++) {
        run.add_affine(g);
        const fq_t izzz = run.zzz.inverse();
        const fq_t izz = izzz.sqr() * run.zz.sqr();
        pool.push_back({run.x * izz, run.y * izzz});
    }
    const fq_t c406 = fq_t::from_table(FqLConv::C406), c348 = fq_t::from_table(FqLConv::C348);
    splitmix64_t next{seed};
    g1_xyzz_t exact = g1_xyzz_t::inf();
    xyzz_lazy_t lazy = xyzz_lazy_t::infinity();
    int prev = -1;
    bool prev_neg = false;
    for (int it = 0; it < iters; it++) {
        const uint64_t r = next();
        int k = (int)(r % 64);
        bool neg = ((r >> 8) & 1) != 0;
        const int mode = (int)((r >> 16) % 16);
        if (mode == 0 && prev >= 0) k = prev, neg = prev_neg;    // the same point again
        if (mode == 1 && prev >= 0) k = prev, neg = !prev_neg;   // its negative
        if (mode == 2) {                                         // restart from infinity: acc = P, then P again -> doubling
            exact = g1_xyzz_t::inf();
            lazy = xyzz_lazy_t::infinity();
        }
        prev = k;
        prev_neg = neg;
        const g1_aff_t p = pool[k];
        exact.add_affine(p, neg);
        const fql_t px = fql_t::from_limbs(p.x * c406), py = fql_t::from_limbs(p.y * c406);
        if (!lazy.madd(px, py, neg)) {  // exceptional (or a false alarm of the low-limb filter): the exact arithmetic decides
            g1_xyzz_t e = lazy.to_exact();
            fq_t ex, ey;
            for (int i = 0; i < 13; i++) ex.v[i] = (uint32_t)px.v[i], ey.v[i] = (uint32_t)py.v[i];
            e.add_affine({ex * c348, ey * c348}, neg);
            lazy = xyzz_lazy_t::from_exact(e);
        }
        const g1_xyzz_t got = lazy.to_exact();
        if (got.is_inf() != exact.is_inf()) return it + 1;
        if (!exact.is_inf() && (got.x != exact.x || got.y != exact.y || got.zz != exact.zz || got.zzz != exact.zzz)) return it + 1;
    }
    // field routines on operands at the edges of their ranges: a = -q .. values near +-q with extreme limbs
    for (int t = 0; t < 200; t++) {
        fq_t a, b;
        for (int i = 0; i < 13; i++) a.v[i] = (uint32_t)(next() & LIMB_MASK), b.v[i] = (uint32_t)(next() & LIMB_MASK);
        a.v[12] &= 0x00ffffffu;
        b.v[12] &= 0x00ffffffu;
        if (t & 1) for (int i = 0; i < 12; i++) a.v[i] = LIMB_MASK;  // all-ones limbs
        if (t & 2) for (int i = 0; i < 12; i++) b.v[i] = (i & 1) ? LIMB_MASK : 0;
        const fql_t la = fql_t::from_exact(a), lb = fql_t::from_exact(b);
        if (fql_t::mul(la, lb).to_exact() != a * b) return -(4 * t + 1);
        if (fql_t::sqr(la - lb).to_exact() != (a - b).sqr()) return -(4 * t + 2);
        if (fql_t::diff_of_products(la - lb, lb - la, fql_t::from_exact(a * b).normalized(), la).to_exact() != fq_t::diff_of_products(a - b, b - a, a * b, a))
            return -(4 * t + 3);
        if (((la + lb) - (lb + lb)).normalized().to_exact() != (a - b)) return -(4 * t + 4);
        // raw memory image (how partial sums leave the accumulate kernel): a wide signed value through store_raw / load_raw
        alignas(16) uint32_t raw[12];
        const fql_t wide = (la - lb - lb - lb).normalized();
        wide.store_raw(raw);
        const fql_t back = fql_t::load_raw(raw);
        for (int i = 0; i < 13; i++)
            if (back.v[i] != wide.v[i]) return -(100000 + t);
    }
    return 0;
}
// The lazy arithmetic behind field-like operators (ffl.hip.h::fqz_t: the tail of a G1 MSM under tuning lazy_tail) against the exact
// one, on the host: two chains over the generic xyzz_t<F> - F = fq_t and F = fqz_t - fed the same GENERAL points (multiples of the
// generator with random zz / zzz scalings, so that the full addition law runs, not the mixed one), with repeated points (the doubling
// inside the addition), negatives (infinity), restarts and explicit doublings; every coordinate of the lazy accumulator is converted and
// compared after every step.  Returns 0, or the (1-based) step of the first mismatch.
int snarkvm_hip_selftest_g1_lazy_tail(uint64_t seed, int iters) {
    const g1_aff_t g = g1_generator();
    std::vector<g1_xyzz_t> pool;
    g1_xyzz_t run = g1_xyzz_t::inf();
    for (int k = 0; k < 48; k++) {
        run.add_affine(g);
        pool.push_back(run);
    }
    splitmix64_t next{seed};
    auto to_lazy = [](const g1_xyzz_t& p) {
        xyzz_t<fqz_t> r = xyzz_t<fqz_t>::inf();
        if (!p.is_inf()) r = {{fql_t::from_exact(p.x)}, {fql_t::from_exact(p.y)}, {fql_t::from_exact(p.zz)}, {fql_t::from_exact(p.zzz)}};
        return r;
    };
    g1_xyzz_t exact = g1_xyzz_t::inf();
    xyzz_t<fqz_t> lazy = xyzz_t<fqz_t>::inf();
    g1_xyzz_t prev = g1_xyzz_t::inf();
    for (int it = 0; it < iters; it++) {
        const uint64_t r = next();
        g1_xyzz_t p = pool[r % 48];
        // another representative of the same point: (l^2 X, l^3 Y, l^2 ZZ, l^3 ZZZ)
        fq_t l = fq_t::zero();
        for (int i = 0; i < 12; i++) l.v[i] = (uint32_t)(next() & LIMB_MASK);
        l.v[0] |= 1;
        const fq_t l2 = l.sqr(), l3 = l2 * l;
        p = {p.x * l2, p.y * l3, p.zz * l2, p.zzz * l3};
        if ((r >> 8) & 1) p.y = p.y.neg();
        const int mode = (int)((r >> 16) % 16);
        if (mode == 0) p = prev;                                  // the same representative again
        if (mode == 1) p = {prev.x, prev.y.neg(), prev.zz, prev.zzz};  // its negative
        if (mode == 2) {                                         // restart: acc = P, then (next step, mode 0 or 3) P again -> doubling
            exact = g1_xyzz_t::inf();
            lazy = xyzz_t<fqz_t>::inf();
        }
        if (mode == 3) p = exact;                                // acc + acc: the doubling inside the addition
        if (mode == 4) {                                         // explicit doubling
            exact = exact.dbl();
            lazy = lazy.dbl();
        } else {
            prev = p;
            exact.add(p);
            lazy.add(to_lazy(p));
        }
        if (lazy.is_inf() != exact.is_inf()) return it + 1;
        if (!exact.is_inf() && (lazy.x.to_exact() != exact.x || lazy.y.to_exact() != exact.y || lazy.zz.to_exact() != exact.zz || lazy.zzz.to_exact() != exact.zzz))
            return it + 1;
        // the memory image the tail kernels exchange
        xyzz_mem_t<fqz_t> m;
        store_xyzz<fqz_t>(&m, lazy);
        lazy = load_xyzz<fqz_t>(&m);
    }
    // a representative of zero other than 0 is still the point at infinity / an equal coordinate: q and -q as limbs
    fqz_t zq;
    for (int i = 0; i < 13; i++) zq.a.v[i] = FqL::MOD[i];
    if (!zq.is_zero() || !zq.neg().is_zero() || !(zq + zq).is_zero() || (zq + fqz_t::one()).is_zero()) return -1;
    return 0;
}
// The host-side finish of an MSM (msm_run.hip.h msm_accum_t) on its own, no device needed: out (144 B) = sum_i 2^pos[i] *
// planes[i] for `n` G1 points given as Jacobian memory images.  Lets the CPU test-suite pin the Horner code on the oracle.
int snarkvm_hip_selftest_g1_finish(const void* planes_jacobian, const int32_t* pos, size_t n, void* out) {
    try {
        std::unique_ptr<msm_accum_t<fq_t>> acc(new msm_accum_t<fq_t>());
        const uint32_t* src = (const uint32_t*)planes_jacobian;
        for (size_t i = 0; i < n; i++) {
            const g1_jac_t j = {fq_t::from_raw_words(src + 36 * i), fq_t::from_raw_words(src + 36 * i + 12), fq_t::from_raw_words(src + 36 * i + 24)};
            acc->add(pos[i], g1_xyzz_t::from_jacobian(j));
        }
        acc->finish(out);
        return 0;
    } catch (...) {
        return 1;
    }
}

// snarkvm_hip_fr_assignment_evals on host memory with the CPU in the kernel's place, over a GIVEN thread count: the same validation, then per member
// thread t over k = t, t + threads, ... through the kernel's own per-index routine (poly.hip.h: fr_assignment_at).  0, or -1 when refused.
int snarkvm_hip_selftest_fr_assignment_evals(void* out, size_t n, const void* vars, size_t num_vars, size_t input_size, size_t count, size_t stride_out, size_t stride_vars,
                                             uint32_t threads) {
    if (threads < 1 || fr_assignment_check(out, n, vars, num_vars, input_size, count, stride_out, stride_vars)) return -1;
    if (count == 0 || n == 0) return 0;
    if (count == 1) stride_out = stride_vars = 0;
    for (size_t m = 0; m < count; m++)
        for (size_t t = 0; t < threads && t < n; t++)
            for (size_t k = t; k < n; k += threads)
                fr_assignment_at((fr_mem_t*)out + m * stride_out, (const fr_mem_t*)vars + m * stride_vars, (uint32_t)num_vars, (uint32_t)input_size, (uint32_t)(n / input_size),
                                 (uint32_t)k);
    return 0;
}
// what snarkvm_hip_fr_assignment_evals launches per member of n elements: out3 = {workgroups, threads per workgroup, the cap on the workgroups}
int snarkvm_hip_selftest_fr_assignment_geometry(size_t n, uint32_t* out3) {
    if (!out3 || n > FR_ASSIGNMENT_N_MAX) return -1;
    out3[0] = fr_grid(n, FR_ASSIGNMENT_BLOCK), out3[1] = FR_ASSIGNMENT_BLOCK, out3[2] = fr_grid(FR_ASSIGNMENT_N_MAX, FR_ASSIGNMENT_BLOCK);
    return 0;
}

#ifdef SV_NO_G2  // development builds only: no Fq2 arithmetic to test
int snarkvm_hip_selftest_fq2_pair(const void*, size_t, uint64_t, int) { return -1; }
int snarkvm_hip_selftest_g2_hex(const void*, size_t, uint64_t, int) { return -1; }
#else
// ---- test hook: the lane-pair Fq2 arithmetic of the G2 accumulate kernel (ffl2p.hip.h) against the exact arithmetic, on the host ----
// The SAME source the kernel runs (fq2p::xyzz_pair_t) instantiated with the two-lane host exchange policy: a chain of `iters` mixed
// additions of +- points[k] - the same point again (doubling, resolved inside the pair arithmetic), its negative (cancellation),
// restarts from infinity - with every coordinate component compared with xyzz_t<fq2_t>::add_affine after every step, the raw partial-sum
// image and its conversion on the way.  0 = identical; > 0: first differing step; < 0: a conversion case.
int snarkvm_hip_selftest_fq2_pair(const void* points, size_t npoints, uint64_t seed, int iters) {
    if (!points || npoints < 2) return -2;
    const std::vector<aff_t<fq2_t>> pool = g2_pool_from_records(points, npoints);
    splitmix64_t next{seed};
    auto same = [](const fql_t (&l)[2], const fq2_t& e) { return l[0].to_exact() == e.c0 && l[1].to_exact() == e.c1; };
    xyzz_t<fq2_t> exact = xyzz_t<fq2_t>::inf();
    fq2p::xyzz_pair_t<fq2p::xp_host> pr;
    pr.inf = true;
    int prev = -1;
    bool prev_neg = false;
    for (int it = 0; it < iters; it++) {
        const uint64_t r = next();
        int k = (int)(r % npoints);
        bool neg = ((r >> 8) & 1) != 0;
        const int mode = (int)((r >> 16) % 16);
        if (mode == 0 && prev >= 0) k = prev, neg = prev_neg;
        if (mode == 1 && prev >= 0) k = prev, neg = !prev_neg;
        if (mode == 2) {
            exact = xyzz_t<fq2_t>::inf();
            pr.inf = true;
        }
        prev = k;
        prev_neg = neg;
        const aff_t<fq2_t> p = pool[k];
        exact.add_affine(p, neg);
        // the base slot as the kernel reads it: component c of x and y
        alignas(128) aff_mem_t<fq2_t> slot;
        const fq_t c406 = fq_t::from_table(FqLConv::C406);
        g2_lazy_slot_t::store(&slot, {p.x.c0 * c406, p.x.c1 * c406}, {p.y.c0 * c406, p.y.c1 * c406}, false);
        fql_t px[2], py[2];
        for (int c = 0; c < 2; c++) ((const g2_lazy_slot_t*)&slot)->component(c, px[c], py[c]);
        pr.madd(px, py, neg);
        if (pr.inf != exact.is_inf()) return it + 1;
        if (!pr.inf && !(same(pr.x, exact.x) && same(pr.y, exact.y) && same(pr.zz, exact.zz) && same(pr.zzz, exact.zzz))) return it + 1;
        if (!pr.inf && (it & 7) == 0) {  // the raw partial-sum image through the conversion the device kernel applies per component
            const fql_t* cs[4] = {pr.x, pr.y, pr.zz, pr.zzz};
            const fq2_t* es[4] = {&exact.x, &exact.y, &exact.zz, &exact.zzz};
            for (int c4 = 0; c4 < 4; c4++)
                for (int c = 0; c < 2; c++) {
                    fql_t back;
                    for (int j = 0; j < 13; j++) back.v[j] = cs[c4][c].v[j];
                    if (!(back.to_exact() == (c ? es[c4]->c1 : es[c4]->c0))) return -(it + 1);
                }
        }
    }
    return 0;
}

// The sixteen-lane cooperative Fq2 addition of the G2 tail trees (csrc/hex2.hip.h) on sixteen SIMULATED lanes - the same source as the kernel's, every lane
// with its own copy of the state, the pair exchange and the gathers indexing the other lanes' copies - against xyzz_t<fq2_t>::add: `iters` additions of partial
// sums built from +- points[k] (general ZZ / ZZZ), with the cases a tree meets: an operand at infinity (either, both), P + P (every lane must ask for the
// plain law), P + (-P).  0 = every lane of every addition ends with exactly the exact sum; > 0: first differing iteration; < 0: bad arguments.
int snarkvm_hip_selftest_g2_hex(const void* points, size_t npoints, uint64_t seed, int iters) {
    if (!points || npoints < 2) return -2;
    const std::vector<aff_t<fq2_t>> pool = g2_pool_from_records(points, npoints);
    splitmix64_t next{seed};
    auto partial = [&](int terms) {  // a partial sum with general ZZ, ZZZ
        xyzz_t<fq2_t> a = xyzz_t<fq2_t>::inf();
        for (int t = 0; t < terms; t++) {
            const uint64_t r = next();
            a.add_affine(pool[r % npoints], ((r >> 40) & 1) != 0);
        }
        return a;
    };
    for (int it = 0; it < iters; it++) {
        const int mode = (int)(next() % 12);
        xyzz_t<fq2_t> a = partial(1 + (int)(next() % 3)), b = partial(1 + (int)(next() % 3));
        if (mode == 0) b = a;                                  // doubling: the equal-x fallback on every lane
        if (mode == 1) b = a, b.y = b.y.neg();                 // cancellation: equal x as well
        if (mode == 2) a = xyzz_t<fq2_t>::inf();
        if (mode == 3) b = xyzz_t<fq2_t>::inf();
        if (mode == 4) a = xyzz_t<fq2_t>::inf(), b = xyzz_t<fq2_t>::inf();
        xyzz_t<fq2_t> want = a;
        want.add(b);
        if (hex_add_host_check(a, b, want)) return it + 1;
        // the flagged plain addition of the tail kernels (xyzz_t::add_flag): equal x coordinates of two finite operands raise the flag and leave the accumulator
        // alone - P + P and P - P alike -, everything else is the exact sum and leaves the flag down
        xyzz_t<fq2_t> f = a;
        bool flagged = false;
        f.add_flag(b, flagged);
        const bool same_x = !a.is_inf() && !b.is_inf() && a.x * b.zz == b.x * a.zz;
        if (flagged != same_x) return 100000 + it + 1;
        const xyzz_t<fq2_t>& expect = flagged ? a : want;
        if (!(f.x == expect.x && f.y == expect.y && f.zz == expect.zz && f.zzz == expect.zzz)) return 200000 + it + 1;
    }
    return 0;
}
#endif

}  // extern "C"
