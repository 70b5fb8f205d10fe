// ffl2.hip.h - what the G2 bucket-accumulation loop shares on the signed limbs of ffl.hip.h: the per-component helpers of the lazily reduced
// Fq2 = Fq[u] / (u^2 + 5) arithmetic and the base-slot layout.  The arithmetic itself is ffl2p.hip.h (one Fq2 value over a lane pair); its
// round-4 predecessor, both components in one lane, lived here and is retired (HISTORY.md, "retired variants").
//
// Every product operand is "tight": normalised limbs (0 .. 11 in [0, 2^29), limb 12 signed) and a value within [-1, 1] q (+- 2^-26 q),
// i.e. every limb below 2^29 in magnitude.  The factor 5 of the non-residue never meets a reduced value (5 x a value within q overflows
// the signed top limb): it is folded into an OPERAND as a 14-limb normalised integer (times5: one shift-add and one carry per limb).
// Sums and differences of tight values are not tight; the addition law normalises each one with the multiple of q that brings it back
// (sub_norm), one carry pass each.
#pragma once
#include "ffl.hip.h"

namespace sv {

namespace fq2l {

static constexpr int N = 13;
static constexpr uint32_t MASK = fql_t::MASK;

// 5 b as 14 normalised limbs (limb 13: the small signed overflow).  b tight.
SV_HD void times5(const fql_t& b, int32_t* o) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const uint32_t x = 5u * (uint32_t)b.v[i] + c;  // < 5 * 2^29 + 5 < 2^32
        o[i] = (int32_t)(x & MASK);
        c = x >> 29;
    }
    const int64_t t = 5 * (int64_t)b.v[N - 1] + (int64_t)c;
    o[N - 1] = (int32_t)((uint32_t)t & MASK);
    o[N] = (int32_t)(t >> 29);
}
// a - b + add * q, carry-normalised.  add: 0, 1, or -1 for "q if the difference is negative" (decided on the top limbs: a carry
// from below can only matter within 2^-28 q of zero, where either choice keeps the value tight).
SV_HD fql_t sub_norm(const fql_t& a, const fql_t& b, int add) {
    int32_t mask = add > 0 ? -1 : 0;
    if (add < 0) mask = (a.v[N - 1] - b.v[N - 1]) < 0 ? -1 : 0;
    fql_t r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const int32_t x = a.v[i] - b.v[i] + (FqL::MOD[i] & mask) + c;
        r.v[i] = (int32_t)((uint32_t)x & MASK);
        c = x >> 29;
    }
    r.v[N - 1] = a.v[N - 1] - b.v[N - 1] + (FqL::MOD[N - 1] & mask) + c;
    SV_OPAQUE_13(r.v);
    return r;
}
// q - y for a canonical y (the negated base coordinate as a NON-NEGATIVE normalised value), or y itself
SV_HD fql_t cond_neg_canonical(const fql_t& y, bool neg) {
    const int32_t m = neg ? -1 : 0;
    fql_t r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const int32_t x = ((y.v[i] ^ m) - m) + (FqL::MOD[i] & m) + c;
        r.v[i] = (int32_t)((uint32_t)x & MASK);
        c = x >> 29;
    }
    r.v[N - 1] = ((y.v[N - 1] ^ m) - m) + (FqL::MOD[N - 1] & m) + c;
    SV_OPAQUE_13(r.v);
    return r;
}

}  // namespace fq2l

// A base slot of a G2 MSM on this arithmetic: the 256 bytes of an aff_mem_t<fq2_t> reinterpreted as four groups of 16 words - x.c0, x.c1,
// y.c0, y.c1: 13 limbs each (canonical residues of the coordinate components times 2^406, one 29-bit limb per word) and three words of
// padding, so that a lane of the pair kernel (ffl2p.hip.h) reads ITS component of a coordinate as four aligned 16-byte loads - and a flag
// word for the point at infinity in the first group's padding.
struct alignas(128) g2_lazy_slot_t {
    static constexpr int GROUP = 16, INF_WORD = 15;
    uint32_t w[64];  // [16 g, 16 g + 13): limbs of component g (x.c0, x.c1, y.c0, y.c1); w[15]: 1 = point at infinity
    // component `comp` (0: c0, 1: c1) of x and y
    SV_HD void component(int comp, fql_t& px, fql_t& py) const {
        const uint4* q = (const uint4*)w;
        uint32_t t[32];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 a = q[4 * comp + k], b = q[8 + 4 * comp + k];
            t[4 * k] = a.x, t[4 * k + 1] = a.y, t[4 * k + 2] = a.z, t[4 * k + 3] = a.w;
            t[16 + 4 * k] = b.x, t[16 + 4 * k + 1] = b.y, t[16 + 4 * k + 2] = b.z, t[16 + 4 * k + 3] = b.w;
        }
#pragma unroll
        for (int i = 0; i < 13; i++) px.v[i] = (int32_t)t[i], py.v[i] = (int32_t)t[16 + i];
        SV_OPAQUE_13(px.v);
        SV_OPAQUE_13(py.v);
    }
    // x406, y406: canonical residues of coordinate * 2^406 (exact-arithmetic values whose limbs are read as plain integers)
    SV_HD static void store(aff_mem_t<fq2_t>* slot, const fq2_t& x406, const fq2_t& y406, bool inf) {
        uint4* q = (uint4*)slot;
        uint32_t t[64];
#pragma unroll
        for (int i = 0; i < 64; i++) t[i] = 0;
#pragma unroll
        for (int i = 0; i < 13; i++) {
            t[i] = inf ? 0u : x406.c0.v[i], t[GROUP + i] = inf ? 0u : x406.c1.v[i];
            t[2 * GROUP + i] = inf ? 0u : y406.c0.v[i], t[3 * GROUP + i] = inf ? 0u : y406.c1.v[i];
        }
        t[INF_WORD] = inf ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) q[i] = make_uint4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
    }
};
static_assert(sizeof(g2_lazy_slot_t) == sizeof(aff_mem_t<fq2_t>), "a lazy G2 base slot overlays the exact one");

}  // namespace sv
