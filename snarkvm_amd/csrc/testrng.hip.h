#pragma once
// testrng.hip.h - what the host-side test hooks (api_selftest.hip, api_tailtest.hip) share: the SplitMix64 stream the hooks draw their cases from and the
// reader of a pool of G2 points (the G1 generator: g1_generator.hip.h).  Seeds and the order of draws are part of the hooks' contract: the host
// tests pin return codes that depend on them.
#include <vector>

#include "ec.hip.h"

// SplitMix64: next() is the stream's next value
struct splitmix64_t {
    uint64_t seed;
    uint64_t operator()() {
        seed += 0x9E3779B97F4A7C15ull;
        uint64_t z = seed;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

// npoints G2 affine points from 200-byte records (x, y as raw words; the hooks' callers pass finite points)
static inline std::vector<aff_t<fq2_t>> g2_pool_from_records(const void* points, size_t npoints) {
    std::vector<aff_t<fq2_t>> pool;
    for (size_t i = 0; i < npoints; i++) {
        const uint32_t* src = (const uint32_t*)((const uint8_t*)points + 200 * i);
        pool.push_back({fq2_t::from_raw_words(src), fq2_t::from_raw_words(src + 24)});
    }
    return pool;
}
