#pragma once
// g1_generator.hip.h - the G1 generator: the seed of the synthetic bases (api.hip, snarkvm_hip_g1_generate_bases_device) and of the host-side test hooks.
#include <string.h>

#include "ec.hip.h"

// G1 generator (g1.rs:219-253), memory Montgomery form, 64-bit limbs
static const uint64_t G1_GEN_X[6] = {1171681672315280277ull, 6528257384425852712ull,  7514971432460253787ull,
                                     2032708395764262463ull, 12876543207309632302ull, 107509843840671767ull};
static const uint64_t G1_GEN_Y[6] = {13572190014569192121ull, 15344828677741220784ull, 17067903700058808083ull,
                                     10342263224753415805ull, 1083990386877464092ull,  21335464879237822ull};
// the generator as an affine point in the exact internal form, converted on the host with the arithmetic the kernels use
static inline g1_aff_t g1_generator() {
    uint32_t xw[12], yw[12];
    memcpy(xw, G1_GEN_X, 48);
    memcpy(yw, G1_GEN_Y, 48);
    return {fq_t::unpack(xw).from_mem_mont(), fq_t::unpack(yw).from_mem_mont()};
}
