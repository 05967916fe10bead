// Philox4x32-10 (Salmon et al., SC'11) for the on-device augmentations (augment.hip, spatial.hip): counter-based, so a draw
// depends on (counter, key) alone and a replayed graph that advances its DEVICE sample counter draws fresh numbers.
#pragma once
#include "common.h"

namespace ctu_rng {

// counter c, key (k0, k1)
__device__ __forceinline__ uint4 philox(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// draw c0 of stream `stream` of sample `seq`
__device__ __forceinline__ uint4 philox_seq(uint32_t c0, uint32_t stream, int64_t seq, uint32_t k0, uint32_t k1) {
    return philox(make_uint4(c0, stream, (uint32_t)(uint64_t)seq, (uint32_t)((uint64_t)seq >> 32)), k0, k1);
}

// u = (r >> 8) 2^-24 in [0, 1), exact in either type; the rules that use them are written in that type
__device__ __forceinline__ float unif_f32(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-08f; }
__device__ __forceinline__ double unif_f64(uint32_t r) { return (double)(r >> 8) * 5.9604644775390625e-08; }

}  // namespace ctu_rng
