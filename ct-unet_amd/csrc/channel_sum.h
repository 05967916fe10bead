// Block bodies of the deterministic per-channel sum (ctu_channel_sum, elementwise.hip), shared with the fused up-convolution's
// projection (upconv_fused.hip), which runs them inside its own launches next to the face sums and V.
#pragma once
#include "common.h"

constexpr int CSUM_BLOCK = 256;      // threads per block of both stages

// Stage 1, block `bid` of `nblocks`: its grid-stride share of the voxels -> partials[bid][cp].  red: CSUM_BLOCK * 4 floats of LDS.
template <class T>
__device__ __forceinline__ void channel_sum_partial_block(const T* __restrict__ x, int cs, int cp, int64_t nvox,
                                                          float* __restrict__ partials, int bid, int nblocks, float* red) {
    const int nq = cp >> 2;
    const int tpv = CSUM_BLOCK / nq;
    const int qd = threadIdx.x % nq, vl = threadIdx.x / nq;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vl < tpv)
        for (int64_t v = (int64_t)bid * tpv + vl; v < nvox; v += (int64_t)nblocks * tpv) {
            const float4 t = ld4<T>(x + v * cs + qd * 4);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
    float* r = &red[threadIdx.x * 4];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    __syncthreads();
    if (threadIdx.x < cp) {
        const int c = threadIdx.x, q = c >> 2, j = c & 3;
        float s = 0.f;
        for (int l = 0; l < tpv; ++l) s += red[(l * nq + q) * 4 + j];
        partials[(size_t)bid * cp + c] = s;
    }
}

// Stage 2, one block per channel c: fixed-order fp64 tree over the nb partial rows -> deterministic.  r: CSUM_BLOCK doubles of
// LDS.  Every thread returns the sum (the tree's last barrier has passed).
__device__ __forceinline__ float channel_sum_final_block(const float* __restrict__ partials, int nb, int cp, int c, double* r) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += CSUM_BLOCK) s += (double)partials[(size_t)b * cp + c];
    r[threadIdx.x] = s;
    __syncthreads();
    for (int o = CSUM_BLOCK / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
        __syncthreads();
    }
    return (float)r[0];
}
