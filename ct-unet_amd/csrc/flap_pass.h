// What the two hole augmentations (augment.hip: sphere / box / flap; defect.hip: irregular defects) share: the search for
// the k-th bone voxel behind ctu_flap_count's chunk counts, and the pieces of the fused streaming pass around the shape
// test -- the read of a thread's 4 voxels, the salt-and-pepper noise, the writes of the network input and the one-hot
// targets, the advance of the instances' device state.  The rules are pinned in ctunet_amd/transforms.py.
#pragma once
#include "common.h"
#include "philox.h"

namespace ctu_flap {

using namespace ctu_rng;

constexpr int AB = 256;
constexpr int REC = CTU_FLAP_RECORD;

// lo + floor(r (hi - lo) / 2^32): uniform integer in [lo, hi) for hi - lo <= 2^32
__device__ __forceinline__ int64_t draw_int(uint32_t r, int64_t lo, uint64_t span) {
    return lo + (int64_t)(((uint64_t)r * span) >> 32);
}

__device__ __forceinline__ bool bone_at(const void* skull, int u8, int64_t i) {
    return u8 ? static_cast<const uint8_t*>(skull)[i] != 0 : static_cast<const float*>(skull)[i] >= 1.0f;
}

// ------------------------------------------------------------------------------------------- the k-th bone voxel
// A block of AB threads finds it in three steps, with a __syncthreads() of the caller's between them:
//   1. every thread:  segment_counts  (tsum[t] = bone voxels of thread t's run of chunks)
//   2. thread 0:      bone_total, then find_chunk for the k it drew
//   3. wave 0:        scan_chunk
__device__ __forceinline__ void segment_counts(const int32_t* cn, int nchunks, int64_t* tsum) {
    const int per = (nchunks + AB - 1) / AB;
    const int c0 = threadIdx.x * per, c1 = min(nchunks, c0 + per);
    int64_t s = 0;
    for (int c = c0; c < c1; ++c) s += cn[c];
    tsum[threadIdx.x] = s;
}

__device__ __forceinline__ int64_t bone_total(const int64_t* tsum) {
    int64_t total = 0;
    for (int t = 0; t < AB; ++t) total += tsum[t];
    return total;
}

// the thread segment, then the chunk, that holds the k-th bone voxel (k < total); kloc: its rank inside that chunk
__device__ __forceinline__ void find_chunk(const int32_t* cn, int nchunks, const int64_t* tsum, int64_t k, int64_t& chunk,
                                           int64_t& kloc) {
    const int per = (nchunks + AB - 1) / AB;
    int64_t acc = 0;
    int t = 0;
    while (acc + tsum[t] <= k) acc += tsum[t++];
    for (int c = t * per;; ++c) {
        if (acc + cn[c] > k) { chunk = c; kloc = k - acc; break; }
        acc += cn[c];
    }
}

// wave 0 rescans the chunk, 64 voxels per ballot; the lane that holds the voxel stores its flat index in *idx
__device__ __forceinline__ void scan_chunk(const void* skull, int u8, int64_t base, int64_t V, int64_t chunk, int64_t kl,
                                           int64_t* idx) {
    const int lane = threadIdx.x;
    const int64_t e = min(V, (chunk + 1) * CTU_FLAP_CHUNK);
    for (int64_t b = chunk * CTU_FLAP_CHUNK; b < e; b += 64) {
        const int64_t i = b + lane;
        const bool bone = i < e && bone_at(skull, u8, base + i);
        const uint64_t m = __ballot(bone);
        const int pc = __popcll(m);
        if (kl < pc) {
            if (bone && __popcll(m & ((1ull << lane) - 1ull)) == kl) *idx = i;
            break;
        }
        kl -= pc;
    }
}

// ------------------------------------------------------------------------------------------- the streaming pass
// advance the instances' device state (nothing else reads it in the apply launch); params: the noise records
__device__ __forceinline__ void advance_state(int mode, int decay, int N, const int32_t* params, int64_t* hole_seq,
                                              int64_t* noise_seq, float* noise_nd) {
    if (mode & CTU_FLAP_HOLE) hole_seq[0] += N;
    if (mode & CTU_FLAP_NOISE) {
        noise_seq[0] += N;
        if (decay) noise_nd[0] = __int_as_float(params[(int64_t)(N - 1) * REC + 11]);
    }
}

// the skull's 4 voxels from flat index src (x its first column): value = its uint8 cast (truncation on [0, 256))
__device__ __forceinline__ void read_quad(const void* skull, int u8, int vec, int64_t src, int x, int W, float val[4]) {
    if (vec) {
        if (u8) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(skull) + src);
#pragma unroll
            for (int l = 0; l < 4; ++l) val[l] = (float)((w >> (8 * l)) & 0xFFu);
        } else {
            const f32x4 v = *reinterpret_cast<const f32x4*>(static_cast<const float*>(skull) + src);
#pragma unroll
            for (int l = 0; l < 4; ++l) val[l] = truncf(v[l]);
        }
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            val[l] = 0.f;
            if (x + l < W)
                val[l] = u8 ? (float)static_cast<const uint8_t*>(skull)[src + l]
                            : truncf(static_cast<const float*>(skull)[src + l]);
        }
    }
}

// salt and pepper on the 4 voxels of quad c0 = (z H + y) ceil(W / 4) + x / 4 of the sample with noise record rec
__device__ __forceinline__ void salt_pepper(const int32_t* rec, uint32_t c0, uint32_t nk0, uint32_t nk1, float img[4]) {
    const int64_t seq = (int64_t)(((uint64_t)(uint32_t)rec[15] << 32) | (uint32_t)rec[14]);
    const uint4 r1 = philox_seq(c0, 1, seq, nk0, nk1);
    const uint4 r2 = philox_seq(c0, 2, seq, nk0, nk1);
    const float t0 = __int_as_float(rec[12]), t1 = __int_as_float(rec[13]);
    const uint32_t w1[4] = {r1.x, r1.y, r1.z, r1.w}, w2[4] = {r2.x, r2.y, r2.z, r2.w};
#pragma unroll
    for (int l = 0; l < 4; ++l) img[l] = (img[l] != 0.f && !(unif_f32(w1[l]) <= t0)) || unif_f32(w2[l]) <= t1 ? 1.f : 0.f;
}

// the quad's outputs: xo = channel 0 of the sample's input at the quad, fo / po = channel 0 of its full / flap target there
// (either may be null), atlas = the atlas at the quad (null: no second input channel)
__device__ __forceinline__ void write_quad(float* xo, const float* atlas, float* fo, float* po, int64_t V, int vec, int x,
                                           int W, const float img[4], const float bone[4], const float fl[4]) {
    if (vec) {
        *reinterpret_cast<f32x4*>(xo) = f32x4{img[0], img[1], img[2], img[3]};
        if (atlas) *reinterpret_cast<f32x4*>(xo + V) = *reinterpret_cast<const f32x4*>(atlas);
        if (fo) {
            *reinterpret_cast<f32x4*>(fo) = f32x4{1.f - bone[0], 1.f - bone[1], 1.f - bone[2], 1.f - bone[3]};
            *reinterpret_cast<f32x4*>(fo + V) = f32x4{bone[0], bone[1], bone[2], bone[3]};
        }
        if (po) {
            *reinterpret_cast<f32x4*>(po) = f32x4{1.f - fl[0], 1.f - fl[1], 1.f - fl[2], 1.f - fl[3]};
            *reinterpret_cast<f32x4*>(po + V) = f32x4{fl[0], fl[1], fl[2], fl[3]};
        }
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (x + l >= W) break;
            xo[l] = img[l];
            if (atlas) xo[V + l] = atlas[l];
            if (fo) { fo[l] = 1.f - bone[l]; fo[V + l] = bone[l]; }
            if (po) { po[l] = 1.f - fl[l]; po[V + l] = fl[l]; }
        }
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// every output of the pass, and the skull, on the grid of the 16-byte path (4 bytes for a uint8 skull)
inline int quad_vec(const void* skull, int u8, const float* atlas, int W, const float* x, const float* full, const float* flap) {
    return W % 4 == 0 && aligned(skull, u8 ? 4 : 16) && aligned(x, 16) && (!atlas || aligned(atlas, 16)) &&
           (!full || aligned(full, 16)) && (!flap || aligned(flap, 16));
}

inline int check_shape(int N, int D, int H, int W) {
    CTU_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "flap: bad shape %dx%dx%dx%d", N, D, H, W);
    CTU_REQUIRE((int64_t)D * H * W < ((int64_t)1 << 31), "flap: %dx%dx%d voxels per sample (< 2^31 supported)", D, H, W);
    CTU_REQUIRE((int64_t)D * H * ((W + 3) / 4) < ((int64_t)1 << 32), "flap: noise counter overflow");
    return CTU_OK;
}

}  // namespace ctu_flap
