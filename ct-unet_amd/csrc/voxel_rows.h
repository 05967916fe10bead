// The front end of the volume kernels (morphology, distance, surface, mesh, fill holes, region properties): a lane reads 16
// x-consecutive voxels of a uint8 / int32 / int64 / float32 map and turns them into a 16-bit membership mask.  One routine,
// mask16, and one small functor per membership rule; with them each16 (the values themselves), store_mask16, the way back
// from a mask to 16 bytes of 0 / 1, and the constants every one of these kernels shares.
#pragma once
#include "common.h"

namespace ctu_vox {

// A lane owns 16 voxels of a row and a wave one row, so a row has at most 64 x 16 voxels; the line passes of edt_line.h
// stack a whole line in LDS within the same limit.
constexpr int MAX_SIDE = 1024;
constexpr int NONE_POS = 1 << 20;       // "no such voxel in this row": above every x, and every x - NONE_POS stays an int

inline bool sides_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D <= MAX_SIDE && H <= MAX_SIDE && W <= MAX_SIDE;
}

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ membership rules
// foreground of a label map: == label, or nonzero
struct Foreground {
    int has_label;
    long long label;
    __device__ __forceinline__ bool operator()(long long v) const { return has_label ? v == label : v != 0; }
};
// class c of a label map (v == c), or channel c of a one-hot tensor (v != 0)
struct InClass {
    int onehot, c;
    __device__ __forceinline__ bool operator()(uint8_t v) const { return onehot ? v != 0 : v == c; }
    __device__ __forceinline__ bool operator()(long long v) const { return onehot ? v != 0 : v == c; }
    __device__ __forceinline__ bool operator()(float v) const { return onehot ? v != 0.f : v == (float)c; }
};
// inside of a surface mesh: the foreground of a mask or label map, above the level in a scalar field
struct Inside {
    Foreground fg;
    float level;
    __device__ __forceinline__ bool operator()(uint8_t v) const { return fg(v); }
    __device__ __forceinline__ bool operator()(long long v) const { return fg(v); }
    __device__ __forceinline__ bool operator()(float v) const { return v > level; }
};

// ------------------------------------------------------------------------------------------------ the reader
// bit u of the result: pred(p[u]) for u < nv <= 16, the rest 0.  16 voxels at a 16-byte aligned p take 16-byte loads
// (one for uint8, four for float32, eight for int64), anything else is read voxel by voxel.
template <class T, class Pred>
__device__ __forceinline__ uint32_t mask16(const T* p, int nv, Pred pred) {
    constexpr int PER = 16 / (int)sizeof(T);        // voxels of one 16-byte load
    typedef T Vec __attribute__((ext_vector_type(PER)));
    uint32_t b = 0;
    if (nv == 16 && ((uintptr_t)p & 15) == 0) {
        if constexpr (sizeof(T) == 1) {             // bytes shifted out of four words: the pack kernels measure 2 % faster
            const uint4 v = *reinterpret_cast<const uint4*>(p);   // than with a vector of 16 bytes (profiles/voxel_rows.md)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 16; ++u) b |= (uint32_t)pred((T)(w[u >> 2] >> (8 * (u & 3)))) << u;
        } else {
#pragma unroll
            for (int q = 0; q < 16 / PER; ++q) {
                const Vec v = reinterpret_cast<const Vec*>(p)[q];
#pragma unroll
                for (int u = 0; u < PER; ++u) b |= (uint32_t)pred(v[u]) << (q * PER + u);
            }
        }
    } else {
        for (int u = 0; u < nv; ++u) b |= (uint32_t)pred(p[u]) << u;
    }
    return b;
}

// the values themselves, for the kernels that need more than membership (regionprops.hip): f(u, p[u]) for u < nv <= 16,
// with mask16's loads (int32 takes four).  Fully unrolled, so an f that fills a register array keeps it in registers.
template <class T, class F>
__device__ __forceinline__ void each16(const T* p, int nv, F f) {
    constexpr int PER = 16 / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(PER)));
    if (nv == 16 && ((uintptr_t)p & 15) == 0) {
        if constexpr (sizeof(T) == 1) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 16; ++u) f(u, (T)(w[u >> 2] >> (8 * (u & 3))));
        } else {
#pragma unroll
            for (int q = 0; q < 16 / PER; ++q) {
                const Vec v = reinterpret_cast<const Vec*>(p)[q];
#pragma unroll
                for (int u = 0; u < PER; ++u) f(q * PER + u, v[u]);
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (u < nv) f(u, p[u]);
    }
}

// the way back: bit u of m as the byte p[u] = 0 / 1 for u < nv <= 16, one 16-byte store where all 16 go to an aligned p
__device__ __forceinline__ void store_mask16(uint8_t* p, int nv, uint32_t m) {
    if (nv == 16 && ((uintptr_t)p & 15) == 0) {
        // 4 bits -> 4 bytes of 0 / 1: bit i lands on bit 8 i, no two partial products share a position
        uint4 o;
        o.x = ((m & 0xf) * 0x00204081u) & 0x01010101u;
        o.y = (((m >> 4) & 0xf) * 0x00204081u) & 0x01010101u;
        o.z = (((m >> 8) & 0xf) * 0x00204081u) & 0x01010101u;
        o.w = (((m >> 12) & 0xf) * 0x00204081u) & 0x01010101u;
        *reinterpret_cast<uint4*>(p) = o;
    } else {
        for (int u = 0; u < nv; ++u) p[u] = (m >> u) & 1;
    }
}

}  // namespace ctu_vox
