// Trilinear interpolation and the label vote of label_linear, shared by resample.hip and affine.hip.
//   lerp(p, q, w) = p + w (q - p) in float32, every operation rounded on its own; tri: four lerps along x, two along y, one
//   along z over corners ordered c[4 dz + 2 dy + dx].  The pragma below keeps that so whatever the including file compiles
//   under: float code inlined from a header built under another contraction setting was once fused into FMAs there.
//   label_vote evaluates only the classes present among the 8 corner labels, in increasing order, and keeps the first
//   strict maximum starting from (class 0, score 0): an absent class scores exactly 0 and no score is negative, so this is
//   the smallest class of the largest score over all K classes.  A label outside [0, K) belongs to no class; the test is
//   made in the label's own unsigned type, so an int64 label is never truncated before it is compared.
#pragma once
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

namespace ctu_tri {

constexpr int NEAREST = CTU_RESAMPLE_NEAREST, LINEAR = CTU_RESAMPLE_LINEAR, LABEL = CTU_RESAMPLE_LABEL_LINEAR;
constexpr int NO_CLASS = 31;                    // a label >= K: belongs to no class

// the output type: float32 for linear, the input's own otherwise
template <class T, int MODE> struct OutOf { typedef T type; };
template <class T> struct OutOf<T, LINEAR> { typedef float type; };

// plain operators: the __f*_rn functions of the HIP headers are compiled under the headers' own contraction setting
__device__ __forceinline__ float lerp(float p, float q, float w) {
    const float d = q - p;
    const float t = w * d;
    return p + t;
}

__device__ __forceinline__ float tri(const float c[8], float wx, float wy, float wz) {
    const float c00 = lerp(c[0], c[1], wx), c01 = lerp(c[2], c[3], wx), c10 = lerp(c[4], c[5], wx), c11 = lerp(c[6], c[7], wx);
    return lerp(lerp(c00, c01, wy), lerp(c10, c11, wy), wz);
}

// the class of the largest interpolated indicator among the corner labels v, K in 2..16
template <class T>
__device__ __forceinline__ int label_vote(const T (&v)[8], int K, float wx, float wy, float wz) {
    typedef typename std::make_unsigned<T>::type UT;
    int l[8];
    uint32_t present = 0;
    bool same = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        l[j] = (UT)v[j] < (UT)K ? (int)v[j] : NO_CLASS;
        same = same && l[j] == l[0];
        if (l[j] != NO_CLASS) present |= 1u << l[j];
    }
    int best = 0;
    if (same) {                                    // one class scores exactly 1 (or none does), the rest 0
        best = l[0] == NO_CLASS ? 0 : l[0];
    } else {
        float bs = 0.f;
        while (present) {
            const int c = __ffs(present) - 1;
            present &= present - 1;
            float ind[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) ind[j] = l[j] == c ? 1.f : 0.f;
            const float s = tri(ind, wx, wy, wz);
            if (s > bs) {
                bs = s;
                best = c;
            }
        }
    }
    return best;
}

}  // namespace ctu_tri
