// The chamfer sample shared by registration.hip and ffd.hip: a world position against a float32 distance field, in float64
// with every operation rounded on its own (rule: ctunet_amd/registration.py, "Sample").  The pragma below keeps that whatever
// the including file compiles under.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace ctu_field {

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }

__device__ __forceinline__ double lerp(double p, double q, double w) {
    const double d = q - p;
    const double t = w * d;
    return p + t;
}

// q_a = ((m_a0 p_0 + m_a1 p_1) + m_a2 p_2) + m_a3
__device__ __forceinline__ void apply(const double* M, const double p[3], double q[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((M[4 * a] * p[0] + M[4 * a + 1] * p[1]) + M[4 * a + 2] * p[2]) + M[4 * a + 3];
}

struct FieldGrid {
    int n[3];
    double sp[3], org[3];
};

// The rigid rule's sample at the world position q: true iff q is inside the grid and v <= bound, then with the trilinear
// value v and its gradient over the spacing g.  Every read sits behind the inside test (NaN fails it).
__device__ __forceinline__ bool sample_inlier(const FieldGrid& a, const float* __restrict__ field, const double q[3], double bound,
                                              double& v, double g[3]) {
    double u[3];
    bool inside = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u[r] = (q[r] - a.org[r]) / a.sp[r];
        inside = inside && u[r] >= 0.0 && u[r] <= (double)(a.n[r] - 1);
    }
    if (!inside) return false;
    int i0[3];
    double f[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fl = fmin(floor(u[r]), (double)(a.n[r] - 2));
        i0[r] = (int)fl;                                                       // 0 .. n - 2
        f[r] = u[r] - fl;
    }
    const int H = a.n[1], W = a.n[2];
    const float* c0 = field + ((int64_t)i0[0] * H + i0[1]) * W + i0[2];
    const float* c1 = c0 + (int64_t)H * W;
    const double c000 = c0[0], c001 = c0[1], c010 = c0[W], c011 = c0[W + 1];
    const double c100 = c1[0], c101 = c1[1], c110 = c1[W], c111 = c1[W + 1];
    const double c00 = lerp(c000, c001, f[2]), c01 = lerp(c010, c011, f[2]);
    const double c10 = lerp(c100, c101, f[2]), c11 = lerp(c110, c111, f[2]);
    const double cz0 = lerp(c00, c01, f[1]), cz1 = lerp(c10, c11, f[1]);
    v = lerp(cz0, cz1, f[0]);
    if (!(v <= bound)) return false;
    g[0] = (cz1 - cz0) / a.sp[0];
    g[1] = lerp(c01 - c00, c11 - c10, f[0]) / a.sp[1];
    g[2] = lerp(lerp(c001 - c000, c011 - c010, f[1]), lerp(c101 - c100, c111 - c110, f[1]), f[0]) / a.sp[2];
    return true;
}

}  // namespace ctu_field
