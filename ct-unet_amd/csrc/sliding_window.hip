// Sliding-window inference over whole CT volumes, gfx950: weighted accumulation of a batch of patch predictions into
// whole-volume accumulators, and the finalize pass that turns them into probabilities and first-argmax labels.
// HBM-bound streaming: per batch every voxel of the batch's bounding box reads and writes its K+1 accumulators once and
// reads the patch values that cover it; no atomics (gather form, fixed tile order => bitwise reproducible).
//
// Replaces: the host loop a user of the reference would write around Model.forward_pass in eval mode
//           (ctunet/pytorch/Model.py:342-352); the reference itself resizes whole volumes to the network size instead
//           (ctunet/pytorch/datasets.py:89-112,195-235).
#include "common.h"

namespace {

constexpr int SB = 256;
constexpr int MAX_BATCH = 64;

__device__ __forceinline__ f32x4 load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p);
    f32x4 r;
    r.x = p[0]; r.y = p[1]; r.z = p[2]; r.w = p[3];
    return r;
}

// One thread = 4 consecutive x voxels (xq-th quad of the box row) of the batch's bounding box
//   box = [oz, oz+bz) x [oy, oy+by) x [ox, ox+bx), origin read from device memory (ox a multiple of 4), extents fixed at
//   launch (the largest box of any batch of the volume, so one captured launch serves every batch).
// For each valid patch p of the batch, in order: w = max(wz[lz] * wy[ly] * wx[lx], wmin), num[k] += w * y_p[k], wsum += w.
// Lanes outside the volume are computed but never stored; a quad no patch covers is not stored at all.  wsum NULL: only
// num is accumulated (the second head of a two-output net shares the first head's weight sum).
template <int K>
__global__ void __launch_bounds__(SB) window_accumulate_kernel(
    const float* __restrict__ patches, const int32_t* __restrict__ coords, const int32_t* __restrict__ valid,
    const int32_t* __restrict__ box, int B, int D, int H, int W, int pd, int ph, int pw, const float* __restrict__ wz,
    const float* __restrict__ wy, const float* __restrict__ wx, float wmin, int bz, int by, int bx,
    float* __restrict__ num, float* __restrict__ wsum) {
    const int oz = box[0], oy = box[1], ox = box[2];
    const int nq = bx >> 2;
    const int64_t total = (int64_t)bz * by * nq;
    const int64_t V = (int64_t)D * H * W;
    const int64_t pv = (int64_t)pd * ph * pw;
    const bool wvec = (W & 3) == 0 && (ox & 3) == 0;   // num / wsum quads 16-byte aligned
    for (int64_t g = (int64_t)blockIdx.x * SB + threadIdx.x; g < total; g += (int64_t)gridDim.x * SB) {
        const int xq = (int)(g % nq);
        const int y = oy + (int)((g / nq) % by);
        const int z = oz + (int)(g / ((int64_t)nq * by));
        const int x = ox + 4 * xq;
        if (z >= D || y >= H || x >= W) continue;
        const int64_t v = ((int64_t)z * H + y) * W + x;
        const bool full = wvec && x + 3 < W;      // all four lanes inside the row and aligned
        f32x4 acc[K];
        f32x4 ws;
        bool loaded = false;
        for (int p = 0; p < B; ++p) {
            if (!valid[p]) continue;
            const int lz = z - coords[3 * p], ly = y - coords[3 * p + 1], lx0 = x - coords[3 * p + 2];
            if (lz < 0 || lz >= pd || ly < 0 || ly >= ph || lx0 + 3 < 0 || lx0 >= pw) continue;
            if (!loaded) {
                if (full) {
                    ws = wsum ? load4(wsum + v, true) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = load4(num + (int64_t)k * V + v, true);
                } else {
                    for (int l = 0; l < 4; ++l) {
                        const bool in = x + l < W;
                        ws[l] = in && wsum ? wsum[v + l] : 0.f;
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k][l] = in ? num[(int64_t)k * V + v + l] : 0.f;
                    }
                }
                loaded = true;
            }
            const float wzy = wz[lz] * wy[ly];
            const float* yp = patches + (int64_t)p * K * pv + ((int64_t)lz * ph + ly) * pw;
            if (lx0 >= 0 && lx0 + 3 < pw && (lx0 & 3) == 0) {       // (pw is a multiple of 16: 16-byte aligned rows)
                const f32x4 gx = load4(wx + lx0, true);
                f32x4 w;
#pragma unroll
                for (int l = 0; l < 4; ++l) w[l] = fmaxf(wzy * gx[l], wmin);
                ws += w;
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] += w * load4(yp + (int64_t)k * pv + lx0, true);
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const int lx = lx0 + l;
                    if (lx < 0 || lx >= pw) continue;
                    const float w = fmaxf(wzy * wx[lx], wmin);
                    ws[l] += w;
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k][l] += w * yp[(int64_t)k * pv + lx];
                }
            }
        }
        if (!loaded) continue;
        if (full) {
            if (wsum) *reinterpret_cast<f32x4*>(wsum + v) = ws;
#pragma unroll
            for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(num + (int64_t)k * V + v) = acc[k];
        } else {
            for (int l = 0; l < 4; ++l) {
                if (x + l >= W) break;
                if (wsum) wsum[v + l] = ws[l];
#pragma unroll
                for (int k = 0; k < K; ++k) num[(int64_t)k * V + v + l] = acc[k][l];
            }
        }
    }
}

// probs[k][v] = num[k][v] / wsum[v] (0 where wsum == 0); labels[v] = first k of the maximum probability.
// probs may alias num (in place).  VEC: V % 4 == 0, four voxels per thread with 16-byte accesses.
template <int K, bool VEC>
__global__ void __launch_bounds__(SB) window_finalize_kernel(const float* num, const float* __restrict__ wsum, int64_t V,
                                                             float* probs, uint8_t* __restrict__ labels) {
    constexpr int NV = VEC ? 4 : 1;
    const int64_t groups = V / NV;
    for (int64_t g = (int64_t)blockIdx.x * SB + threadIdx.x; g < groups; g += (int64_t)gridDim.x * SB) {
        const int64_t v = g * NV;
        float s[NV], q[K][NV];
        if constexpr (VEC) {
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(wsum + v);
#pragma unroll
            for (int l = 0; l < 4; ++l) s[l] = s4[l];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f32x4 n4 = *reinterpret_cast<const f32x4*>(num + (int64_t)k * V + v);
#pragma unroll
                for (int l = 0; l < 4; ++l) q[k][l] = n4[l];
            }
        } else {
            s[0] = wsum[v];
#pragma unroll
            for (int k = 0; k < K; ++k) q[k][0] = num[(int64_t)k * V + v];
        }
        uint8_t lab[NV];
#pragma unroll
        for (int l = 0; l < NV; ++l) {
            float best = 0.f;
            int bi = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float r = s[l] > 0.f ? q[k][l] / s[l] : 0.f;
                q[k][l] = r;
                if (k == 0 || r > best) { best = r; bi = k; }
            }
            lab[l] = (uint8_t)bi;
        }
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                f32x4 o;
#pragma unroll
                for (int l = 0; l < 4; ++l) o[l] = q[k][l];
                *reinterpret_cast<f32x4*>(probs + (int64_t)k * V + v) = o;
            }
            if (labels)
                *reinterpret_cast<uint32_t*>(labels + v) =
                    (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) probs[(int64_t)k * V + v] = q[k][0];
            if (labels) labels[v] = lab[0];
        }
    }
}

unsigned stream_grid(int64_t work) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(work, SB), 2048)); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int ctu_window_accumulate(const float* patches, const int32_t* coords, const int32_t* valid, const int32_t* box,
                                     int B, int K, int D, int H, int W, int pd, int ph, int pw, const float* wz,
                                     const float* wy, const float* wx, float wmin, int bz, int by, int bx, float* num,
                                     float* wsum, void* stream) {
    CTU_REQUIRE(patches && coords && valid && box && wz && wy && wx && num, "window_accumulate: null pointer");
    CTU_REQUIRE(B > 0 && B <= MAX_BATCH, "window_accumulate: batch %d outside [1, %d]", B, MAX_BATCH);
    CTU_REQUIRE(K >= 1 && K <= 4, "window_accumulate: %d channels (1..4 supported)", K);
    CTU_REQUIRE(D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "window_accumulate: bad shape");
    CTU_REQUIRE(pw % 4 == 0, "window_accumulate: patch width %d not a multiple of 4", pw);
    CTU_REQUIRE(bz > 0 && by > 0 && bx > 0 && bx % 4 == 0, "window_accumulate: box extent %dx%dx%d (x a multiple of 4)", bz, by, bx);
    CTU_REQUIRE(aligned16(patches) && aligned16(wx) && aligned16(num) && (!wsum || aligned16(wsum)),
                "window_accumulate: patches, wx, num and wsum must be 16-byte aligned");
    const unsigned grid = stream_grid((int64_t)bz * by * (bx / 4));
    hipStream_t st = (hipStream_t)stream;
#define CTU_WA(KK)                                                                                                     \
    window_accumulate_kernel<KK><<<grid, SB, 0, st>>>(patches, coords, valid, box, B, D, H, W, pd, ph, pw, wz, wy, wx, \
                                                      wmin, bz, by, bx, num, wsum)
    switch (K) {
        case 1: CTU_WA(1); break;
        case 2: CTU_WA(2); break;
        case 3: CTU_WA(3); break;
        default: CTU_WA(4); break;
    }
#undef CTU_WA
    CTU_CHECK_LAUNCH("window_accumulate");
    return CTU_OK;
}

extern "C" int ctu_window_finalize(const float* num, const float* wsum, int K, int64_t V, float* probs, uint8_t* labels,
                                   void* stream) {
    CTU_REQUIRE(num && wsum && probs, "window_finalize: null pointer");
    CTU_REQUIRE(K >= 1 && K <= 4 && V > 0, "window_finalize: bad shape K=%d", K);
    const bool vec = V % 4 == 0 && aligned16(num) && aligned16(wsum) && aligned16(probs) && (!labels || ((uintptr_t)labels & 3) == 0);
    const unsigned grid = stream_grid(vec ? V / 4 : V);
    hipStream_t st = (hipStream_t)stream;
#define CTU_WF(KK)                                                                                                  \
    if (vec) window_finalize_kernel<KK, true><<<grid, SB, 0, st>>>(num, wsum, V, probs, labels);                    \
    else window_finalize_kernel<KK, false><<<grid, SB, 0, st>>>(num, wsum, V, probs, labels)
    switch (K) {
        case 1: CTU_WF(1); break;
        case 2: CTU_WF(2); break;
        case 3: CTU_WF(3); break;
        default: CTU_WF(4); break;
    }
#undef CTU_WF
    CTU_CHECK_LAUNCH("window_finalize");
    return CTU_OK;
}
