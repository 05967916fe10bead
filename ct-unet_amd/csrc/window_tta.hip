// Test-time mirroring, ensembles and per-voxel uncertainty for sliding-window inference, gfx950: the three kernels of
// sliding_window.hip / volume.hip with a flip word and optional moment accumulators.
//   extract:    patch windows of the volume, mirrored on the way in, 16-byte row accesses where the volume allows
//   accumulate: window_accumulate_kernel reading each patch at the mirrored local index (the un-mirroring of the net's
//               output), optionally also S2 += w y^2 and SH += w h(y)
//   finalize:   probabilities and labels as window_finalize_kernel, plus variance, entropy and mutual information
// The flip word lives in device memory (bit 0 = x, 1 = y, 2 = z; only the low 3 bits count), so one captured launch
// serves every mirrored pass.  HBM-bound streaming, gather form, no atomics: bitwise reproducible.  The rule is pinned in
// the module docstring of ctunet_amd/inference.py and restated in tests/tta_ref.py.
//
// Replaces: nothing in the reference, which predicts one resized volume once (ctunet/pytorch/Model.py:342-352).
#include "common.h"

namespace {

constexpr int SB = 256;
constexpr int MAX_BATCH = 64;

__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 reverse4(f32x4 v) { return f32x4{v.w, v.z, v.y, v.x}; }

// out[p][c][i][j][k] = x_p[c][i^][j^][k^], x_p the zero-padded window of the volume at coords[p], a^ = P_a-1-a on the
// mirrored axes.  One thread = one 16-byte quad of an output row (pw a multiple of 4); blockIdx.y = p * C + c.  The
// source quad of an x-mirrored row starts at pw-4-k and has its lanes reversed.  It is one 16-byte load when W is a
// multiple of 4, vol is 16-byte aligned, the quad's first voxel sits at a multiple of 4 and the quad lies inside the row;
// otherwise four bounds-checked scalar loads.
__global__ void __launch_bounds__(SB) extract_flip_kernel(const float* __restrict__ vol, const int32_t* __restrict__ coords,
                                                          const int32_t* __restrict__ flip, int C, int D, int H, int W,
                                                          int pd, int ph, int pw, float* __restrict__ out) {
    const int f = flip[0];
    const bool fx = f & 1, fy = f & 2, fz = f & 4;
    const int p = blockIdx.y / C, c = blockIdx.y % C;
    const int z0 = coords[3 * p], y0 = coords[3 * p + 1], x0 = coords[3 * p + 2];
    const unsigned nq = (unsigned)pw >> 2;
    const unsigned total = (unsigned)pd * ph * nq;           // (host: pd * ph * pw < 2^31)
    const bool wvec = (W & 3) == 0 && ((uintptr_t)vol & 15) == 0;      // rows of the volume 16-byte aligned
    const float* vc = vol + (int64_t)c * D * H * W;
    float* oc = out + (int64_t)blockIdx.y * pd * ph * pw;
    for (unsigned q = blockIdx.x * SB + threadIdx.x; q < total; q += gridDim.x * SB) {
        const unsigned row = q / nq;
        const int k = (int)(q - row * nq) << 2;
        const int j = (int)(row % ph), i = (int)(row / ph);
        const int gz = z0 + (fz ? pd - 1 - i : i), gy = y0 + (fy ? ph - 1 - j : j);
        const int gx = x0 + (fx ? pw - 4 - k : k);
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (gz >= 0 && gz < D && gy >= 0 && gy < H) {
            const float* src = vc + ((int64_t)gz * H + gy) * W;
            if (wvec && (gx & 3) == 0 && gx >= 0 && gx + 3 < W) {
                r = load4(src + gx);
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l)
                    if (gx + l >= 0 && gx + l < W) r[l] = src[gx + l];
            }
        }
        *reinterpret_cast<f32x4*>(oc + (int64_t)q * 4) = fx ? reverse4(r) : r;
    }
}

// h(y) = -sum_k q_k ln q_k / ln K, q_k = max(y_k, 0) / sum_j max(y_j, 0); 0 for a zero sum, 0 ln 0 = 0.  inv_lnk = 1 / ln K.
template <int K>
__device__ __forceinline__ float entropy_of(const float (&y)[K], float inv_lnk) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) s += fmaxf(y[k], 0.f);
    if (!(s > 0.f)) return 0.f;
    float h = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float q = fmaxf(y[k], 0.f) / s;
        if (q > 0.f) h -= q * logf(q);
    }
    return h * inv_lnk;
}

// window_accumulate_kernel (sliding_window.hip) with the patch read at the mirrored local index: one thread = 4
// consecutive x voxels of the batch's bounding box; for each valid patch p in order
//   w = max(wz[lz] * wy[ly] * wx[lx], wmin) at the UN-mirrored local position, y = patches[p][.][lz^][ly^][lx^],
//   num[k] += w y_k, wsum += w, and with SQ: sq[k] += w (y_k y_k), with SH: sh += w h(y).
// The x-mirrored fast path loads the aligned quad at pw-4-lx0 and reverses its lanes.  wsum may be NULL (second head).
template <int K, bool SQ, bool SH>
__global__ void __launch_bounds__(SB) accumulate_flip_kernel(
    const float* __restrict__ patches, const int32_t* __restrict__ coords, const int32_t* __restrict__ valid,
    const int32_t* __restrict__ box, const int32_t* __restrict__ flip, int B, int D, int H, int W, int pd, int ph, int pw,
    const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx, float wmin, int bz, int by,
    int bx, float* __restrict__ num, float* __restrict__ wsum, float* __restrict__ sq, float* __restrict__ sh,
    float inv_lnk) {
    const int oz = box[0], oy = box[1], ox = box[2];
    const int f = flip[0];
    const bool fx = f & 1, fy = f & 2, fz = f & 4;
    const int nq = bx >> 2;
    const int64_t total = (int64_t)bz * by * nq;
    const int64_t V = (int64_t)D * H * W;
    const int64_t pv = (int64_t)pd * ph * pw;
    const bool wvec = (W & 3) == 0 && (ox & 3) == 0;   // accumulator quads 16-byte aligned
    for (int64_t g = (int64_t)blockIdx.x * SB + threadIdx.x; g < total; g += (int64_t)gridDim.x * SB) {
        const int xq = (int)(g % nq);
        const int y = oy + (int)((g / nq) % by);
        const int z = oz + (int)(g / ((int64_t)nq * by));
        const int x = ox + 4 * xq;
        if (z >= D || y >= H || x >= W) continue;
        const int64_t v = ((int64_t)z * H + y) * W + x;
        const bool full = wvec && x + 3 < W;      // all four lanes inside the row and aligned
        f32x4 acc[K], asq[SQ ? K : 1];
        f32x4 ws, ah;
        bool loaded = false;
        for (int p = 0; p < B; ++p) {
            if (!valid[p]) continue;
            const int lz = z - coords[3 * p], ly = y - coords[3 * p + 1], lx0 = x - coords[3 * p + 2];
            if (lz < 0 || lz >= pd || ly < 0 || ly >= ph || lx0 + 3 < 0 || lx0 >= pw) continue;
            if (!loaded) {
                if (full) {
                    ws = wsum ? load4(wsum + v) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] = load4(num + (int64_t)k * V + v);
                    if constexpr (SQ) {
#pragma unroll
                        for (int k = 0; k < K; ++k) asq[k] = load4(sq + (int64_t)k * V + v);
                    }
                    if constexpr (SH) ah = load4(sh + v);
                } else {
                    for (int l = 0; l < 4; ++l) {
                        const bool in = x + l < W;
                        ws[l] = in && wsum ? wsum[v + l] : 0.f;
#pragma unroll
                        for (int k = 0; k < K; ++k) acc[k][l] = in ? num[(int64_t)k * V + v + l] : 0.f;
                        if constexpr (SQ) {
#pragma unroll
                            for (int k = 0; k < K; ++k) asq[k][l] = in ? sq[(int64_t)k * V + v + l] : 0.f;
                        }
                        if constexpr (SH) ah[l] = in ? sh[v + l] : 0.f;
                    }
                }
                loaded = true;
            }
            const float wzy = wz[lz] * wy[ly];
            const int mz = fz ? pd - 1 - lz : lz, my = fy ? ph - 1 - ly : ly;
            const float* yp = patches + (int64_t)p * K * pv + ((int64_t)mz * ph + my) * pw;
            if (lx0 >= 0 && lx0 + 3 < pw && (lx0 & 3) == 0) {       // (pw is a multiple of 4: 16-byte aligned rows)
                const f32x4 gx = load4(wx + lx0);
                const int mx0 = fx ? pw - 4 - lx0 : lx0;
                f32x4 w, yv[K];
#pragma unroll
                for (int l = 0; l < 4; ++l) w[l] = fmaxf(wzy * gx[l], wmin);
                ws += w;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const f32x4 t = load4(yp + (int64_t)k * pv + mx0);
                    yv[k] = fx ? reverse4(t) : t;
                    acc[k] += w * yv[k];
                    if constexpr (SQ) asq[k] += w * (yv[k] * yv[k]);
                }
                if constexpr (SH) {
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        float yl[K];
#pragma unroll
                        for (int k = 0; k < K; ++k) yl[k] = yv[k][l];
                        ah[l] += w[l] * entropy_of<K>(yl, inv_lnk);
                    }
                }
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const int lx = lx0 + l;
                    if (lx < 0 || lx >= pw) continue;
                    const float w = fmaxf(wzy * wx[lx], wmin);
                    const int mx = fx ? pw - 1 - lx : lx;
                    ws[l] += w;
                    float yl[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        yl[k] = yp[(int64_t)k * pv + mx];
                        acc[k][l] += w * yl[k];
                        if constexpr (SQ) asq[k][l] += w * (yl[k] * yl[k]);
                    }
                    if constexpr (SH) ah[l] += w * entropy_of<K>(yl, inv_lnk);
                }
            }
        }
        if (!loaded) continue;
        if (full) {
            if (wsum) *reinterpret_cast<f32x4*>(wsum + v) = ws;
#pragma unroll
            for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(num + (int64_t)k * V + v) = acc[k];
            if constexpr (SQ) {
#pragma unroll
                for (int k = 0; k < K; ++k) *reinterpret_cast<f32x4*>(sq + (int64_t)k * V + v) = asq[k];
            }
            if constexpr (SH) *reinterpret_cast<f32x4*>(sh + v) = ah;
        } else {
            for (int l = 0; l < 4; ++l) {
                if (x + l >= W) break;
                if (wsum) wsum[v + l] = ws[l];
#pragma unroll
                for (int k = 0; k < K; ++k) num[(int64_t)k * V + v + l] = acc[k][l];
                if constexpr (SQ) {
#pragma unroll
                    for (int k = 0; k < K; ++k) sq[(int64_t)k * V + v + l] = asq[k][l];
                }
                if constexpr (SH) sh[v + l] = ah[l];
            }
        }
    }
}

// window_finalize_kernel plus the statistics, each written only where its pointer is non-NULL:
//   probs_k = num_k / wsum (0 where wsum == 0), labels = first argmax,
//   var_k = max(sq_k / wsum - probs_k^2, 0), ent = h(probs), mi = max(ent - sh / wsum, 0); all 0 where wsum == 0.
// probs may alias num and var may alias sq (each thread reads its voxels before it writes them).
template <int K, bool VEC>
__global__ void __launch_bounds__(SB) finalize_stats_kernel(const float* num, const float* __restrict__ wsum, const float* sq,
                                                            const float* __restrict__ sh, int64_t V, float* probs,
                                                            uint8_t* __restrict__ labels, float* var,
                                                            float* __restrict__ ent, float* __restrict__ mi, float inv_lnk) {
    constexpr int NV = VEC ? 4 : 1;
    const int64_t groups = V / NV;
    for (int64_t g = (int64_t)blockIdx.x * SB + threadIdx.x; g < groups; g += (int64_t)gridDim.x * SB) {
        const int64_t v = g * NV;
        float s[NV], q[K][NV], m2[K][NV], hs[NV];
        auto rd = [&](const float* src, float* dst) {
            if constexpr (VEC) {
                const f32x4 t = load4(src);
#pragma unroll
                for (int l = 0; l < 4; ++l) dst[l] = t[l];
            } else {
                dst[0] = src[0];
            }
        };
        auto wr = [&](float* dst, const float* src) {
            if constexpr (VEC) {
                *reinterpret_cast<f32x4*>(dst) = f32x4{src[0], src[1], src[2], src[3]};
            } else {
                dst[0] = src[0];
            }
        };
        rd(wsum + v, s);
#pragma unroll
        for (int k = 0; k < K; ++k) rd(num + (int64_t)k * V + v, q[k]);
        if (var) {
#pragma unroll
            for (int k = 0; k < K; ++k) rd(sq + (int64_t)k * V + v, m2[k]);
        }
        if (mi) rd(sh + v, hs);
        uint8_t lab[NV];
        float e[NV], mo[NV];
#pragma unroll
        for (int l = 0; l < NV; ++l) {
            const bool cov = s[l] > 0.f;
            float best = 0.f;
            int bi = 0;
            float pk[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float r = cov ? q[k][l] / s[l] : 0.f;
                q[k][l] = r;
                pk[k] = r;
                if (k == 0 || r > best) { best = r; bi = k; }
                if (var) m2[k][l] = cov ? fmaxf(m2[k][l] / s[l] - r * r, 0.f) : 0.f;
            }
            lab[l] = (uint8_t)bi;
            e[l] = (ent || mi) ? entropy_of<K>(pk, inv_lnk) : 0.f;
            mo[l] = (mi && cov) ? fmaxf(e[l] - hs[l] / s[l], 0.f) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) wr(probs + (int64_t)k * V + v, q[k]);
        if (var) {
#pragma unroll
            for (int k = 0; k < K; ++k) wr(var + (int64_t)k * V + v, m2[k]);
        }
        if (ent) wr(ent + v, e);
        if (mi) wr(mi + v, mo);
        if (labels) {
            if constexpr (VEC)
                *reinterpret_cast<uint32_t*>(labels + v) =
                    (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
            else
                labels[v] = lab[0];
        }
    }
}

unsigned stream_grid(int64_t work) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(work, SB), 2048)); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

float inv_ln(int K) { return K > 1 ? (float)(1.0 / log((double)K)) : 0.f; }

}  // namespace

extern "C" int ctu_extract_patches_flip(const float* vol, const int32_t* coords, const int32_t* flip, int P, int C, int D,
                                        int H, int W, int pd, int ph, int pw, float* out, void* stream) {
    CTU_REQUIRE(vol && coords && flip && out, "extract_patches_flip: null pointer");
    CTU_REQUIRE(P > 0 && C > 0 && D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "extract_patches_flip: bad shape");
    CTU_REQUIRE(pw % 4 == 0, "extract_patches_flip: patch width %d not a multiple of 4", pw);
    CTU_REQUIRE((int64_t)pd * ph * pw < ((int64_t)1 << 31), "extract_patches_flip: patch %dx%dx%d too large", pd, ph, pw);
    CTU_REQUIRE((int64_t)P * C <= 65535, "extract_patches_flip: %d patches x %d channels above 65535", P, C);
    // (vol at any float address, e.g. a view into a stack of odd-sized volumes: the kernel then reads it with scalar loads)
    CTU_REQUIRE(aligned16(out), "extract_patches_flip: out must be 16-byte aligned");
    const int64_t quads = (int64_t)pd * ph * (pw / 4);
    // enough blocks per (patch, channel) to fill the chip at any P * C, at most 2048 in all
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(quads, SB), ceil_div64(2048, (int64_t)P * C)));
    extract_flip_kernel<<<dim3(gx, (unsigned)(P * C)), SB, 0, (hipStream_t)stream>>>(vol, coords, flip, C, D, H, W, pd, ph, pw,
                                                                                     out);
    CTU_CHECK_LAUNCH("extract_patches_flip");
    return CTU_OK;
}

extern "C" int ctu_window_accumulate_flip(const float* patches, const int32_t* coords, const int32_t* valid,
                                          const int32_t* box, const int32_t* flip, int B, int K, int D, int H, int W, int pd,
                                          int ph, int pw, const float* wz, const float* wy, const float* wx, float wmin,
                                          int bz, int by, int bx, float* num, float* wsum, float* sq, float* sh,
                                          void* stream) {
    CTU_REQUIRE(patches && coords && valid && box && flip && wz && wy && wx && num, "window_accumulate_flip: null pointer");
    CTU_REQUIRE(B > 0 && B <= MAX_BATCH, "window_accumulate_flip: batch %d outside [1, %d]", B, MAX_BATCH);
    CTU_REQUIRE(K >= 1 && K <= 4, "window_accumulate_flip: %d channels (1..4 supported)", K);
    CTU_REQUIRE(!sh || K >= 2, "window_accumulate_flip: the entropy sum needs at least 2 channels");
    CTU_REQUIRE(D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "window_accumulate_flip: bad shape");
    CTU_REQUIRE(pw % 4 == 0, "window_accumulate_flip: patch width %d not a multiple of 4", pw);
    CTU_REQUIRE(bz > 0 && by > 0 && bx > 0 && bx % 4 == 0, "window_accumulate_flip: box extent %dx%dx%d (x a multiple of 4)", bz, by, bx);
    CTU_REQUIRE(aligned16(patches) && aligned16(wx) && aligned16(num) && (!wsum || aligned16(wsum)) && (!sq || aligned16(sq)) &&
                    (!sh || aligned16(sh)),
                "window_accumulate_flip: patches, wx and the accumulators must be 16-byte aligned");
    const unsigned grid = stream_grid((int64_t)bz * by * (bx / 4));
    hipStream_t st = (hipStream_t)stream;
    const float il = inv_ln(K);
#define CTU_WA(KK, SQ, SH)                                                                                              \
    accumulate_flip_kernel<KK, SQ, SH><<<grid, SB, 0, st>>>(patches, coords, valid, box, flip, B, D, H, W, pd, ph, pw, wz, wy, \
                                                            wx, wmin, bz, by, bx, num, wsum, sq, sh, il)
#define CTU_WA_K(KK)                                  \
    if (sq && sh) CTU_WA(KK, true, true);             \
    else if (sq) CTU_WA(KK, true, false);             \
    else if (sh) CTU_WA(KK, false, true);             \
    else CTU_WA(KK, false, false)
    switch (K) {
        case 1: if (sq) CTU_WA(1, true, false); else CTU_WA(1, false, false); break;
        case 2: CTU_WA_K(2); break;
        case 3: CTU_WA_K(3); break;
        default: CTU_WA_K(4); break;
    }
#undef CTU_WA_K
#undef CTU_WA
    CTU_CHECK_LAUNCH("window_accumulate_flip");
    return CTU_OK;
}

extern "C" int ctu_window_finalize_stats(const float* num, const float* wsum, const float* sq, const float* sh, int K,
                                         int64_t V, float* probs, uint8_t* labels, float* var, float* ent, float* mi,
                                         void* stream) {
    CTU_REQUIRE(num && wsum && probs, "window_finalize_stats: null pointer");
    CTU_REQUIRE(K >= 1 && K <= 4 && V > 0, "window_finalize_stats: bad shape K=%d", K);
    CTU_REQUIRE(!var || sq, "window_finalize_stats: variance needs the second-moment accumulator");
    CTU_REQUIRE(!mi || sh, "window_finalize_stats: mutual information needs the entropy accumulator");
    CTU_REQUIRE(!(ent || mi) || K >= 2, "window_finalize_stats: entropy needs at least 2 channels");
    const bool vec = V % 4 == 0 && aligned16(num) && aligned16(wsum) && aligned16(probs) && (!labels || ((uintptr_t)labels & 3) == 0) &&
                     (!var || (aligned16(sq) && aligned16(var))) && (!mi || (aligned16(sh) && aligned16(mi))) &&
                     (!ent || aligned16(ent));
    const unsigned grid = stream_grid(vec ? V / 4 : V);
    hipStream_t st = (hipStream_t)stream;
    const float il = inv_ln(K);
#define CTU_WF(KK)                                                                                                            \
    if (vec) finalize_stats_kernel<KK, true><<<grid, SB, 0, st>>>(num, wsum, sq, sh, V, probs, labels, var, ent, mi, il);     \
    else finalize_stats_kernel<KK, false><<<grid, SB, 0, st>>>(num, wsum, sq, sh, V, probs, labels, var, ent, mi, il)
    switch (K) {
        case 1: CTU_WF(1); break;
        case 2: CTU_WF(2); break;
        case 3: CTU_WF(3); break;
        default: CTU_WF(4); break;
    }
#undef CTU_WF
    CTU_CHECK_LAUNCH("window_finalize_stats");
    return CTU_OK;
}
