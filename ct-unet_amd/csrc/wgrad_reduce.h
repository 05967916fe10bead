// Block bodies of the fp32 weight-gradient slab reductions (conv3d.hip k = 3, conv3d_first.hip, convt.hip) and of the
// BatchNorm-backward finalize (elementwise.hip), shared with the merged launch of elementwise.hip that runs pending
// reductions in spare blocks of the finalize launch that comes next anyway (ctu_bn_bwd_finalize_jobs).  Each body takes its
// block index and thread index as arguments and its LDS from the caller; the stand-alone kernels are one-line callers.
#pragma once
#include "common.h"

// kinds of a ctu_wgrad_job (0 = empty: the entry reduced immediately)
constexpr int WGJ_K3S = 1;       // + (SM - 1) * 2 + (SN - 1): conv3d_wgrad_k3s_kernel<SM, SN>'s slabs
constexpr int WGJ_FIRST = 5;     // + (CIN - 1):               first_wgrad_kernel<CIN>'s
constexpr int WGJ_CONVT = 7;     // + (MI - 1) * 2 + (NJ - 1): convt2_wgrad_kernel<MI, NJ>'s
constexpr int WGJ_KINDS = 11;
constexpr int WGJ_LOADS = 16;     // loads a deferred reduction keeps in flight per thread (slab_sum; the stand-alone kernels: 1)
constexpr int FINALIZE_BLOCK = 256;      // threads that take part in the finalize body (EW_BLOCK of elementwise.hip)

// s = sum over k = part, part + RPARTS, ... < gx of src[k * stride], added in exactly that order.  U > 1: the loads of U
// terms are issued before their adds (the adds stay one chain in k order, so the sum has the same bits) -- a reduction that
// runs long after its slabs were written finds them in HBM, not in L2, and one dependent round trip per term is what its
// duration is made of.
template <int U>
__device__ __forceinline__ float slab_sum(const float* __restrict__ src, size_t stride, int part, int gx) {
    float s = 0.f;
    int k = part;
    if (U > 1) {
        for (; k + (U - 1) * RPARTS < gx; k += U * RPARTS) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[(size_t)(k + u * RPARTS) * stride];
#pragma unroll
            for (int u = 0; u < U; ++u) s += v[u];
        }
        for (; k + 3 * RPARTS < gx; k += 4 * RPARTS) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(k + u * RPARTS) * stride];
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
    }
    for (; k < gx; k += RPARTS) s += src[(size_t)k * stride];
    return s;
}

// conv3d_wgrad_k3s_kernel<SM, SN>: block (bx, pair) sums 64 consecutive slab elements of its channel-group pair over the
// gx slabs and scatters them into torch's [Co][Ci][27]
template <int SM, int SN, int U = 1>
__device__ __forceinline__ void wgrad_k3s_reduce_block(const float* __restrict__ ws, float* __restrict__ dw, int Co, int Ci,
                                                       const int32_t* __restrict__ cinv, int cin_p, int n_ci_g, int gx,
                                                       int bx, int pair, int tid, float (*red)[64]) {
    constexpr int QN = (SM == 2 && SN == 2) ? 1 : ((SM == 1 && SN == 1) ? 3 : 2);
    constexpr int NMF = 9 * QN;
    constexpr int CM = 16 / SM, CN = 16 / SN;
    const int e = tid & 63, part = tid >> 6;
    const int el = bx * 64 + e;
    float s = 0.f;
    if (el < NMF * 256) s = slab_sum<U>(ws + (size_t)pair * gx * (NMF * 256) + el, NMF * 256, part, gx);
    red[part][e] = s;
    __syncthreads();
    if (part != 0 || el >= NMF * 256) return;
    const float tot = red_total(red, e);
    const int t = el >> 8, i = (el >> 4) & 15, j = el & 15;
    const int r = t / QN, q = t % QN;
    const int sm = (SM == 2) ? i / 8 : 0, cil = (SM == 2) ? i % 8 : i;
    const int sn = (SN == 2) ? j / 8 : 0, col = (SN == 2) ? j % 8 : j;
    int kw;
    bool ok = true;
    if (SM == 1 && SN == 1) kw = q;
    else if (SM == 2 && SN == 2) { kw = sm + sn; ok = !(sm == 0 && sn == 1); }
    else if (SN == 2) { if (q == 0) { kw = 0; ok = sn == 0; } else kw = 1 + sn; }
    else { if (q == 0) kw = sm; else { kw = 2; ok = sm == 1; } }
    const int cig = pair % n_ci_g, cog = pair / n_ci_g;
    const int cip = cig * CM + cil, co = cog * CN + col;
    const int ci = (cip < cin_p) ? (cinv ? cinv[cip] : (cip < Ci ? cip : -1)) : -1;
    if (ok && ci >= 0 && co < Co) dw[((size_t)co * Ci + ci) * 27 + r * 3 + kw] = tot;
}

// first_wgrad_kernel<CIN>: block bx sums 64 consecutive elements of the [MTN][16 rows][16 co] slabs
template <int CIN, int U = 1>
__device__ __forceinline__ void first_wgrad_reduce_block(const float* __restrict__ ws, float* __restrict__ dw, int Co, int gx,
                                                         int bx, int tid, float (*red)[64]) {
    constexpr int MTN = (27 * CIN + 15) / 16;
    static_assert(RPARTS == 16, "16 slab groups x 64 elements");
    const int e = tid & 63, part = tid >> 6;          // 1024 threads: 16 slab groups x 64 elements
    const int el = bx * 64 + e;
    float s = 0.f;
    if (el < MTN * 256) {
        // 4 independent chains per thread (coalesced 256-byte rows of 4 slabs in flight), combined in a fixed order
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = part;
        if (U > 1) {                               // U rounds of the four chains, their loads first (same adds, same order)
            for (; k + 64 * (U - 1) + 48 < gx; k += 64 * U) {
                float v[U][4];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[u][c] = ws[(size_t)(k + 64 * u + 16 * c) * (MTN * 256) + el];
#pragma unroll
                for (int u = 0; u < U; ++u) { s0 += v[u][0]; s1 += v[u][1]; s2 += v[u][2]; s3 += v[u][3]; }
            }
        }
        for (; k + 48 < gx; k += 64) {
            s0 += ws[(size_t)k * (MTN * 256) + el];
            s1 += ws[(size_t)(k + 16) * (MTN * 256) + el];
            s2 += ws[(size_t)(k + 32) * (MTN * 256) + el];
            s3 += ws[(size_t)(k + 48) * (MTN * 256) + el];
        }
        for (; k < gx; k += 16) s0 += ws[(size_t)k * (MTN * 256) + el];
        s = (s0 + s1) + (s2 + s3);
    }
    red[part][e] = s;
    __syncthreads();
    if (part != 0 || el >= MTN * 256) return;
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += red[q][e];
    const int r = el >> 4, co = el & 15, tap = r / CIN, ci = r % CIN;
    if (r < 27 * CIN && co < Co) dw[((size_t)co * CIN + ci) * 27 + tap] = tot;
}

// convt2_wgrad_kernel<MI, NJ>: dw[ci][co][tap]: block bx owns 64 consecutive outputs (co fastest) and sums the gx slabs of
// their tile group; the outputs after the last weight are the bias gradient (wsb: the per-block column sums)
template <int MI, int NJ, int U = 1>
__device__ __forceinline__ void convt2_wgrad_reduce_block(const float* __restrict__ ws, const float* __restrict__ wsb,
                                                          float* __restrict__ dw, float* __restrict__ dbias, int Ci, int Co,
                                                          const int32_t* __restrict__ imap, int n_ci_t, int gx, int bx,
                                                          int tid, float (*red)[64]) {
    constexpr int CA = 16 * MI, CG = 16 * NJ, SL = 8 * MI * NJ * 256;
    const int e = tid & 63, part = tid >> 6;
    const int idx = bx * 64 + e;
    float s = 0.f;
    const int ndw = Ci * Co * 8;
    const bool ok = idx < ndw, okb = dbias && idx >= ndw && idx < ndw + Co;
    int co = 0, ci = 0, tap = 0;
    if (ok) {
        co = idx % Co; ci = (idx / Co) % Ci; tap = idx / (Co * Ci);
        const int cip = imap ? imap[ci] : ci;      // logical -> padded position
        const int cig = cip / CA, cog = co / CG, x = (cip % CA) >> 4, y = (co % CG) >> 4;
        const float* src = ws + ((size_t)(cog * n_ci_t + cig) * gx) * SL + ((tap * MI + x) * NJ + y) * 256 + (cip & 15) * 16 + (co & 15);
        s = slab_sum<U>(src, SL, part, gx);
    } else if (okb) {
        co = idx - ndw;
        s = slab_sum<U>(wsb + ((size_t)(co / CG) * gx) * CG + co % CG, CG, part, gx);
    }
    red[part][e] = s;
    __syncthreads();
    if (part == 0 && ok) dw[((size_t)ci * Co + co) * 8 + tap] = red_total(red, e);
    if (part == 0 && okb) dbias[co] = red_total(red, e);
}

// what ctu_bn_bwd_finalize takes (the merged launch carries it in its kernel arguments)
struct BnBwdFinArgs {
    const float* partials; const float* gamma; const float* invstd; const float* mean;
    float* dgamma; float* dbeta; float* coef; float* rmean; float* rvar;
    long long* nbt;
    double count;
    float momentum, eps;
    int nb, C, cp;
};

// BatchNorm-backward finalize of channel c.  coef[0..cp) = k0 = gamma*invstd ; coef[cp..2cp) = k1 = dbeta/n ;
// coef[2cp..3cp) = k2 = dgamma/n ; and the same backward as one affine map of the raw output (bn_bwd_lazy4, common.h):
// coef[3cp..4cp) = A = -k0 k2 invstd, coef[4cp..5cp) = B = -k0 (k1 - k2 mean invstd).
// Threads tid < FINALIZE_BLOCK stride over the rows and their waves are summed in a fixed order; EVERY thread of the block
// must call (one barrier), the threads of a larger block beyond FINALIZE_BLOCK add nothing.  sm: 2 * FINALIZE_BLOCK / 64 doubles.
__device__ __forceinline__ void bn_bwd_finalize_block(const BnBwdFinArgs& f, int c, int tid, double* sm) {
    const int cp = f.cp;
    if (f.nbt && f.rmean && c == 0 && tid == 0) f.nbt[0] += 1;                       // the replayed update counts too
    float g_ = 0.f, is_ = 0.f, mu_ = 0.f, rm0 = 0.f, rv0 = 0.f;                      // (prefetched: see bn_finalize_kernel)
    if (tid == 0 && c < f.C) {
        g_ = f.gamma[c]; is_ = f.invstd[c]; mu_ = f.mean[c];
        if (f.rmean) { rm0 = f.rmean[c]; rv0 = f.rvar[c]; }
    }
    double s1 = 0.0, s2 = 0.0;
    if (tid < FINALIZE_BLOCK) {
        if (c < f.C) {
#pragma unroll 4
            for (int b = tid; b < f.nb; b += FINALIZE_BLOCK) {
                s1 += (double)f.partials[(size_t)b * 2 * cp + c];
                s2 += (double)f.partials[(size_t)b * 2 * cp + cp + c];
            }
        }
        // sum over the FINALIZE_BLOCK threads: wave butterflies, one LDS exchange, a fixed-order sum over the waves
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        if ((tid & 63) == 0) { sm[(tid >> 6) * 2] = s1; sm[(tid >> 6) * 2 + 1] = s2; }
    }
    __syncthreads();
    if (tid != 0) return;
    s1 = 0.0; s2 = 0.0;
#pragma unroll
    for (int w = 0; w < FINALIZE_BLOCK / 64; ++w) { s1 += sm[w * 2]; s2 += sm[w * 2 + 1]; }
    float* coef = f.coef;
    if (c < f.C) {
        f.dbeta[c] = (float)s1;
        f.dgamma[c] = (float)s2;
        const float k0 = g_ * is_, k1 = (float)(s1 / f.count), k2 = (float)(s2 / f.count);
        coef[c] = k0;
        coef[cp + c] = k1;
        coef[2 * cp + c] = k2;
        coef[3 * cp + c] = -k0 * k2 * is_;
        coef[4 * cp + c] = -k0 * (k1 - k2 * mu_ * is_);
        if (f.rmean) {
            // the running-stat update torch.utils.checkpoint's recompute repeats in backward (models.py:232-255):
            // same batch statistics as the forward update; the biased variance is recovered from invstd
            const double istd = (double)is_;
            double var = 1.0 / (istd * istd) - (double)f.eps;
            if (var < 0.0) var = 0.0;
            const float unb = (float)(var * (f.count / (f.count > 1.0 ? f.count - 1.0 : 1.0)));
            f.rmean[c] = (1.f - f.momentum) * rm0 + f.momentum * mu_;
            f.rvar[c] = (1.f - f.momentum) * rv0 + f.momentum * unb;
        }
    } else {
        coef[c] = 0.f; coef[cp + c] = 0.f; coef[2 * cp + c] = 0.f; coef[3 * cp + c] = 0.f; coef[4 * cp + c] = 0.f;
    }
}

// blocks a job's reduction needs (host): its stand-alone kernel's grid, flattened
inline int wgrad_job_blocks(const ctu_wgrad_job& j) {
    if (j.kind >= WGJ_K3S && j.kind < WGJ_FIRST) return ceil_div(j.nmf * 256, 64) * j.pairs;
    if (j.kind >= WGJ_FIRST && j.kind < WGJ_CONVT) return ceil_div(j.nmf * 256, 64);
    return ceil_div(j.Ci * j.Co * 8 + j.Co, 64);
}

// block `b` of job j's reduction (b < wgrad_job_blocks(j)); every thread of the 64 * RPARTS-thread block calls
__device__ __forceinline__ void wgrad_job_block(const ctu_wgrad_job& j, int b, int tid, float (*red)[64]) {
    const int nbx = j.nmf * 4;                     // k3s: blocks per channel-group pair
#define CTU_WGJ_K3S(SM_, SN_) \
    wgrad_k3s_reduce_block<SM_, SN_, WGJ_LOADS>(j.ws, j.dw, j.Co, j.Ci, j.cinv, j.cin_p, j.n_ci_g, j.gx, b % nbx, b / nbx, tid, red)
#define CTU_WGJ_CONVT(MI_, NJ_)                                                                                          \
    convt2_wgrad_reduce_block<MI_, NJ_, WGJ_LOADS>(j.ws, j.ws + (size_t)j.pairs * j.gx * (8 * MI_ * NJ_ * 256), j.dw, j.db, j.Ci, j.Co, \
                                        j.cinv, j.n_ci_g, j.gx, b, tid, red)
    switch (j.kind) {
    case WGJ_K3S + 0: CTU_WGJ_K3S(1, 1); break;
    case WGJ_K3S + 1: CTU_WGJ_K3S(1, 2); break;
    case WGJ_K3S + 2: CTU_WGJ_K3S(2, 1); break;
    case WGJ_K3S + 3: CTU_WGJ_K3S(2, 2); break;
    case WGJ_FIRST + 0: first_wgrad_reduce_block<1, WGJ_LOADS / 4>(j.ws, j.dw, j.Co, j.gx, b, tid, red); break;
    case WGJ_FIRST + 1: first_wgrad_reduce_block<2, WGJ_LOADS / 4>(j.ws, j.dw, j.Co, j.gx, b, tid, red); break;
    case WGJ_CONVT + 0: CTU_WGJ_CONVT(1, 1); break;
    case WGJ_CONVT + 1: CTU_WGJ_CONVT(1, 2); break;
    case WGJ_CONVT + 2: CTU_WGJ_CONVT(2, 1); break;
    case WGJ_CONVT + 3: CTU_WGJ_CONVT(2, 2); break;
    default: break;
    }
#undef CTU_WGJ_K3S
#undef CTU_WGJ_CONVT
}
