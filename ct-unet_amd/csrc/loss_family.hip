// Segmentation loss family on one 2-channel NCDHW map for gfx950: class-weighted / focal cross-entropy, the reference's
// squared-denominator Dice, a Tversky term on the foreground channel and a boundary (surface) term that reads a signed
// distance map.  Same structure as the CE + Dice pair of head_loss.hip: HBM-bound streaming kernels, LOSS_BX blocks per
// item, 16-byte loads of the four planes (five with the distance map), two-stage deterministic reductions, no atomics.
//
// Definition (ctunet_amd/losses.py restates it; tests/loss_family_ref.py is the float64 reference), per voxel with
// logits (a, b), target (ta, tb), class c = 1 where tb > ta else 0, p = softmax(a, b), view pr = p (dice_softmax) or (a, b),
// q = pr[1], g = tb:
//   ce       = ce_lambda * sum w_c (1 - p_c)^gamma (-log p_c) / sum w_c                       over all items and voxels
//   dice     = dice_lambda * (1 - 2 mean_n (sum pr t + eps) / (sum pr^2 + sum t^2 + eps))
//   tversky  = tversky_lambda * (1 - mean_n (TP + eps) / (TP + alpha FP + beta FN + eps)),  TP = sum q g, FP = sum q - TP,
//              FN = sum g - TP
//   boundary = boundary_lambda * sum q phi / (N V),  a non-finite phi counting as 0
// The extensions are template flags (PHI: the fifth stream, FOCAL: gamma != 0, TV: the Tversky sums), so a weighted-CE call
// pays for neither the focal factor's exponential nor the distance map.
#include "common.h"

namespace {

constexpr int HB = 256;
constexpr int LOSS_BX = 1024;   // blocks per batch item, as head_loss.hip (4 per CU: 16 B x 4..5 streams per lane in flight)
constexpr int ROW = 8;          // floats of one block's partial row: ce num, ce weight, dice num, dice den, q g, q, g, q phi
constexpr int TAIL = 4;         // floats per item behind the rows: dice (num + eps, den + eps), Tversky (A, B); then the weight sum

struct SegP {
    const float* pred;
    const float* tgt;
    const float* phi;           // [N, V] or NULL
    int N;
    int64_t V;
    float w0, w1, gamma;
    int dice_softmax;
};

// one voxel's softmax from one exponential: e = exp(-|a - b|), the larger probability is 1 / (1 + e), the smaller e / (1 + e)
struct Point {
    float pa, pb;               // softmax
    float pc, po;               // ... of the target class and of the other one (1 - p_c, not by subtraction)
    float nll;                  // -log p_c  = max(other - own, 0) + log(1 + e)
    float nlo;                  // -log po   = max(own - other, 0) + log(1 + e): po^gamma is exp(-gamma nlo), no pow
    bool cls1;
};
__device__ __forceinline__ Point seg_point(float a, float b, float ta, float tb) {
    Point r;
    const float e = expf(-fabsf(a - b));
    const float s = 1.f + e;
    const float hi = 1.f / s, lo = e * hi;
    const bool bmax = b > a;
    r.pa = bmax ? lo : hi;
    r.pb = bmax ? hi : lo;
    r.cls1 = tb > ta;                               // argmax: the first index wins ties
    r.pc = r.cls1 ? r.pb : r.pa;
    r.po = r.cls1 ? r.pa : r.pb;
    const float d = r.cls1 ? a - b : b - a;         // other logit minus own
    const float l = logf(s);
    r.nll = fmaxf(d, 0.f) + l;
    r.nlo = fmaxf(-d, 0.f) + l;
    return r;
}
// (1 - p_c)^gamma, gamma > 0: 0 where the other probability underflowed, never inf
__device__ __forceinline__ float focal_factor(const Point& r, float gamma) { return expf(-gamma * r.nlo); }

__device__ __forceinline__ float finite_or_zero(float x) { return fabsf(x) <= 3.402823466e38f ? x : 0.f; }   // NaN fails too

template <bool PHI, bool FOCAL, bool TV>
__global__ __launch_bounds__(HB) void seg_loss_fwd_kernel(SegP p, float* __restrict__ ws) {
    const int n = blockIdx.y;
    const int64_t V = p.V;
    const float* p0 = p.pred + (size_t)n * 2 * V;
    const float* p1 = p0 + V;
    const float* t0 = p.tgt + (size_t)n * 2 * V;
    const float* t1 = t0 + V;
    const float* ph = PHI ? p.phi + (size_t)n * V : nullptr;
    float acc[ROW] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto point = [&](float a, float b, float ta, float tb, float f) {
        const Point r = seg_point(a, b, ta, tb);
        const float w = r.cls1 ? p.w1 : p.w0;
        float ce = w * r.nll;
        if (FOCAL) ce *= focal_factor(r, p.gamma);
        acc[0] += ce;
        acc[1] += w;
        const float va = p.dice_softmax ? r.pa : a, vb = p.dice_softmax ? r.pb : b;
        acc[2] += va * ta + vb * tb;
        acc[3] += (va * va + vb * vb) + (ta * ta + tb * tb);
        if (TV) { acc[4] += vb * tb; acc[5] += vb; acc[6] += tb; }
        if (PHI) acc[7] += vb * finite_or_zero(f);
    };
    uintptr_t al = reinterpret_cast<uintptr_t>(p.pred) | reinterpret_cast<uintptr_t>(p.tgt);
    if (PHI) al |= reinterpret_cast<uintptr_t>(p.phi);
    const bool vec = (V & 3) == 0 && (al & 15) == 0;
    if (vec) {
        const int64_t V4 = V >> 2;
        for (int64_t q = (int64_t)blockIdx.x * HB + threadIdx.x; q < V4; q += (int64_t)gridDim.x * HB) {
            const float4 a = reinterpret_cast<const float4*>(p0)[q], b = reinterpret_cast<const float4*>(p1)[q];
            const float4 ta = reinterpret_cast<const float4*>(t0)[q], tb = reinterpret_cast<const float4*>(t1)[q];
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (PHI) f = reinterpret_cast<const float4*>(ph)[q];
            point(a.x, b.x, ta.x, tb.x, f.x); point(a.y, b.y, ta.y, tb.y, f.y);
            point(a.z, b.z, ta.z, tb.z, f.z); point(a.w, b.w, ta.w, tb.w, f.w);
        }
    } else {
        for (int64_t v = (int64_t)blockIdx.x * HB + threadIdx.x; v < V; v += (int64_t)gridDim.x * HB)
            point(p0[v], p1[v], t0[v], t1[v], PHI ? ph[v] : 0.f);
    }
    __shared__ float red[HB / 64][ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < ROW; ++j) {
        const float s = wave_sum(acc[j]);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < ROW) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < HB / 64; ++w) s += red[w][threadIdx.x];
        ws[((size_t)n * gridDim.x + blockIdx.x) * ROW + threadIdx.x] = s;
    }
}

// one wave: lane l sums the block rows l, l + 64, ... in double, then a fixed-order butterfly -> deterministic.
// Writes the four terms and the tail the backward reads: per item (dice num + eps, dice den + eps, A, B) with the Tversky
// ratio's derivative d(-ratio / N)/dq = A g + B, then the global CE weight sum.
__global__ void seg_loss_final_kernel(float* __restrict__ ws, int N, int nbx, int64_t V, ctu_seg_loss_cfg c,
                                      float* __restrict__ terms) {
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    const double eps = 0.0000001;
    double ce = 0.0, wsum = 0.0, dsum = 0.0, tsum = 0.0, bsum = 0.0;
    float* tail = ws + (size_t)N * nbx * ROW;
    for (int n = 0; n < N; ++n) {
        double r[ROW] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int b = lane; b < nbx; b += 64) {
            const float4* row = reinterpret_cast<const float4*>(ws + ((size_t)n * nbx + b) * ROW);
            const float4 u = row[0], v = row[1];
            r[0] += u.x; r[1] += u.y; r[2] += u.z; r[3] += u.w; r[4] += v.x; r[5] += v.y; r[6] += v.z; r[7] += v.w;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < ROW; ++j) r[j] += __shfl_xor(r[j], o);
        }
        ce += r[0]; wsum += r[1]; bsum += r[7];
        dsum += (r[2] + eps) / (r[3] + eps);
        const double tp = r[4], a = c.tversky_alpha, be = c.tversky_beta;
        const double tnum = tp + eps, tden = tp + a * (r[5] - tp) + be * (r[6] - tp) + eps;
        tsum += tnum / tden;
        if (lane == 0) {
            tail[n * TAIL + 0] = (float)(r[2] + eps);
            tail[n * TAIL + 1] = (float)(r[3] + eps);
            tail[n * TAIL + 2] = (float)(-(1.0 / tden - tnum * (1.0 - a - be) / (tden * tden)) / N);
            tail[n * TAIL + 3] = (float)(a * tnum / (tden * tden) / N);
        }
    }
    if (lane == 0) {
        tail[(size_t)N * TAIL] = (float)wsum;
        terms[0] = c.ce_lambda != 0.f ? (float)(c.ce_lambda * ce / wsum) : 0.f;
        terms[1] = c.dice_lambda != 0.f ? (float)(c.dice_lambda * (1.0 - 2.0 * dsum / N)) : 0.f;
        terms[2] = c.tversky_lambda != 0.f ? (float)(c.tversky_lambda * (1.0 - tsum / N)) : 0.f;
        terms[3] = c.boundary_lambda != 0.f ? (float)(c.boundary_lambda * bsum / ((double)N * (double)V)) : 0.f;
    }
}

struct SegG {
    const float* tail;
    const float* g[4];          // upstream gradients of (ce, dice, tversky, boundary): one device float each, NULL = 1
    float lam[4];
    float* gpred;
    int accumulate;
};

template <bool PHI, bool FOCAL, bool TV>
__global__ __launch_bounds__(HB) void seg_loss_bwd_kernel(SegP p, SegG s) {
    const int n = blockIdx.y;
    const int64_t V = p.V;
    float k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = (s.g[j] ? s.g[j][0] : 1.f) * s.lam[j];
    const float kce = k[0] / s.tail[(size_t)p.N * TAIL];
    const float nume = s.tail[n * TAIL + 0], dene = s.tail[n * TAIL + 1];
    const float kd = k[1] * (-2.f / (float)p.N);
    const float kd_t = kd / dene, kd_p = kd * nume * 2.f / (dene * dene);
    const float ktA = TV ? k[2] * s.tail[n * TAIL + 2] : 0.f, ktB = TV ? k[2] * s.tail[n * TAIL + 3] : 0.f;
    const float kb = PHI ? k[3] / ((float)p.N * (float)V) : 0.f;
    const bool dice_on = s.lam[1] != 0.f;
    const size_t base = (size_t)n * 2 * V;
    const float* ph = PHI ? p.phi + (size_t)n * V : nullptr;
    auto point = [&](float a, float b, float ta, float tb, float f, float& ga, float& gb) {
        const Point r = seg_point(a, b, ta, tb);
        // d/dz of w po^gamma (-log p_c), z = own logit - other:  -w po^gamma (gamma p_c nll + po); with
        // d po / dz = -p_c po the factor (1 - p)^(gamma - 1) never appears, so saturated logits give 0, not inf * 0
        float dz = r.po;
        if (FOCAL) dz = focal_factor(r, p.gamma) * fmaf(p.gamma * r.pc, r.nll, r.po);
        dz *= -kce * (r.cls1 ? p.w1 : p.w0);
        ga = r.cls1 ? -dz : dz;
        gb = r.cls1 ? dz : -dz;
        if (dice_on || TV || PHI) {
            const float va = p.dice_softmax ? r.pa : a, vb = p.dice_softmax ? r.pb : b;
            float da = 0.f, db = 0.f;
            if (dice_on) { da = kd_t * ta - kd_p * va; db = kd_t * tb - kd_p * vb; }
            if (TV) db += fmaf(ktA, tb, ktB);
            if (PHI) db += kb * finite_or_zero(f);
            if (p.dice_softmax) {
                const float dot = da * r.pa + db * r.pb;
                da = r.pa * (da - dot); db = r.pb * (db - dot);
            }
            ga += da; gb += db;
        }
    };
    uintptr_t al = reinterpret_cast<uintptr_t>(p.pred) | reinterpret_cast<uintptr_t>(p.tgt) | reinterpret_cast<uintptr_t>(s.gpred);
    if (PHI) al |= reinterpret_cast<uintptr_t>(p.phi);
    const bool vec = (V & 3) == 0 && (al & 15) == 0;
    if (vec) {
        const int64_t V4 = V >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(p.pred + base);
        const float4* b4 = reinterpret_cast<const float4*>(p.pred + base + V);
        const float4* ta4 = reinterpret_cast<const float4*>(p.tgt + base);
        const float4* tb4 = reinterpret_cast<const float4*>(p.tgt + base + V);
        float4* ga4 = reinterpret_cast<float4*>(s.gpred + base);
        float4* gb4 = reinterpret_cast<float4*>(s.gpred + base + V);
        for (int64_t q = (int64_t)blockIdx.x * HB + threadIdx.x; q < V4; q += (int64_t)gridDim.x * HB) {
            const float4 a = a4[q], b = b4[q], ta = ta4[q], tb = tb4[q];
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (PHI) f = reinterpret_cast<const float4*>(ph)[q];
            float4 ga, gb;
            point(a.x, b.x, ta.x, tb.x, f.x, ga.x, gb.x); point(a.y, b.y, ta.y, tb.y, f.y, ga.y, gb.y);
            point(a.z, b.z, ta.z, tb.z, f.z, ga.z, gb.z); point(a.w, b.w, ta.w, tb.w, f.w, ga.w, gb.w);
            if (s.accumulate) {
                const float4 oa = ga4[q], ob = gb4[q];
                ga.x += oa.x; ga.y += oa.y; ga.z += oa.z; ga.w += oa.w; gb.x += ob.x; gb.y += ob.y; gb.z += ob.z; gb.w += ob.w;
            }
            ga4[q] = ga; gb4[q] = gb;
        }
        return;
    }
    for (int64_t v = (int64_t)blockIdx.x * HB + threadIdx.x; v < V; v += (int64_t)gridDim.x * HB) {
        float ga, gb;
        point(p.pred[base + v], p.pred[base + V + v], p.tgt[base + v], p.tgt[base + V + v], PHI ? ph[v] : 0.f, ga, gb);
        if (s.accumulate) { ga += s.gpred[base + v]; gb += s.gpred[base + V + v]; }
        s.gpred[base + v] = ga;
        s.gpred[base + V + v] = gb;
    }
}

// the three extension flags -> one of eight instantiations
template <bool PHI, bool FOCAL>
void launch_fwd2(bool tv, dim3 grid, hipStream_t st, const SegP& p, float* ws) {
    if (tv) seg_loss_fwd_kernel<PHI, FOCAL, true><<<grid, HB, 0, st>>>(p, ws);
    else seg_loss_fwd_kernel<PHI, FOCAL, false><<<grid, HB, 0, st>>>(p, ws);
}
void launch_fwd(bool phi, bool focal, bool tv, dim3 grid, hipStream_t st, const SegP& p, float* ws) {
    if (phi) { if (focal) launch_fwd2<true, true>(tv, grid, st, p, ws); else launch_fwd2<true, false>(tv, grid, st, p, ws); }
    else { if (focal) launch_fwd2<false, true>(tv, grid, st, p, ws); else launch_fwd2<false, false>(tv, grid, st, p, ws); }
}
template <bool PHI, bool FOCAL>
void launch_bwd2(bool tv, dim3 grid, hipStream_t st, const SegP& p, const SegG& s) {
    if (tv) seg_loss_bwd_kernel<PHI, FOCAL, true><<<grid, HB, 0, st>>>(p, s);
    else seg_loss_bwd_kernel<PHI, FOCAL, false><<<grid, HB, 0, st>>>(p, s);
}
void launch_bwd(bool phi, bool focal, bool tv, dim3 grid, hipStream_t st, const SegP& p, const SegG& s) {
    if (phi) { if (focal) launch_bwd2<true, true>(tv, grid, st, p, s); else launch_bwd2<true, false>(tv, grid, st, p, s); }
    else { if (focal) launch_bwd2<false, true>(tv, grid, st, p, s); else launch_bwd2<false, false>(tv, grid, st, p, s); }
}

}  // namespace

// =================================================================== C ABI
static int fill_seg(SegP& p, const float* pred, const float* target, const float* phi, int N, int64_t V,
                    const ctu_seg_loss_cfg* c, const char* name) {
    CTU_REQUIRE(pred && target && c, "%s: null pointer", name);
    CTU_REQUIRE(N > 0 && N <= 65535 && V > 0, "%s: N=%d V=%lld", name, N, (long long)V);
    CTU_REQUIRE(c->w0 > 0.f && c->w1 > 0.f && c->w0 <= 3.0e38f && c->w1 <= 3.0e38f, "%s: class weights must be positive and finite (%g, %g)",
                name, (double)c->w0, (double)c->w1);
    CTU_REQUIRE(c->focal_gamma >= 0.f && c->focal_gamma <= 3.0e38f, "%s: focal_gamma must be >= 0 and finite (%g)", name, (double)c->focal_gamma);
    CTU_REQUIRE(c->tversky_alpha >= 0.f && c->tversky_beta >= 0.f && c->tversky_alpha <= 3.0e38f && c->tversky_beta <= 3.0e38f,
                "%s: tversky_alpha / tversky_beta must be >= 0 and finite (%g, %g)", name, (double)c->tversky_alpha, (double)c->tversky_beta);
    CTU_REQUIRE(c->boundary_lambda == 0.f || phi, "%s: boundary_lambda != 0 needs the distance map", name);
    p.pred = pred; p.tgt = target;
    p.phi = c->boundary_lambda != 0.f ? phi : nullptr;
    p.N = N; p.V = V; p.w0 = c->w0; p.w1 = c->w1; p.gamma = c->focal_gamma; p.dice_softmax = c->dice_softmax != 0;
    return CTU_OK;
}

extern "C" size_t ctu_seg_loss_ws_floats(int N, int64_t V) {
    (void)V;
    return (size_t)N * LOSS_BX * ROW + (size_t)N * TAIL + 1;
}

extern "C" int ctu_seg_loss_fwd(const float* pred, const float* target, const float* phi, int N, int64_t V,
                                const ctu_seg_loss_cfg* cfg, float* terms, float* ws, void* stream) {
    SegP p;
    int rc = fill_seg(p, pred, target, phi, N, V, cfg, "seg_loss_fwd");
    if (rc != CTU_OK) return rc;
    CTU_REQUIRE(terms && ws, "seg_loss_fwd: null pointer");
    CTU_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "seg_loss_fwd: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    launch_fwd(p.phi != nullptr, cfg->focal_gamma != 0.f, cfg->tversky_lambda != 0.f, dim3(LOSS_BX, N), st, p, ws);
    CTU_CHECK_LAUNCH("seg_loss_fwd");
    seg_loss_final_kernel<<<1, 64, 0, st>>>(ws, N, LOSS_BX, V, *cfg, terms);
    CTU_CHECK_LAUNCH("seg_loss_final");
    return CTU_OK;
}

extern "C" int ctu_seg_loss_bwd(const float* pred, const float* target, const float* phi, int N, int64_t V,
                                const ctu_seg_loss_cfg* cfg, const float* ws, const float* g_ce, const float* g_dice,
                                const float* g_tversky, const float* g_boundary, float* gpred, int accumulate, void* stream) {
    SegP p;
    int rc = fill_seg(p, pred, target, phi, N, V, cfg, "seg_loss_bwd");
    if (rc != CTU_OK) return rc;
    CTU_REQUIRE(ws && gpred, "seg_loss_bwd: null pointer");
    SegG s;
    s.tail = ws + (size_t)N * LOSS_BX * ROW;
    s.g[0] = g_ce; s.g[1] = g_dice; s.g[2] = g_tversky; s.g[3] = g_boundary;
    s.lam[0] = cfg->ce_lambda; s.lam[1] = cfg->dice_lambda; s.lam[2] = cfg->tversky_lambda; s.lam[3] = cfg->boundary_lambda;
    s.gpred = gpred; s.accumulate = accumulate;
    launch_bwd(p.phi != nullptr, cfg->focal_gamma != 0.f, cfg->tversky_lambda != 0.f, dim3(LOSS_BX, N), (hipStream_t)stream, p, s);
    CTU_CHECK_LAUNCH("seg_loss_bwd");
    return CTU_OK;
}
