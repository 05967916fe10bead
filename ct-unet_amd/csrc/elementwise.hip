// HBM-bound kernels of the U-Net path for gfx950: layout conversion, BatchNorm3d statistics
// finalisation and backward, MaxPool3d(2,2) forward/backward, skip add, per-channel sums (the optimizers: optim.hip).
// All activation accesses are 16-byte (float4) channels-last vectors; reductions are
// two-stage (per-block partials, then a small finalize kernel) -- no float atomics, so
// results are bitwise reproducible run to run.
#include "common.h"
#include "bn_tail.h"
#include "channel_sum.h"
#include "wgrad_reduce.h"

static thread_local char g_err[512] = "";

void ctu_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* ctu_last_error(void) { return g_err; }
extern "C" int ctu_abi_version(void) { return CTU_ABI_VERSION; }
extern "C" const char* ctu_arch(void) { return "gfx950"; }

namespace {

constexpr int EW_BLOCK = 256;
static_assert(EW_BLOCK == FINALIZE_BLOCK, "wgrad_reduce.h block size");
static_assert(EW_BLOCK == CSUM_BLOCK, "channel_sum.h block size");
constexpr int FIN_BLOCK = 256;    // threads of the per-channel statistics finalisation
constexpr int MAX_RED_BLOCKS = 1024;

// ------------------------------------------------------------------ layout
// NCDHW -> NDHWC: one thread per (voxel, channel-quad); reads are coalesced along w per channel.
template <class T>
__global__ void ncdhw_to_ndhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int C, int64_t V,
                                      int64_t total_vox, int cp, int cs) {
    const int nq = cp >> 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total_vox * nq) return;
    // voxel fastest so that each channel plane is read contiguously by consecutive lanes
    const int64_t vox = idx % total_vox;
    const int qd = (int)(idx / total_vox);
    const int64_t n = vox / V, v = vox % V;
    float4 o;
    float* op = &o.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = qd * 4 + j;
        op[j] = (c < C) ? src[(n * C + c) * V + v] : 0.f;
    }
    st4<T>(dst + vox * cs + qd * 4, o);
}

template <class T>
__global__ void ndhwc_to_ncdhw_kernel(const T* __restrict__ src, float* __restrict__ dst, int C, int64_t V,
                                      int64_t total_vox, int cs) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total_vox * C) return;
    const int64_t vox = idx % total_vox;
    const int c = (int)(idx / total_vox);
    const int64_t n = vox / V, v = vox % V;
    dst[(n * C + c) * V + v] = (float)src[vox * cs + c];
}

// Sum of (a, b) over the NT threads of a block, in every thread: wave butterflies, one LDS exchange, a fixed-order sum
// over the waves (deterministic; one barrier instead of a log2(NT)-step LDS tree -- these kernels are all latency).
template <int NT>
__device__ __forceinline__ void block_sum2(double& a, double& b) {
    __shared__ double sm[2 * (NT / 64)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { sm[(threadIdx.x >> 6) * 2] = a; sm[(threadIdx.x >> 6) * 2 + 1] = b; }
    __syncthreads();
    a = 0.0; b = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) { a += sm[w * 2]; b += sm[w * 2 + 1]; }
}

// ------------------------------------------------------------------ BN finalize
__global__ void bn_finalize_kernel(const float* __restrict__ stats, int nblocks, int C, int cp, double count,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps,
                                   int n_updates, float* __restrict__ scale, float* __restrict__ shift,
                                   float* __restrict__ mean_out, float* __restrict__ invstd_out,
                                   long long* __restrict__ nbt) {
    const int c = blockIdx.x;
    if (nbt && c == 0 && threadIdx.x == 0 && n_updates > 0) nbt[0] += n_updates;     // num_batches_tracked
    // the channel's parameters are fetched BEFORE the row reduction (this kernel is one dependent chain of memory round
    // trips on the step's critical path: rows -> block sum -> parameters -> stores; the parameter trip now overlaps the rows)
    float g_ = 0.f, b_ = 0.f, rm0 = 0.f, rv0 = 0.f;
    if (threadIdx.x == 0 && c < C) {
        g_ = gamma[c]; b_ = beta[c];
        if (rmean && n_updates > 0) { rm0 = rmean[c]; rv0 = rvar[c]; }
    }
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int b = threadIdx.x; b < nblocks; b += FIN_BLOCK) {
            s1 += (double)stats[(size_t)b * 2 * cp + c];
            s2 += (double)stats[(size_t)b * 2 * cp + cp + c];
        }
    }
    block_sum2<FIN_BLOCK>(s1, s2);
    if (threadIdx.x == 0) {
        if (c < C) {
            const double mean = s1 / count;
            double var = s2 / count - mean * mean;
            if (var < 0.0) var = 0.0;
            const float invstd = (float)(1.0 / sqrt(var + (double)eps));
            const float sc = g_ * invstd;
            scale[c] = sc;
            shift[c] = b_ - (float)mean * sc;
            mean_out[c] = (float)mean;
            invstd_out[c] = invstd;
            if (rmean && n_updates > 0) {
                const float unb = (float)(var * (count / (count > 1.0 ? count - 1.0 : 1.0)));
                float rm = rm0, rv = rv0;
                for (int u = 0; u < n_updates; ++u) {
                    rm = (1.f - momentum) * rm + momentum * (float)mean;
                    rv = (1.f - momentum) * rv + momentum * unb;
                }
                rmean[c] = rm; rvar[c] = rv;
            }
        } else {
            scale[c] = 0.f; shift[c] = 0.f; mean_out[c] = 0.f; invstd_out[c] = 0.f;
        }
    }
}

__global__ void bn_eval_affine_kernel(const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                      float eps, int C, int cp, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cp) return;
    if (c < C) {
        const float sc = gamma[c] / sqrtf(rvar[c] + eps);
        scale[c] = sc;
        shift[c] = beta[c] - rmean[c] * sc;
    } else {
        scale[c] = 0.f; shift[c] = 0.f;
    }
}

// ------------------------------------------------------------------ BN+ReLU backward
// thread = (voxel stripe, channel quad); channel quad fixed per thread so its constants sit in registers.
template <class T>
__global__ void bn_relu_bwd_reduce_kernel(const T* __restrict__ y, int y_cs, const T* __restrict__ ga,
                                          int g_cs, int cp, const float* __restrict__ scale,
                                          const float* __restrict__ shift, const float* __restrict__ mean,
                                          const float* __restrict__ invstd, int64_t nvox,
                                          float* __restrict__ partials, ctu_bn_bwd_tail tail) {
    const int nq = cp >> 2;
    const int tpv = EW_BLOCK / nq;                  // voxels per block pass (nq divides 256 or not: extra threads idle)
    const int qd = threadIdx.x % nq, vl = threadIdx.x / nq;
    __shared__ float red[EW_BLOCK * 8];
    float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
    if (vl < tpv) {
        const float4 sc = *reinterpret_cast<const float4*>(scale + qd * 4);
        const float4 sh = *reinterpret_cast<const float4*>(shift + qd * 4);
        const float4 mu = *reinterpret_cast<const float4*>(mean + qd * 4);
        const float4 is = *reinterpret_cast<const float4*>(invstd + qd * 4);
        for (int64_t v = (int64_t)blockIdx.x * tpv + vl; v < nvox; v += (int64_t)gridDim.x * tpv) {
            const float4 yy = ld4<T>(y + v * y_cs + qd * 4);
            const float4 gg = ld4<T>(ga + v * g_cs + qd * 4);
            float gz;
            gz = (fmaf(yy.x, sc.x, sh.x) > 0.f) ? gg.x : 0.f; a1.x += gz; a2.x += gz * (yy.x - mu.x) * is.x;
            gz = (fmaf(yy.y, sc.y, sh.y) > 0.f) ? gg.y : 0.f; a1.y += gz; a2.y += gz * (yy.y - mu.y) * is.y;
            gz = (fmaf(yy.z, sc.z, sh.z) > 0.f) ? gg.z : 0.f; a1.z += gz; a2.z += gz * (yy.z - mu.z) * is.z;
            gz = (fmaf(yy.w, sc.w, sh.w) > 0.f) ? gg.w : 0.f; a1.w += gz; a2.w += gz * (yy.w - mu.w) * is.w;
        }
    }
    float* r = &red[threadIdx.x * 8];
    r[0] = a1.x; r[1] = a1.y; r[2] = a1.z; r[3] = a1.w; r[4] = a2.x; r[5] = a2.y; r[6] = a2.z; r[7] = a2.w;
    __syncthreads();
    // thread t < cp sums channel t over the voxel lanes (fixed order -> deterministic)
    if (threadIdx.x < cp) {
        const int c = threadIdx.x, q = c >> 2, j = c & 3;
        float s1 = 0.f, s2 = 0.f;
        for (int l = 0; l < tpv; ++l) {
            s1 += red[(l * nq + q) * 8 + j];
            s2 += red[(l * nq + q) * 8 + 4 + j];
        }
        st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + c, s1);
        st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + cp + c, s2);
    }
    if (tail.counter) bn_bwd_tail(tail, partials, gridDim.x, cp, gridDim.x);
}

// coef rows and arithmetic: bn_bwd_finalize_block (wgrad_reduce.h); one block per padded channel
__global__ void bn_bwd_finalize_kernel(BnBwdFinArgs f) {
    __shared__ double sm[2 * (EW_BLOCK / 64)];
    bn_bwd_finalize_block(f, blockIdx.x, threadIdx.x, sm);
}

// Pending weight-gradient slab reductions in one launch of 64 * RPARTS-thread blocks: block b of job j runs at
// start[j] + b.  FIN: the first f.cp blocks are bn_bwd_finalize_kernel's instead (their first EW_BLOCK threads) -- the
// reductions ride in spare blocks of a launch the backward chain needs anyway.  The two kinds of blocks exchange nothing.
struct WgJobTable { ctu_wgrad_job job[CTU_WGRAD_JOBS_MAX]; int start[CTU_WGRAD_JOBS_MAX + 1]; int n; };

template <bool FIN>
__global__ __launch_bounds__(64 * RPARTS) void wgrad_reduce_jobs_kernel(BnBwdFinArgs f, WgJobTable t) {
    __shared__ float red[RPARTS][64];
    __shared__ double sm[2 * (EW_BLOCK / 64)];
    int b = blockIdx.x;
    if (FIN) {
        if (b < f.cp) { bn_bwd_finalize_block(f, b, threadIdx.x, sm); return; }
        b -= f.cp;
    }
    int j = 0;
    while (j + 1 < t.n && b >= t.start[j + 1]) ++j;
    switch (j) {                                   // (constant indices: the table stays in the kernel-argument registers)
    case 0: wgrad_job_block(t.job[0], b - t.start[0], threadIdx.x, red); break;
    case 1: wgrad_job_block(t.job[1], b - t.start[1], threadIdx.x, red); break;
    case 2: wgrad_job_block(t.job[2], b - t.start[2], threadIdx.x, red); break;
    default: wgrad_job_block(t.job[3], b - t.start[3], threadIdx.x, red); break;
    }
}

template <class T>
__global__ void bn_relu_bwd_apply_kernel(const T* __restrict__ y, int y_cs, T* __restrict__ ga, int g_cs,
                                         int cp, const float* __restrict__ scale, const float* __restrict__ shift,
                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                         const float* __restrict__ coef, int64_t nvox) {
    const int nq = cp >> 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nvox * nq) return;
    const int qd = (int)(idx % nq);
    const int64_t v = idx / nq;
    const float4 sc = *reinterpret_cast<const float4*>(scale + qd * 4);
    const float4 sh = *reinterpret_cast<const float4*>(shift + qd * 4);
    const float4 mu = *reinterpret_cast<const float4*>(mean + qd * 4);
    const float4 is = *reinterpret_cast<const float4*>(invstd + qd * 4);
    const float4 k0 = *reinterpret_cast<const float4*>(coef + qd * 4);
    const float4 k1 = *reinterpret_cast<const float4*>(coef + cp + qd * 4);
    const float4 k2 = *reinterpret_cast<const float4*>(coef + 2 * cp + qd * 4);
    const float4 yy = ld4<T>(y + v * y_cs + qd * 4);
    float4 gg = ld4<T>(ga + v * g_cs + qd * 4);
    float gz;
    gz = (fmaf(yy.x, sc.x, sh.x) > 0.f) ? gg.x : 0.f; gg.x = k0.x * (gz - k1.x - (yy.x - mu.x) * is.x * k2.x);
    gz = (fmaf(yy.y, sc.y, sh.y) > 0.f) ? gg.y : 0.f; gg.y = k0.y * (gz - k1.y - (yy.y - mu.y) * is.y * k2.y);
    gz = (fmaf(yy.z, sc.z, sh.z) > 0.f) ? gg.z : 0.f; gg.z = k0.z * (gz - k1.z - (yy.z - mu.z) * is.z * k2.z);
    gz = (fmaf(yy.w, sc.w, sh.w) > 0.f) ? gg.w : 0.f; gg.w = k0.w * (gz - k1.w - (yy.w - mu.w) * is.w * k2.w);
    st4<T>(ga + v * g_cs + qd * 4, gg);
}

// ------------------------------------------------------------------ MaxPool3d(2,2)
template <class T>
__global__ void maxpool2_fwd_kernel(const T* __restrict__ in, int in_cs, int cp, const float* __restrict__ scale,
                                    const float* __restrict__ shift, int relu, T* __restrict__ out, int out_cs,
                                    int N, int D, int H, int W) {
    const int nq = cp >> 2;
    const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
    const int64_t total = (int64_t)N * Do * Ho * Wo * nq;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int qd = (int)(idx % nq);
    int64_t o = idx / nq;
    const int wo = (int)(o % Wo); o /= Wo;
    const int ho = (int)(o % Ho); o /= Ho;
    const int dd = (int)(o % Do);
    const int n = (int)(o / Do);
    const bool xf = scale != nullptr;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf) {
        sc = *reinterpret_cast<const float4*>(scale + qd * 4);
        sh = *reinterpret_cast<const float4*>(shift + qd * 4);
    }
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int d = dd * 2 + (t >> 2), h = ho * 2 + ((t >> 1) & 1), w = wo * 2 + (t & 1);
        const size_t vox = (((size_t)n * D + d) * H + h) * W + w;
        float4 v = ld4<T>(in + vox * in_cs + qd * 4);
        if (xf) v = xform4(v, sc, sh, relu);
        best.x = fmaxf(best.x, v.x); best.y = fmaxf(best.y, v.y);
        best.z = fmaxf(best.z, v.z); best.w = fmaxf(best.w, v.w);
    }
    const size_t ovox = (((size_t)n * Do + dd) * Ho + ho) * Wo + wo;
    st4<T>(out + ovox * out_cs + qd * 4, best);
}

// ---- additive skip connections (UNet(cat=False), models.py:250-251): out = act(a) + act(b), act = lazy BN + ReLU
template <class T>
__global__ void skip_add_kernel(const T* __restrict__ a, int a_cs, const float* __restrict__ a_scale,
                                const float* __restrict__ a_shift, int a_relu, const T* __restrict__ b, int b_cs,
                                const float* __restrict__ b_scale, const float* __restrict__ b_shift, int b_relu,
                                T* __restrict__ out, int out_cs, int cp, int64_t nvox) {
    const int nq = cp >> 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nvox * nq) return;
    const int qd = (int)(idx % nq);
    const int64_t v = idx / nq;
    float4 x = ld4<T>(a + v * a_cs + qd * 4);
    if (a_scale)
        x = xform4(x, *reinterpret_cast<const float4*>(a_scale + qd * 4), *reinterpret_cast<const float4*>(a_shift + qd * 4), a_relu);
    if (b) {
        float4 y = ld4<T>(b + v * b_cs + qd * 4);
        if (b_scale)
            y = xform4(y, *reinterpret_cast<const float4*>(b_scale + qd * 4), *reinterpret_cast<const float4*>(b_shift + qd * 4), b_relu);
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
    }
    st4<T>(out + v * out_cs + qd * 4, x);
}

// RED: the pooled tensor is relu(BN(raw conv output)) and gin is the gradient w.r.t. that activated tensor, complete once
// this kernel has added its share -- so the BatchNorm-backward reduction of that layer (sum gz, sum gz * xhat per channel,
// gz = gradient masked by the ReLU) rides along: one block-partial row per block, same layout as bn_relu_bwd_reduce.
template <bool RED, class T>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ in, int in_cs, int cp, const float* __restrict__ scale,
                                    const float* __restrict__ shift, int relu, const T* __restrict__ gout,
                                    int gout_cs, T* __restrict__ gin, int gin_cs, int accumulate, int N, int D,
                                    int H, int W, const float* __restrict__ mean, const float* __restrict__ invstd,
                                    float* __restrict__ partials, ctu_bn_bwd_tail tail) {
    const int nq = cp >> 2;
    const int Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
    const int64_t total = (int64_t)N * Do * Ho * Wo * nq;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
    if (idx < total) {
    const int qd = (int)(idx % nq);
    int64_t o = idx / nq;
    const int wo = (int)(o % Wo); o /= Wo;
    const int ho = (int)(o % Ho); o /= Ho;
    const int dd = (int)(o % Do);
    const int n = (int)(o / Do);
    const bool xf = scale != nullptr;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf) {
        sc = *reinterpret_cast<const float4*>(scale + qd * 4);
        sh = *reinterpret_cast<const float4*>(shift + qd * 4);
    }
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu;
    if constexpr (RED) {
        mu = *reinterpret_cast<const float4*>(mean + qd * 4);
        is = *reinterpret_cast<const float4*>(invstd + qd * 4);
    }
    float4 raw[8];
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    int bi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int d = dd * 2 + (t >> 2), h = ho * 2 + ((t >> 1) & 1), w = wo * 2 + (t & 1);
        const size_t vox = (((size_t)n * D + d) * H + h) * W + w;
        float4 v = ld4<T>(in + vox * in_cs + qd * 4);
        raw[t] = v;
        if (xf) v = xform4(v, sc, sh, relu);
        // first maximum in (d,h,w) scan order wins, as ATen's max_pool3d does (strict >)
        if (v.x > best.x) { best.x = v.x; bi[0] = t; }
        if (v.y > best.y) { best.y = v.y; bi[1] = t; }
        if (v.z > best.z) { best.z = v.z; bi[2] = t; }
        if (v.w > best.w) { best.w = v.w; bi[3] = t; }
    }
    const size_t ovox = (((size_t)n * Do + dd) * Ho + ho) * Wo + wo;
    const float4 g = ld4<T>(gout + ovox * gout_cs + qd * 4);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int d = dd * 2 + (t >> 2), h = ho * 2 + ((t >> 1) & 1), w = wo * 2 + (t & 1);
        const size_t vox = (((size_t)n * D + d) * H + h) * W + w;
        T* gp = gin + vox * gin_cs + qd * 4;
        float4 r = accumulate ? ld4<T>(gp) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (bi[0] == t) r.x += g.x;
        if (bi[1] == t) r.y += g.y;
        if (bi[2] == t) r.z += g.z;
        if (bi[3] == t) r.w += g.w;
        r = rnd4<T>(r);                      // the reduction sees what the BatchNorm-backward apply pass will read back
        st4<T>(gp, r);
        if constexpr (RED) {
            const float4 y = raw[t];
            float gz;
            gz = (fmaf(y.x, sc.x, sh.x) > 0.f) ? r.x : 0.f; a1.x += gz; a2.x += gz * (y.x - mu.x) * is.x;
            gz = (fmaf(y.y, sc.y, sh.y) > 0.f) ? r.y : 0.f; a1.y += gz; a2.y += gz * (y.y - mu.y) * is.y;
            gz = (fmaf(y.z, sc.z, sh.z) > 0.f) ? r.z : 0.f; a1.z += gz; a2.z += gz * (y.z - mu.z) * is.z;
            gz = (fmaf(y.w, sc.w, sh.w) > 0.f) ? r.w : 0.f; a1.w += gz; a2.w += gz * (y.w - mu.w) * is.w;
        }
    }
    }
    if constexpr (RED) {
        // thread t < cp sums channel t over the block's voxel lanes in a fixed order (threadIdx % nq is the channel quad)
        __shared__ float red[EW_BLOCK * 8];
        float* r = &red[threadIdx.x * 8];
        r[0] = a1.x; r[1] = a1.y; r[2] = a1.z; r[3] = a1.w; r[4] = a2.x; r[5] = a2.y; r[6] = a2.z; r[7] = a2.w;
        __syncthreads();
        if (threadIdx.x < cp) {
            const int c = threadIdx.x, q = c >> 2, j = c & 3;
            float s1 = 0.f, s2 = 0.f;
            for (int l = 0; l < EW_BLOCK / nq; ++l) {
                s1 += red[(l * nq + q) * 8 + j];
                s2 += red[(l * nq + q) * 8 + 4 + j];
            }
            st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + c, s1);
            st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + cp + c, s2);
        }
        if (tail.counter) bn_bwd_tail(tail, partials, gridDim.x, cp, gridDim.x);
    }
}

// ---- MaxPool3d(2,2) with lanes along the FINE row (cp / 4 a power of two <= 32; the kernels above serve every other width).
// A coarse row is one (n, do, ho); its flat positions are (w, quad) of the fine grid, W * nq of them, and a thread owns one
// position for the row's four (d, h) planes -- so every load or store instruction of a wave covers one contiguous run of a
// fine row (the kernels above touch every second voxel per instruction).  The two w of a window sit nq lanes apart in one
// wave (W is even and 2 nq divides 64): each lane reduces its own w over (d, h) with strict >, then the pair exchanges
// {maximum, its (d, h) index} once.  Grid-stride over positions (the backward with reduction rows: two trips per block, one
// block per row): every stride is a multiple of nq, so a thread keeps its channel quad and that quad's constants stay in
// registers.
struct PoolRows { unsigned total, rowlen; int lg_nq, Do, Ho; };      // positions overall / per coarse row, log2(nq)

__device__ __forceinline__ void pool_row_decode(const PoolRows& g, unsigned f, int D, int H, int W, size_t& vox,
                                                size_t& ovox) {
    const unsigned r = f / g.rowlen, w = (f - r * g.rowlen) >> g.lg_nq;
    const unsigned ho = r % (unsigned)g.Ho, nd = r / (unsigned)g.Ho;                  // nd = n * Do + do
    const unsigned dd = nd % (unsigned)g.Do, n = nd / (unsigned)g.Do;
    vox = (((size_t)n * D + dd * 2) * H + ho * 2) * W + w;                            // plane (d, h) = (0, 0) of the window
    ovox = (size_t)r * (W >> 1) + (w >> 1);
}

template <class T>
__global__ __launch_bounds__(EW_BLOCK) void maxpool2_fwd_row_kernel(const T* __restrict__ in, int in_cs,
                                                                     const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, int relu,
                                                                     T* __restrict__ out, int out_cs, int D, int H, int W,
                                                                     PoolRows g) {
    const int nq = 1 << g.lg_nq, qd = threadIdx.x & (nq - 1);
    const bool xf = scale != nullptr;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf) {
        sc = *reinterpret_cast<const float4*>(scale + qd * 4);
        sh = *reinterpret_cast<const float4*>(shift + qd * 4);
    }
    const bool upper = (threadIdx.x & nq) != 0;                                       // this lane holds the odd w of its window
    for (unsigned f = blockIdx.x * EW_BLOCK + threadIdx.x; f < g.total; f += gridDim.x * EW_BLOCK) {
        size_t vox, ovox;
        pool_row_decode(g, f, D, H, W, vox, ovox);
        float4 v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            v[t] = ld4<T>(in + (vox + ((size_t)(t >> 1) * H + (t & 1)) * W) * in_cs + qd * 4);
        float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 a = xf ? xform4(v[t], sc, sh, relu) : v[t];
            best.x = fmaxf(best.x, a.x); best.y = fmaxf(best.y, a.y);
            best.z = fmaxf(best.z, a.z); best.w = fmaxf(best.w, a.w);
        }
        best.x = fmaxf(best.x, __shfl_xor(best.x, nq)); best.y = fmaxf(best.y, __shfl_xor(best.y, nq));
        best.z = fmaxf(best.z, __shfl_xor(best.z, nq)); best.w = fmaxf(best.w, __shfl_xor(best.w, nq));
        if (!upper) st4<T>(out + ovox * out_cs + qd * 4, best);
    }
}

template <bool RED, class T>
__global__ __launch_bounds__(EW_BLOCK) void maxpool2_bwd_row_kernel(const T* __restrict__ in, int in_cs, int cp,
                                                                     const float* __restrict__ scale,
                                                                     const float* __restrict__ shift, int relu,
                                                                     const T* __restrict__ gout, int gout_cs,
                                                                     T* __restrict__ gin, int gin_cs, int accumulate, int D,
                                                                     int H, int W, PoolRows g, const float* __restrict__ mean,
                                                                     const float* __restrict__ invstd,
                                                                     float* __restrict__ partials, ctu_bn_bwd_tail tail) {
    const int nq = 1 << g.lg_nq, qd = threadIdx.x & (nq - 1);
    const bool xf = scale != nullptr;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf) {
        sc = *reinterpret_cast<const float4*>(scale + qd * 4);
        sh = *reinterpret_cast<const float4*>(shift + qd * 4);
    }
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu;
    if constexpr (RED) {
        mu = *reinterpret_cast<const float4*>(mean + qd * 4);
        is = *reinterpret_cast<const float4*>(invstd + qd * 4);
    }
    const bool upper = (threadIdx.x & nq) != 0;
    // RED: a block owns 2 * EW_BLOCK consecutive positions = the EW_BLOCK (pooled voxel, quad) items of one partial row of
    // the kernel above, and sums them in that kernel's order, so the rows are the same bit for bit (what is trained from
    // them does not depend on which kernel ran); red holds the items' sums.
    __shared__ float red[RED ? EW_BLOCK * 8 : 1];
    if constexpr (RED) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = 0.f;
        __syncthreads();
    }
    constexpr unsigned PER = RED ? 2 * EW_BLOCK : EW_BLOCK;
    const unsigned stride = RED ? EW_BLOCK : gridDim.x * EW_BLOCK;
    const unsigned stop = RED ? min(g.total, (blockIdx.x + 1) * PER) : g.total;
    unsigned slot = threadIdx.x;                                                      // position inside the block's row (RED)
    for (unsigned f = blockIdx.x * PER + threadIdx.x; f < stop; f += stride, slot += EW_BLOCK) {
        size_t vox, ovox;
        pool_row_decode(g, f, D, H, W, vox, ovox);
        float4 raw[4], r[4], gz[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            raw[t] = ld4<T>(in + (vox + ((size_t)(t >> 1) * H + (t & 1)) * W) * in_cs + qd * 4);
        const float4 go = ld4<T>(gout + ovox * gout_cs + qd * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            r[t] = accumulate ? ld4<T>(gin + (vox + ((size_t)(t >> 1) * H + (t & 1)) * W) * gin_cs + qd * 4)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
        // first maximum in (d, h, w) scan order wins, as ATen's max_pool3d does: strict > over this lane's (d, h) ...
        float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        int bx = 0, by = 0, bz = 0, bw = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 a = xf ? xform4(raw[t], sc, sh, relu) : raw[t];
            if (a.x > best.x) { best.x = a.x; bx = t; }
            if (a.y > best.y) { best.y = a.y; by = t; }
            if (a.z > best.z) { best.z = a.z; bz = t; }
            if (a.w > best.w) { best.w = a.w; bw = t; }
        }
        // ... then between the two w: scan position 2 (d, h) + w, so on equal maxima the odd w wins only with a strictly
        // smaller (d, h) index
        const int mine = bx | (by << 2) | (bz << 4) | (bw << 6);
        const int theirs = __shfl_xor(mine, nq);
        const float4 ob = make_float4(__shfl_xor(best.x, nq), __shfl_xor(best.y, nq), __shfl_xor(best.z, nq),
                                      __shfl_xor(best.w, nq));
        const int ox = theirs & 3, oy = (theirs >> 2) & 3, oz = (theirs >> 4) & 3, ow = (theirs >> 6) & 3;
        const bool wx = upper ? (best.x > ob.x || (best.x == ob.x && bx < ox)) : !(ob.x > best.x || (ob.x == best.x && ox < bx));
        const bool wy = upper ? (best.y > ob.y || (best.y == ob.y && by < oy)) : !(ob.y > best.y || (ob.y == best.y && oy < by));
        const bool wz = upper ? (best.z > ob.z || (best.z == ob.z && bz < oz)) : !(ob.z > best.z || (ob.z == best.z && oz < bz));
        const bool ww = upper ? (best.w > ob.w || (best.w == ob.w && bw < ow)) : !(ob.w > best.w || (ob.w == best.w && ow < bw));
        if (!wx) bx = -1;
        if (!wy) by = -1;
        if (!wz) bz = -1;
        if (!ww) bw = -1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float4 o = r[t];
            if (bx == t) o.x += go.x;
            if (by == t) o.y += go.y;
            if (bz == t) o.z += go.z;
            if (bw == t) o.w += go.w;
            o = rnd4<T>(o);                      // the reduction sees what the BatchNorm-backward apply pass will read back
            st4<T>(gin + (vox + ((size_t)(t >> 1) * H + (t & 1)) * W) * gin_cs + qd * 4, o);
            if constexpr (RED) {
                const float4 y = raw[t];
                gz[t].x = (fmaf(y.x, sc.x, sh.x) > 0.f) ? o.x : 0.f; gz[t].y = (fmaf(y.y, sc.y, sh.y) > 0.f) ? o.y : 0.f;
                gz[t].z = (fmaf(y.z, sc.z, sh.z) > 0.f) ? o.z : 0.f; gz[t].w = (fmaf(y.w, sc.w, sh.w) > 0.f) ? o.w : 0.f;
            }
        }
        if constexpr (RED) {
            // the window's eight terms in scan order, (d, h) outer and w inner: the even-w lane takes the odd-w lane's
            // four {masked gradient, raw value} and sums for the pair
            float4 a1 = make_float4(0.f, 0.f, 0.f, 0.f), a2 = a1;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float4 y = raw[t];
                float4 z = gz[t];
                const float4 yo = make_float4(__shfl_xor(y.x, nq), __shfl_xor(y.y, nq), __shfl_xor(y.z, nq), __shfl_xor(y.w, nq));
                const float4 zo = make_float4(__shfl_xor(z.x, nq), __shfl_xor(z.y, nq), __shfl_xor(z.z, nq), __shfl_xor(z.w, nq));
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    float gz_;
                    gz_ = z.x; a1.x += gz_; a2.x += gz_ * (y.x - mu.x) * is.x;
                    gz_ = z.y; a1.y += gz_; a2.y += gz_ * (y.y - mu.y) * is.y;
                    gz_ = z.z; a1.z += gz_; a2.z += gz_ * (y.z - mu.z) * is.z;
                    gz_ = z.w; a1.w += gz_; a2.w += gz_ * (y.w - mu.w) * is.w;
                    y = yo; z = zo;
                }
            }
            if (!upper) {
                float* r_ = &red[(((slot >> (g.lg_nq + 1)) << g.lg_nq) + qd) * 8];      // item = pooled voxel of the row * nq + quad
                r_[0] = a1.x; r_[1] = a1.y; r_[2] = a1.z; r_[3] = a1.w; r_[4] = a2.x; r_[5] = a2.y; r_[6] = a2.z; r_[7] = a2.w;
            }
        }
    }
    if constexpr (RED) {
        // thread t < cp sums channel t over the row's items in a fixed order
        __syncthreads();
        if (threadIdx.x < cp) {
            const int c = threadIdx.x, q = c >> 2, j = c & 3;
            float s1 = 0.f, s2 = 0.f;
            for (int l = 0; l < EW_BLOCK / nq; ++l) {
                s1 += red[(l * nq + q) * 8 + j];
                s2 += red[(l * nq + q) * 8 + 4 + j];
            }
            st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + c, s1);
            st_row(tail.counter != nullptr, partials + (size_t)blockIdx.x * 2 * cp + cp + c, s2);
        }
        if (tail.counter) bn_bwd_tail(tail, partials, gridDim.x, cp, gridDim.x);
    }
}

// ------------------------------------------------------------------ channel sums
// block bodies in channel_sum.h (the fused up-convolution's projection runs them inside its own launches)
template <class T>
__global__ void channel_sum_partial_kernel(const T* __restrict__ x, int cs, int cp, int64_t nvox,
                                           float* __restrict__ partials) {
    __shared__ float red[EW_BLOCK * 4];
    channel_sum_partial_block<T>(x, cs, cp, nvox, partials, blockIdx.x, gridDim.x, red);
}

// one block per channel, fixed-order tree -> deterministic
__global__ void channel_sum_final_kernel(const float* __restrict__ partials, int nb, int cp, float* __restrict__ out,
                                         int C) {
    __shared__ double r[EW_BLOCK];
    const float s = channel_sum_final_block(partials, nb, cp, blockIdx.x, r);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

}  // namespace

// =================================================================== C ABI
// The activation-touching entry points exist twice: the fp32 ones (float*) and ctu_lp_* (dtype code + void*, 16-bit
// storage); both are thin wrappers over one template per operation.
namespace {

template <class T>
int ncdhw_to_ndhwc_impl(const float* src, T* dst, int N, int C, int D, int H, int W, int cp, int cs, void* stream) {
    CTU_REQUIRE(src && dst && N > 0 && C > 0, "ncdhw_to_ndhwc: null/empty");
    CTU_REQUIRE(cp % 8 == 0 && cp >= C && cs >= cp && cs % 4 == 0, "ncdhw_to_ndhwc: cp=%d cs=%d C=%d", cp, cs, C);
    const int64_t V = (int64_t)D * H * W, tv = V * N;
    const int64_t total = tv * (cp >> 2);
    ncdhw_to_ndhwc_kernel<T><<<(unsigned)ceil_div64(total, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(src, dst, C, V, tv, cp, cs);
    CTU_CHECK_LAUNCH("ncdhw_to_ndhwc");
    return CTU_OK;
}

template <class T>
int ndhwc_to_ncdhw_impl(const T* src, float* dst, int N, int C, int D, int H, int W, int cs, void* stream) {
    CTU_REQUIRE(src && dst && N > 0 && C > 0 && cs >= C, "ndhwc_to_ncdhw: bad argument");
    const int64_t V = (int64_t)D * H * W, tv = V * N;
    ndhwc_to_ncdhw_kernel<T><<<(unsigned)ceil_div64(tv * C, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(src, dst, C, V, tv, cs);
    CTU_CHECK_LAUNCH("ndhwc_to_ncdhw");
    return CTU_OK;
}

template <class T>
int bn_relu_bwd_reduce_impl(const T* y, int y_cs, const T* ga, int g_cs, int cp, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int64_t nvox, float* partials, const ctu_bn_bwd_tail* tail,
                            void* stream) {
    CTU_REQUIRE(y && ga && scale && shift && mean && invstd && partials, "bn_relu_bwd_reduce: null pointer");
    CTU_REQUIRE(!tail || (tail->counter && tail->gamma && tail->invstd && tail->dgamma && tail->dbeta && tail->coef &&
                          tail->C > 0 && tail->C <= cp && tail->count > 0 && (!tail->running_mean || (tail->mean && tail->running_var))),
                "bn_relu_bwd_reduce: incomplete BatchNorm tail");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0 && cp <= 256 && y_cs % 4 == 0 && g_cs % 4 == 0, "bn_relu_bwd_reduce: cp=%d", cp);
    bn_relu_bwd_reduce_kernel<T><<<ctu_bn_bwd_num_blocks(nvox), EW_BLOCK, 0, (hipStream_t)stream>>>(
        y, y_cs, ga, g_cs, cp, scale, shift, mean, invstd, nvox, partials, bwd_tail_or_off(tail));
    CTU_CHECK_LAUNCH("bn_relu_bwd_reduce");
    return CTU_OK;
}

template <class T>
int bn_relu_bwd_apply_impl(const T* y, int y_cs, T* ga, int g_cs, int cp, const float* scale, const float* shift,
                           const float* mean, const float* invstd, const float* coef, int64_t nvox, void* stream) {
    CTU_REQUIRE(y && ga && scale && shift && mean && invstd && coef, "bn_relu_bwd_apply: null pointer");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0, "bn_relu_bwd_apply: cp=%d", cp);
    const int64_t total = nvox * (cp >> 2);
    bn_relu_bwd_apply_kernel<T><<<(unsigned)ceil_div64(total, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(
        y, y_cs, ga, g_cs, cp, scale, shift, mean, invstd, coef, nvox);
    CTU_CHECK_LAUNCH("bn_relu_bwd_apply");
    return CTU_OK;
}

// launch shape of the row kernels: rows.total = 0 where they do not apply (cp / 4 not a power of two <= 32, or more positions
// than 32-bit indices hold) and the (pooled voxel, quad) kernels run instead.  nb: at most 8 resident blocks per CU (the
// backward with reduction rows launches ctu_maxpool2_bwd_bn_num_blocks blocks instead, one per row).
struct PoolPlan { PoolRows rows; int nb; };
PoolPlan pool_plan(int N, int D, int H, int W, int cp) {
    PoolPlan p = {};
    const int nq = cp >> 2;
    const int64_t total = (int64_t)N * (D / 2) * (H / 2) * W * nq;
    if (nq > 32 || (nq & (nq - 1)) != 0 || total <= 0 || total >= ((int64_t)1 << 31)) return p;
    while ((1 << p.rows.lg_nq) < nq) ++p.rows.lg_nq;
    p.rows.total = (unsigned)total;
    p.rows.rowlen = (unsigned)(W * nq);
    p.rows.Do = D / 2;
    p.rows.Ho = H / 2;
    const int64_t nb = ceil_div64(total, EW_BLOCK);
    p.nb = (int)(nb > 2048 ? 2048 : nb);
    return p;
}

template <class T>
int maxpool2_fwd_impl(const T* in, int in_cs, int cp, const float* in_scale, const float* in_shift, int in_relu, T* out,
                      int out_cs, int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(in && out, "maxpool2_fwd: null pointer");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "maxpool2_fwd: D,H,W must be even");
    const PoolPlan pl = pool_plan(N, D, H, W, cp);
    if (pl.rows.total) {
        maxpool2_fwd_row_kernel<T><<<pl.nb, EW_BLOCK, 0, (hipStream_t)stream>>>(in, in_cs, in_scale, in_shift, in_relu, out, out_cs,
                                                                                D, H, W, pl.rows);
    } else {
        const int64_t total = (int64_t)N * (D / 2) * (H / 2) * (W / 2) * (cp >> 2);
        maxpool2_fwd_kernel<T><<<(unsigned)ceil_div64(total, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(
            in, in_cs, cp, in_scale, in_shift, in_relu, out, out_cs, N, D, H, W);
    }
    CTU_CHECK_LAUNCH("maxpool2_fwd");
    return CTU_OK;
}

template <class T>
int maxpool2_bwd_impl(const T* in, int in_cs, int cp, const float* in_scale, const float* in_shift, int in_relu, const T* gout,
                      int gout_cs, T* gin, int gin_cs, int accumulate, int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(in && gout && gin, "maxpool2_bwd: null pointer");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "maxpool2_bwd: D,H,W must be even");
    const PoolPlan pl = pool_plan(N, D, H, W, cp);
    if (pl.rows.total) {
        maxpool2_bwd_row_kernel<false, T><<<pl.nb, EW_BLOCK, 0, (hipStream_t)stream>>>(
            in, in_cs, cp, in_scale, in_shift, in_relu, gout, gout_cs, gin, gin_cs, accumulate, D, H, W, pl.rows, nullptr, nullptr,
            nullptr, bwd_tail_or_off(nullptr));
    } else {
        const int64_t total = (int64_t)N * (D / 2) * (H / 2) * (W / 2) * (cp >> 2);
        maxpool2_bwd_kernel<false, T><<<(unsigned)ceil_div64(total, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(
            in, in_cs, cp, in_scale, in_shift, in_relu, gout, gout_cs, gin, gin_cs, accumulate, N, D, H, W, nullptr, nullptr, nullptr,
            bwd_tail_or_off(nullptr));
    }
    CTU_CHECK_LAUNCH("maxpool2_bwd");
    return CTU_OK;
}

template <class T>
int maxpool2_bwd_bn_impl(const T* in, int in_cs, int cp, const float* in_scale, const float* in_shift, const float* mean,
                         const float* invstd, const T* gout, int gout_cs, T* gin, int gin_cs, int accumulate, int N, int D,
                         int H, int W, float* partials, const ctu_bn_bwd_tail* tail, void* stream) {
    CTU_REQUIRE(in && gout && gin && in_scale && in_shift && mean && invstd && partials, "maxpool2_bwd_bn: null pointer");
    CTU_REQUIRE(!tail || (tail->counter && tail->gamma && tail->invstd && tail->dgamma && tail->dbeta && tail->coef &&
                          tail->C > 0 && tail->C <= cp && tail->count > 0 && (!tail->running_mean || (tail->mean && tail->running_var))),
                "maxpool2_bwd_bn: incomplete BatchNorm tail");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0 && cp <= EW_BLOCK && EW_BLOCK % (cp >> 2) == 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0,
                "maxpool2_bwd_bn: cp=%d must be a multiple of 8 whose quads divide the block; D,H,W even", cp);
    const int nb = ctu_maxpool2_bwd_bn_num_blocks(N, D, H, W, cp);
    const PoolPlan pl = pool_plan(N, D, H, W, cp);
    if (pl.rows.total)
        maxpool2_bwd_row_kernel<true, T><<<nb, EW_BLOCK, 0, (hipStream_t)stream>>>(
            in, in_cs, cp, in_scale, in_shift, 1, gout, gout_cs, gin, gin_cs, accumulate, D, H, W, pl.rows, mean, invstd, partials,
            bwd_tail_or_off(tail));
    else
        maxpool2_bwd_kernel<true, T><<<nb, EW_BLOCK, 0, (hipStream_t)stream>>>(
            in, in_cs, cp, in_scale, in_shift, 1, gout, gout_cs, gin, gin_cs, accumulate, N, D, H, W, mean, invstd, partials,
            bwd_tail_or_off(tail));
    CTU_CHECK_LAUNCH("maxpool2_bwd_bn");
    return CTU_OK;
}

template <class T>
int skip_add_impl(const T* a, int a_cs, const float* a_scale, const float* a_shift, int a_relu, const T* b, int b_cs,
                  const float* b_scale, const float* b_shift, int b_relu, T* out, int out_cs, int cp, int64_t nvox, void* stream) {
    CTU_REQUIRE(a && out, "skip_add: null pointer");
    CTU_REQUIRE(cp % 4 == 0 && cp > 0 && a_cs % 4 == 0 && out_cs % 4 == 0 && (!b || b_cs % 4 == 0), "skip_add: channel counts / strides must be multiples of 4");
    CTU_REQUIRE((a_scale == nullptr) == (a_shift == nullptr) && (b_scale == nullptr) == (b_shift == nullptr), "skip_add: scale/shift come in pairs");
    if (nvox <= 0) return CTU_OK;
    const int64_t total = nvox * (cp >> 2);
    skip_add_kernel<T><<<(unsigned)ceil_div64(total, EW_BLOCK), EW_BLOCK, 0, (hipStream_t)stream>>>(
        a, a_cs, a_scale, a_shift, a_relu, b, b_cs, b_scale, b_shift, b_relu, out, out_cs, cp, nvox);
    CTU_CHECK_LAUNCH("skip_add");
    return CTU_OK;
}

template <class T>
int channel_sum_impl(const T* x, int cs, int cp, int64_t nvox, float* partials, float* out, int C, void* stream) {
    CTU_REQUIRE(x && partials && out, "channel_sum: null pointer");
    CTU_REQUIRE(cp % 8 == 0 && cp > 0 && cp <= 256 && C <= cp && cs % 4 == 0, "channel_sum: cp=%d", cp);
    const int nb = ctu_channel_sum_num_blocks(nvox);
    channel_sum_partial_kernel<T><<<nb, EW_BLOCK, 0, (hipStream_t)stream>>>(x, cs, cp, nvox, partials);
    CTU_CHECK_LAUNCH("channel_sum_partial");
    channel_sum_final_kernel<<<C, EW_BLOCK, 0, (hipStream_t)stream>>>(partials, nb, cp, out, C);
    CTU_CHECK_LAUNCH("channel_sum_final");
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_ncdhw_to_ndhwc(const float* src, float* dst, int N, int C, int D, int H, int W, int cp, int cs,
                                  void* stream) {
    return ncdhw_to_ndhwc_impl<float>(src, dst, N, C, D, H, W, cp, cs, stream);
}
extern "C" int ctu_lp_ncdhw_to_ndhwc(int dtype, const float* src, void* dst, int N, int C, int D, int H, int W, int cp, int cs,
                                     void* stream) {
    CTU_DISPATCH_LP(dtype, return ncdhw_to_ndhwc_impl<T>(src, (T*)dst, N, C, D, H, W, cp, cs, stream));
}

extern "C" int ctu_ndhwc_to_ncdhw(const float* src, float* dst, int N, int C, int D, int H, int W, int cs,
                                  void* stream) {
    return ndhwc_to_ncdhw_impl<float>(src, dst, N, C, D, H, W, cs, stream);
}
extern "C" int ctu_lp_ndhwc_to_ncdhw(int dtype, const void* src, float* dst, int N, int C, int D, int H, int W, int cs,
                                     void* stream) {
    CTU_DISPATCH_LP(dtype, return ndhwc_to_ncdhw_impl<T>((const T*)src, dst, N, C, D, H, W, cs, stream));
}

extern "C" int ctu_bn_finalize(const float* stats, int nblocks, int C, int cp, double count, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                               int n_updates, float* scale, float* shift, float* mean_out, float* invstd_out,
                               long long* num_batches_tracked, void* stream) {
    CTU_REQUIRE(stats && gamma && beta && scale && shift && mean_out && invstd_out, "bn_finalize: null pointer");
    CTU_REQUIRE(C > 0 && cp >= C && cp % 8 == 0 && nblocks > 0 && count > 0, "bn_finalize: bad sizes");
    bn_finalize_kernel<<<cp, FIN_BLOCK, 0, (hipStream_t)stream>>>(stats, nblocks, C, cp, count, gamma, beta,
                                                                running_mean, running_var, momentum, eps, n_updates,
                                                                scale, shift, mean_out, invstd_out, num_batches_tracked);
    CTU_CHECK_LAUNCH("bn_finalize");
    return CTU_OK;
}

extern "C" int ctu_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, int C, int cp, float* scale, float* shift,
                                  void* stream) {
    CTU_REQUIRE(gamma && beta && running_mean && running_var && scale && shift, "bn_eval_affine: null pointer");
    CTU_REQUIRE(C > 0 && cp >= C && cp % 8 == 0, "bn_eval_affine: bad sizes");
    bn_eval_affine_kernel<<<ceil_div(cp, 64), 64, 0, (hipStream_t)stream>>>(gamma, beta, running_mean, running_var,
                                                                           eps, C, cp, scale, shift);
    CTU_CHECK_LAUNCH("bn_eval_affine");
    return CTU_OK;
}

extern "C" int ctu_bn_bwd_num_blocks(int64_t nvox) {
    int64_t nb = ceil_div64(nvox, 64);
    if (nb > MAX_RED_BLOCKS) nb = MAX_RED_BLOCKS;
    if (nb < 1) nb = 1;
    return (int)nb;
}

extern "C" int ctu_bn_relu_bwd_reduce(const float* y, int y_cs, const float* ga, int g_cs, int cp, const float* scale,
                                      const float* shift, const float* mean, const float* invstd, int64_t nvox,
                                      float* partials, const ctu_bn_bwd_tail* tail, void* stream) {
    return bn_relu_bwd_reduce_impl<float>(y, y_cs, ga, g_cs, cp, scale, shift, mean, invstd, nvox, partials, tail, stream);
}
extern "C" int ctu_lp_bn_relu_bwd_reduce(int dtype, const void* y, int y_cs, const void* ga, int g_cs, int cp, const float* scale,
                                         const float* shift, const float* mean, const float* invstd, int64_t nvox,
                                         float* partials, const ctu_bn_bwd_tail* tail, void* stream) {
    CTU_DISPATCH_LP(dtype, return bn_relu_bwd_reduce_impl<T>((const T*)y, y_cs, (const T*)ga, g_cs, cp, scale, shift, mean, invstd,
                                                             nvox, partials, tail, stream));
}

// the job table of a merged launch: the non-empty jobs and their block ranges; *nblocks = blocks of all of them
static int wgrad_job_table(const ctu_wgrad_job* jobs, int njobs, WgJobTable* t, int* nblocks, const char* what) {
    CTU_REQUIRE(njobs >= 0 && njobs <= CTU_WGRAD_JOBS_MAX, "%s: njobs=%d (0 .. %d)", what, njobs, CTU_WGRAD_JOBS_MAX);
    CTU_REQUIRE(njobs == 0 || jobs, "%s: null job table", what);
    *t = WgJobTable{};
    int n = 0, total = 0;
    for (int i = 0; i < njobs; ++i) {
        const ctu_wgrad_job& j = jobs[i];
        if (j.kind == 0) continue;
        CTU_REQUIRE(j.kind > 0 && j.kind < WGJ_KINDS, "%s: job %d has unknown kind %d", what, i, j.kind);
        CTU_REQUIRE(j.ws && j.dw, "%s: job %d: null pointer", what, i);
        CTU_REQUIRE(((uintptr_t)j.ws & 3) == 0 && ((uintptr_t)j.dw & 3) == 0 && ((uintptr_t)j.db & 3) == 0 && ((uintptr_t)j.cinv & 3) == 0,
                    "%s: job %d: pointers must be 4-byte aligned", what, i);
        CTU_REQUIRE(j.Co > 0 && j.Ci > 0 && j.gx > 0 && j.pairs > 0 && j.nmf > 0 && j.nmf <= 32 && j.pairs <= 65535,
                    "%s: job %d: bad geometry", what, i);
        CTU_REQUIRE(j.kind >= WGJ_FIRST || (j.n_ci_g > 0 && j.cin_p > 0), "%s: job %d: bad channel groups", what, i);
        CTU_REQUIRE(j.kind < WGJ_CONVT || (j.n_ci_g > 0 && (int64_t)j.Ci * j.Co * 8 + j.Co < (1LL << 31)), "%s: job %d: bad ConvTranspose job", what, i);
        t->job[n] = j;
        t->start[n] = total;
        total += wgrad_job_blocks(j);
        ++n;
    }
    for (int i = n; i <= CTU_WGRAD_JOBS_MAX; ++i) t->start[i] = total;
    t->n = n;
    *nblocks = total;
    return CTU_OK;
}

static int bn_bwd_fin_args(BnBwdFinArgs* f, const float* partials, int nb, int C, int cp, double count, const float* gamma,
                           const float* invstd, float* dgamma, float* dbeta, float* coef, const float* mean,
                           float* running_mean, float* running_var, float momentum, float eps,
                           long long* num_batches_tracked) {
    CTU_REQUIRE(partials && gamma && invstd && dgamma && dbeta && coef && mean, "bn_bwd_finalize: null pointer");
    CTU_REQUIRE((running_mean == nullptr) == (running_var == nullptr) && (!running_mean || mean),
                "bn_bwd_finalize: the running-stat replay needs mean, running_mean and running_var together");
    *f = BnBwdFinArgs{partials, gamma, invstd, mean, dgamma, dbeta, coef, running_mean, running_var, num_batches_tracked,
                      count, momentum, eps, nb, C, cp};
    return CTU_OK;
}

extern "C" int ctu_bn_bwd_finalize(const float* partials, int nb, int C, int cp, double count, const float* gamma,
                                   const float* invstd, float* dgamma, float* dbeta, float* coef, const float* mean,
                                   float* running_mean, float* running_var, float momentum, float eps,
                                   long long* num_batches_tracked, void* stream) {
    BnBwdFinArgs f;
    const int rc = bn_bwd_fin_args(&f, partials, nb, C, cp, count, gamma, invstd, dgamma, dbeta, coef, mean, running_mean,
                                   running_var, momentum, eps, num_batches_tracked);
    if (rc != CTU_OK) return rc;
    bn_bwd_finalize_kernel<<<cp, EW_BLOCK, 0, (hipStream_t)stream>>>(f);
    CTU_CHECK_LAUNCH("bn_bwd_finalize");
    return CTU_OK;
}

extern "C" int ctu_bn_bwd_finalize_jobs(const float* partials, int nb, int C, int cp, double count, const float* gamma,
                                        const float* invstd, float* dgamma, float* dbeta, float* coef, const float* mean,
                                        float* running_mean, float* running_var, float momentum, float eps,
                                        long long* num_batches_tracked, const ctu_wgrad_job* jobs, int njobs, void* stream) {
    BnBwdFinArgs f;
    int rc = bn_bwd_fin_args(&f, partials, nb, C, cp, count, gamma, invstd, dgamma, dbeta, coef, mean, running_mean,
                             running_var, momentum, eps, num_batches_tracked);
    if (rc != CTU_OK) return rc;
    CTU_REQUIRE(cp > 0 && C <= cp && nb >= 0, "bn_bwd_finalize_jobs: C=%d cp=%d nb=%d", C, cp, nb);
    WgJobTable t;
    int nblocks = 0;
    rc = wgrad_job_table(jobs, njobs, &t, &nblocks, "bn_bwd_finalize_jobs");
    if (rc != CTU_OK) return rc;
    if (nblocks == 0) bn_bwd_finalize_kernel<<<cp, EW_BLOCK, 0, (hipStream_t)stream>>>(f);      // exactly ctu_bn_bwd_finalize
    else wgrad_reduce_jobs_kernel<true><<<cp + nblocks, 64 * RPARTS, 0, (hipStream_t)stream>>>(f, t);
    CTU_CHECK_LAUNCH("bn_bwd_finalize_jobs");
    return CTU_OK;
}

extern "C" int ctu_wgrad_reduce_jobs(const ctu_wgrad_job* jobs, int njobs, void* stream) {
    WgJobTable t;
    int nblocks = 0;
    const int rc = wgrad_job_table(jobs, njobs, &t, &nblocks, "wgrad_reduce_jobs");
    if (rc != CTU_OK) return rc;
    if (nblocks == 0) return CTU_OK;
    wgrad_reduce_jobs_kernel<false><<<nblocks, 64 * RPARTS, 0, (hipStream_t)stream>>>(BnBwdFinArgs{}, t);
    CTU_CHECK_LAUNCH("wgrad_reduce_jobs");
    return CTU_OK;
}

extern "C" int ctu_bn_relu_bwd_apply(const float* y, int y_cs, float* ga, int g_cs, int cp, const float* scale,
                                     const float* shift, const float* mean, const float* invstd, const float* coef,
                                     int64_t nvox, void* stream) {
    return bn_relu_bwd_apply_impl<float>(y, y_cs, ga, g_cs, cp, scale, shift, mean, invstd, coef, nvox, stream);
}
extern "C" int ctu_lp_bn_relu_bwd_apply(int dtype, const void* y, int y_cs, void* ga, int g_cs, int cp, const float* scale,
                                        const float* shift, const float* mean, const float* invstd, const float* coef,
                                        int64_t nvox, void* stream) {
    CTU_DISPATCH_LP(dtype, return bn_relu_bwd_apply_impl<T>((const T*)y, y_cs, (T*)ga, g_cs, cp, scale, shift, mean, invstd, coef,
                                                            nvox, stream));
}

extern "C" int ctu_maxpool2_fwd(const float* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                int in_relu, float* out, int out_cs, int N, int D, int H, int W, void* stream) {
    return maxpool2_fwd_impl<float>(in, in_cs, cp, in_scale, in_shift, in_relu, out, out_cs, N, D, H, W, stream);
}
extern "C" int ctu_lp_maxpool2_fwd(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                   int in_relu, void* out, int out_cs, int N, int D, int H, int W, void* stream) {
    CTU_DISPATCH_LP(dtype, return maxpool2_fwd_impl<T>((const T*)in, in_cs, cp, in_scale, in_shift, in_relu, (T*)out, out_cs, N, D,
                                                       H, W, stream));
}

extern "C" int ctu_maxpool2_bwd(const float* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                int in_relu, const float* gout, int gout_cs, float* gin, int gin_cs, int accumulate,
                                int N, int D, int H, int W, void* stream) {
    return maxpool2_bwd_impl<float>(in, in_cs, cp, in_scale, in_shift, in_relu, gout, gout_cs, gin, gin_cs, accumulate, N, D, H, W,
                                    stream);
}
extern "C" int ctu_lp_maxpool2_bwd(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                   int in_relu, const void* gout, int gout_cs, void* gin, int gin_cs, int accumulate,
                                   int N, int D, int H, int W, void* stream) {
    CTU_DISPATCH_LP(dtype, return maxpool2_bwd_impl<T>((const T*)in, in_cs, cp, in_scale, in_shift, in_relu, (const T*)gout, gout_cs,
                                                       (T*)gin, gin_cs, accumulate, N, D, H, W, stream));
}

extern "C" int ctu_maxpool2_bwd_bn_num_blocks(int N, int D, int H, int W, int cp) {
    // 0 = not available for this channel count (the in-block reduction needs threadIdx % (cp/4) to be the channel quad)
    if (cp <= 0 || cp % 8 != 0 || cp > EW_BLOCK || EW_BLOCK % (cp >> 2) != 0) return 0;
    return (int)ceil_div64((int64_t)N * (D / 2) * (H / 2) * (W / 2) * (cp >> 2), EW_BLOCK);
}

extern "C" int ctu_maxpool2_bwd_bn(const float* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                   const float* mean, const float* invstd, const float* gout, int gout_cs, float* gin,
                                   int gin_cs, int accumulate, int N, int D, int H, int W, float* partials, const ctu_bn_bwd_tail* tail, void* stream) {
    return maxpool2_bwd_bn_impl<float>(in, in_cs, cp, in_scale, in_shift, mean, invstd, gout, gout_cs, gin, gin_cs, accumulate, N, D,
                                       H, W, partials, tail, stream);
}
extern "C" int ctu_lp_maxpool2_bwd_bn(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                                      const float* mean, const float* invstd, const void* gout, int gout_cs, void* gin,
                                      int gin_cs, int accumulate, int N, int D, int H, int W, float* partials, const ctu_bn_bwd_tail* tail, void* stream) {
    CTU_DISPATCH_LP(dtype, return maxpool2_bwd_bn_impl<T>((const T*)in, in_cs, cp, in_scale, in_shift, mean, invstd, (const T*)gout,
                                                          gout_cs, (T*)gin, gin_cs, accumulate, N, D, H, W, partials, tail, stream));
}

extern "C" int ctu_skip_add(const float* a, int a_cs, const float* a_scale, const float* a_shift, int a_relu,
                            const float* b, int b_cs, const float* b_scale, const float* b_shift, int b_relu,
                            float* out, int out_cs, int cp, int64_t nvox, void* stream) {
    return skip_add_impl<float>(a, a_cs, a_scale, a_shift, a_relu, b, b_cs, b_scale, b_shift, b_relu, out, out_cs, cp, nvox, stream);
}
extern "C" int ctu_lp_skip_add(int dtype, const void* a, int a_cs, const float* a_scale, const float* a_shift, int a_relu,
                               const void* b, int b_cs, const float* b_scale, const float* b_shift, int b_relu,
                               void* out, int out_cs, int cp, int64_t nvox, void* stream) {
    CTU_DISPATCH_LP(dtype, return skip_add_impl<T>((const T*)a, a_cs, a_scale, a_shift, a_relu, (const T*)b, b_cs, b_scale, b_shift,
                                                   b_relu, (T*)out, out_cs, cp, nvox, stream));
}

extern "C" int ctu_channel_sum_num_blocks(int64_t nvox) {
    int64_t nb = ceil_div64(nvox, 256);
    if (nb > MAX_RED_BLOCKS) nb = MAX_RED_BLOCKS;
    if (nb < 1) nb = 1;
    return (int)nb;
}

extern "C" int ctu_channel_sum(const float* x, int cs, int cp, int64_t nvox, float* partials, float* out, int C,
                               void* stream) {
    return channel_sum_impl<float>(x, cs, cp, nvox, partials, out, C, stream);
}
extern "C" int ctu_lp_channel_sum(int dtype, const void* x, int cs, int cp, int64_t nvox, float* partials, float* out, int C,
                                  void* stream) {
    CTU_DISPATCH_LP(dtype, return channel_sum_impl<T>((const T*)x, cs, cp, nvox, partials, out, C, stream));
}
