// First encoder convolution (C_in = 1 or 2, k = 3, C_out <= 8) for gfx950.
//
// nn.Conv3d(input_channels, i_size, 3, 1, 1, bias=False) at ctunet/pytorch/models.py:26 with
// input_channels in {1, 2} (models.py:175, 272-296).  K = 27 * C_in is far too short for an implicit-GEMM tile
// (the generic kernel pads C_in to 8: 8x the MFMAs, plus a padded channels-last copy of the input), and the layer is
// HBM-bound (12-21 FLOP/B), so:
//   forward ......... direct VALU convolution, reads the caller's NCDHW planes in place, writes channels-last + BN partials
//   input gradient .. direct VALU convolution of the 8-channel gradient with the flipped weights, writes NCDHW planes
//   weight gradient . MFMA with M = (tap, c_in) (27*C_in rows, padded to 32/64), N = c_out, K = voxels
// All three are persistent over 4x4x32 / 4x4x16 voxel boxes with the box staged in LDS.
#include <type_traits>
#include "common.h"
#include "bn_tail.h"
#include "wgrad_reduce.h"

namespace {

struct FirstP {
    const float* x;        // NCDHW input planes [N][CIN][D][H][W]
    const float* w;        // torch weight [Co][CIN][27]
    const float* bias;
    const void* g;         // channels-last gradient / output side tensor (8 padded channels), element type T
    void* out;             // fwd: channels-last output (T); bwd-data: NCDHW dx (float)
    float* stats;
    float* ws;
    int g_cs, out_cs, Co, nbias;
    int N, D, H, W;
    int tiles_d, tiles_h, tiles_w, ntiles;
    // lazy BatchNorm + ReLU backward in first_wgrad_kernel<.., LZ = true> (as conv3d_wgrad_k3s_kernel's, conv3d.hip): g is the
    // gradient w.r.t. the ACTIVATED output, lz_y the raw output (geometry and stride of g), lz_coef bn_bwd_finalize's
    // [5][8] rows; the raw-output gradient goes to lz_out (geometry of g) for first_bwd_data_kernel
    const float* lz_y;
    float* lz_out;
    const float* lz_scale;
    const float* lz_shift;
    const float* lz_coef;
};

constexpr int TD = 4, TH = 4;

__device__ __forceinline__ void box_origin(const FirstP& p, int t, int TW, int& n, int& d0, int& h0, int& w0) {
    const int tx = t % p.tiles_w; t /= p.tiles_w;
    const int ty = t % p.tiles_h; t /= p.tiles_h;
    const int tz = t % p.tiles_d; t /= p.tiles_d;
    n = t; d0 = tz * TD; h0 = ty * TH; w0 = tx * TW;
}

// ------------------------------------------------------------------ forward: MFMA, weights in registers
// rows = (w-shift s, c_out) [16], columns = 16 voxel pairs (w = 2m, 2m+1), K = (kd, kh, kw' in 0..3, ci):
//   out[(d,h,2m+s), co] = sum x[(d+kd, h+kh, 2m+kw') - 1][ci] * W[co][ci][kd,kh,kw'-s]   (0 <= kw'-s <= 2)
// K = 36*CIN -> 9*CIN MFMAs per 32 voxels.  The per-lane weight fragments (9*CIN floats) and LDS offsets are
// computed once per block; each MFMA needs a single ds_read_b32.  Box 4x4x32, persistent, register prefetch.
template <int CIN, class T>
__global__ __launch_bounds__(256) void first_fwd_kernel(FirstP p, int tiles_per_block, ctu_bn_tail tail) {
    constexpr int TW = 32, HD = TD + 2, HH = TH + 2, HW = TW + 2, HV = HD * HH * HW;
    constexpr int NIT = (HV * CIN + 255) / 256;
    constexpr int NS = 9 * CIN;                                     // K-steps of 4
    __shared__ float sX[HV * CIN];                                  // [ci][halo voxel]
    __shared__ float sRed[4 * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;
    // weight fragment of this lane as the ROW operand: row = m = (s, co), k = 4*st + kq = (tap', ci)
    float wreg[NS];
    int aoff[NS];
    {
        const int s_ = m >> 3, co = m & 7;
#pragma unroll
        for (int st = 0; st < NS; ++st) {
            const int k = 4 * st + kq, tapp = k / CIN, ci = k % CIN;       // tap' = (kd*3+kh)*4 + kw'
            const int kwp = tapp & 3, r = tapp >> 2, kw = kwp - s_;
            wreg[st] = (co < p.Co && kw >= 0 && kw <= 2) ? p.w[((size_t)co * CIN + ci) * 27 + r * 3 + kw] : 0.f;
            aoff[st] = ci * HV + ((r / 3) * HH + r % 3) * HW + kwp;
        }
    }
    int abase[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) abase[mt] = (wave * HH + mt) * HW + 2 * m;       // td = wave, th = mt, pair m
    const int64_t plane = (int64_t)p.D * p.H * p.W;
    const int cq = (kq & 1) * 4, sh = kq >> 1;                       // this lane's 4 channels / shift in the epilogue
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) {
        bv.x = cq + 0 < p.nbias ? p.bias[cq + 0] : 0.f; bv.y = cq + 1 < p.nbias ? p.bias[cq + 1] : 0.f;
        bv.z = cq + 2 < p.nbias ? p.bias[cq + 2] : 0.f; bv.w = cq + 3 < p.nbias ? p.bias[cq + 3] : 0.f;
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    int tile = blockIdx.x * tiles_per_block;
    const int tile_end = min(p.ntiles, tile + tiles_per_block);
    float vx[NIT];
    auto load = [&](int t) {
        int n, d0, h0, w0;
        box_origin(p, t, TW, n, d0, h0, w0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256;
            const int ci = e / HV, v = e % HV;
            const int pw = v % HW, t2 = v / HW, ph = t2 % HH, pd = t2 / HH;
            const int gd = d0 + pd - 1, gh = h0 + ph - 1, gw = w0 + pw - 1;
            float val = 0.f;
            if (e < HV * CIN && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W)
                val = p.x[((int64_t)n * CIN + ci) * plane + ((int64_t)gd * p.H + gh) * p.W + gw];
            vx[it] = val;
        }
    };
    if (tile < tile_end) load(tile);
    while (tile < tile_end) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256;
            if (e < HV * CIN) sX[e] = vx[it];
        }
        __syncthreads();
        if (tile + 1 < tile_end) load(tile + 1);
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NS; ++st) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wreg[st], sX[abase[mt] + aoff[st]], acc[mt], 0, 0, 0);
        }
        int n, d0, h0, w0;
        box_origin(p, tile, TW, n, d0, h0, w0);
        const int gd = d0 + wave, gw = w0 + 2 * m + sh;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int gh = h0 + mt;
            if (gd < p.D && gh < p.H && gw < p.W) {
                const float4 o = rnd4<T>(make_float4(acc[mt][0] + bv.x, acc[mt][1] + bv.y, acc[mt][2] + bv.z, acc[mt][3] + bv.w));
                st4<T>(reinterpret_cast<T*>(p.out) + ((((size_t)n * p.D + gd) * p.H + gh) * p.W + gw) * p.out_cs + cq, o);
                s1[0] += o.x; s1[1] += o.y; s1[2] += o.z; s1[3] += o.w;
                s2[0] += o.x * o.x; s2[1] += o.y * o.y; s2[2] += o.z * o.z; s2[3] += o.w * o.w;
            }
        }
        ++tile;
    }
    if (p.stats) {                                   // one BN partial row [2][8] per block
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a1 = s1[r], a2 = s2[r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); }
            a1 += __shfl_xor(a1, 32); a2 += __shfl_xor(a2, 32);          // the two shifts hold the same channels
            if (m == 0 && kq < 2) { sRed[wave * 16 + cq + r] = a1; sRed[wave * 16 + 8 + cq + r] = a2; }
        }
        __syncthreads();
        if (tid < 16) st_row(tail.counter != nullptr, p.stats + (size_t)blockIdx.x * 16 + tid, (sRed[tid] + sRed[16 + tid]) + (sRed[32 + tid] + sRed[48 + tid]));
        if (tail.counter) bn_fwd_tail(tail, p.stats, gridDim.x, 8, gridDim.x);
    }
}

// ------------------------------------------------------------------ input gradient: dx[v][ci] = sum g[v - tap + 1][co] W[co][ci][tap]
template <int CIN, class T>
__global__ __launch_bounds__(256) void first_bwd_data_kernel(FirstP p, int tiles_per_block) {
    constexpr int TW = 32, HD = TD + 2, HH = TH + 2, HW = TW + 2, HV = HD * HH * HW;
    constexpr int NIT = (HV * 2 + 255) / 256;
    // Haloed gradient box, 8 channels (32 bytes) per voxel with no padding inside a voxel: voxel pw of a w row sits in slot
    // pw + pw / 4 of RS = 44, so the w quads of a row start 5 slots apart and the d planes 6 * 44 = 0 (mod 8) slots apart.
    // The 16 lanes one ds_read_b128 cycle serves (quads {0, 1, 6, 7} of one d plane and {2, 3, 4, 5} of the next, both
    // channel halves) then fall into 8 different slots mod 8 = all 64 banks.  50.7 KB: three blocks per CU, as the grid assumes.
    constexpr int RS = 44, GS = 8;
    __shared__ __attribute__((aligned(16))) float sG[HD * HH * RS * GS];
    __shared__ __attribute__((aligned(16))) float sW[27 * CIN * 8];     // [(kd, kh) row][channel half][ci][kw][4 co], taps flipped
    const int tid = threadIdx.x;
    for (int i = tid; i < 27 * CIN * 8; i += 256) {
        const int c4 = i & 3, kw = (i >> 2) % 3, r = (i >> 2) / 3, ci = r % CIN, hf = (r / CIN) & 1, r9 = (r / CIN) >> 1;
        const int co = hf * 4 + c4;
        sW[i] = co < p.Co ? p.w[((size_t)co * CIN + ci) * 27 + (26 - (r9 * 3 + kw))] : 0.f;
    }
    // A lane pair owns four consecutive w outputs of one (d, h) row: the even lane sums gradient channels 0-3, the odd lane
    // channels 4-7, and the two halves of each output's pairwise tree meet in one cross-lane add.  Per (kd, kh) row a lane reads
    // the six voxels its four outputs need once (its 16-byte half of each) and its 3 * CIN weight quads.
    const int half = tid & 1, wq = (tid >> 1) & 7, td = (tid >> 4) & 3, th = tid >> 6;
    const int pbase = ((td * HH + th) * RS + 5 * wq) * GS + half * 4;
    // a pair of outputs goes out as one 8-byte store where every row of dx starts 8-byte aligned
    const bool st2 = (p.W & 1) == 0 && ((uintptr_t)p.out & 7) == 0;
    const int64_t plane = (int64_t)p.D * p.H * p.W;
    int tile = blockIdx.x * tiles_per_block;
    const int tile_end = min(p.ntiles, tile + tiles_per_block);
    float4 vg[NIT];
    auto load = [&](int t) {
        int n, d0, h0, w0;
        box_origin(p, t, TW, n, d0, h0, w0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256, v = e >> 1;
            const int pw = v % HW, t2 = v / HW, ph = t2 % HH, pd = t2 / HH;
            const int gd = d0 + pd - 1, gh = h0 + ph - 1, gw = w0 + pw - 1;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < HV * 2 && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W)
                val = ld4<T>(reinterpret_cast<const T*>(p.g) + ((((size_t)n * p.D + gd) * p.H + gh) * p.W + gw) * p.g_cs + half * 4);
            vg[it] = val;
        }
    };
    if (tile < tile_end) load(tile);
    while (tile < tile_end) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256;
            const int v = e >> 1, pw = v % HW;
            if (e < HV * 2) *reinterpret_cast<float4*>(&sG[((v / HW) * RS + pw + (pw >> 2)) * GS + half * 4]) = vg[it];
        }
        __syncthreads();
        if (tile + 1 < tile_end) load(tile + 1);
        // 8 independent partial sums (one per gradient channel) per output and voxel: no long dependent FMA chain
        float q[4][CIN][4];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                for (int c = 0; c < 4; ++c) q[o][ci][c] = 0.f;
        // the (kd, kh) rows stay rolled: unrolled by 3 the kernel needs 212 registers instead of 144 and a third block no
        // longer fits a CU (measured slower), fully unrolled it spills
#pragma unroll 1
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
            const float* gp = &sG[pbase + ((kd * HH + kh) * RS) * GS];
            const float* wr = &sW[(((kd * 3 + kh) * 2 + half) * CIN) * 12];
            float4 gv[6], wv[CIN][3];
#pragma unroll
            for (int j = 0; j < 6; ++j) gv[j] = *reinterpret_cast<const float4*>(gp + (j + (j >> 2)) * GS);
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) wv[ci][kw] = *reinterpret_cast<const float4*>(wr + (ci * 3 + kw) * 4);
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)                   // every partial sum takes its taps in (kd, kh, kw) order
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        q[o][ci][0] = fmaf(gv[o + kw].x, wv[ci][kw].x, q[o][ci][0]);
                        q[o][ci][1] = fmaf(gv[o + kw].y, wv[ci][kw].y, q[o][ci][1]);
                        q[o][ci][2] = fmaf(gv[o + kw].z, wv[ci][kw].z, q[o][ci][2]);
                        q[o][ci][3] = fmaf(gv[o + kw].w, wv[ci][kw].w, q[o][ci][3]);
                    }
        }
        // ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)): each lane forms its half, the pair's other lane supplies the rest
        // the even lane finishes and stores outputs 0 and 1, the odd lane outputs 2 and 3
        float o0[CIN], o1[CIN];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            const float m0 = (q[0][ci][0] + q[0][ci][1]) + (q[0][ci][2] + q[0][ci][3]);
            const float m1 = (q[1][ci][0] + q[1][ci][1]) + (q[1][ci][2] + q[1][ci][3]);
            const float m2 = (q[2][ci][0] + q[2][ci][1]) + (q[2][ci][2] + q[2][ci][3]);
            const float m3 = (q[3][ci][0] + q[3][ci][1]) + (q[3][ci][2] + q[3][ci][3]);
            const float r0 = __shfl_xor(half ? m0 : m2, 1), r1 = __shfl_xor(half ? m1 : m3, 1);
            const float k0 = half ? m2 : m0, k1 = half ? m3 : m1;
            o0[ci] = half ? r0 + k0 : k0 + r0;                // channels 0-3 first, as in the tree
            o1[ci] = half ? r1 + k1 : k1 + r1;
        }
        int n, d0, h0, w0;
        box_origin(p, tile, TW, n, d0, h0, w0);
        const int gd = d0 + td, gh = h0 + th, gw = w0 + 4 * wq + 2 * half;
        if (gd < p.D && gh < p.H) {
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                float* dst = reinterpret_cast<float*>(p.out) + ((int64_t)n * CIN + ci) * plane + ((int64_t)gd * p.H + gh) * p.W + gw;
                if (st2) {
                    if (gw < p.W) *reinterpret_cast<float2*>(dst) = make_float2(o0[ci], o1[ci]);
                } else {
                    if (gw < p.W) dst[0] = o0[ci];
                    if (gw + 1 < p.W) dst[1] = o1[ci];
                }
            }
        }
        ++tile;
    }
}

// ------------------------------------------------------------------ weight gradient: M = (tap, ci), N = co, K = voxels
template <int CIN, class T, bool LZ = false>
__global__ __launch_bounds__(256) void first_wgrad_kernel(FirstP p, int tiles_per_block) {
    constexpr int TW = 32, HD = TD + 2, HH = TH + 2, HW = TW + 2, HV = HD * HH * HW, NV = TD * TH * TW;
    constexpr int MTN = (27 * CIN + 15) / 16;                  // M tiles
    constexpr int NIT = (HV * CIN + 255) / 256;
    constexpr int GIT = NV * 2 / 256;
    __shared__ float sX[HV * CIN];                             // [ci][halo voxel]
    __shared__ __attribute__((aligned(16))) float sG[NV * 8];
    __shared__ float sRed[4 * MTN * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int64_t plane = (int64_t)p.D * p.H * p.W;
    int rowoff[MTN];
    bool rowok[MTN];
#pragma unroll
    for (int mt = 0; mt < MTN; ++mt) {
        const int r = mt * 16 + i, tap = r / CIN, ci = r % CIN;
        rowok[mt] = r < 27 * CIN;
        const int tp = rowok[mt] ? tap : 0;
        rowoff[mt] = ci * HV + ((tp / 9) * HH + (tp / 3) % 3) * HW + tp % 3;
    }
    f32x4 acc[MTN];
#pragma unroll
    for (int mt = 0; mt < MTN; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int tile = blockIdx.x * tiles_per_block;
    const int tile_end = min(p.ntiles, tile + tiles_per_block);
    const int half = tid & 1;
    float vx[NIT];
    float4 vg[GIT];
    float4 vy[LZ ? GIT : 1];
    float4 l_sc = make_float4(0.f, 0.f, 0.f, 0.f), l_sh = l_sc, l_k0 = l_sc, l_A = l_sc, l_B = l_sc;
    if constexpr (LZ) {
        l_sc = *reinterpret_cast<const float4*>(p.lz_scale + half * 4);
        l_sh = *reinterpret_cast<const float4*>(p.lz_shift + half * 4);
        l_k0 = *reinterpret_cast<const float4*>(p.lz_coef + half * 4);
        l_A = *reinterpret_cast<const float4*>(p.lz_coef + 24 + half * 4);
        l_B = *reinterpret_cast<const float4*>(p.lz_coef + 32 + half * 4);
    }
    auto load = [&](int t) {
        int n, d0, h0, w0;
        box_origin(p, t, TW, n, d0, h0, w0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256;
            const int ci = e / HV, v = e % HV;
            const int pw = v % HW, t2 = v / HW, ph = t2 % HH, pd = t2 / HH;
            const int gd = d0 + pd - 1, gh = h0 + ph - 1, gw = w0 + pw - 1;
            float val = 0.f;
            if (e < HV * CIN && (unsigned)gd < (unsigned)p.D && (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W)
                val = p.x[((int64_t)n * CIN + ci) * plane + ((int64_t)gd * p.H + gh) * p.W + gw];
            vx[it] = val;
        }
#pragma unroll
        for (int it = 0; it < GIT; ++it) {
            const int e = tid + it * 256, v = e >> 1;
            const int tw_ = v % TW, th_ = (v / TW) % TH, td_ = v / (TW * TH);
            const int gd = d0 + td_, gh = h0 + th_, gw = w0 + tw_;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gd < p.D && gh < p.H && gw < p.W) {
                const size_t idx = ((((size_t)n * p.D + gd) * p.H + gh) * p.W + gw) * p.g_cs + half * 4;
                val = ld4<T>(reinterpret_cast<const T*>(p.g) + idx);
                if constexpr (LZ) vy[it] = *reinterpret_cast<const float4*>(p.lz_y + idx);
            }
            vg[it] = val;
        }
    };
    if (tile < tile_end) load(tile);
    while (tile < tile_end) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int e = tid + it * 256;
            if (e < HV * CIN) sX[e] = vx[it];
        }
        if constexpr (LZ) {
            // the registers hold box `tile`: form its raw-output gradient (out-of-volume items stay 0) and write it out
            int n, d0, h0, w0;
            box_origin(p, tile, TW, n, d0, h0, w0);
#pragma unroll
            for (int it = 0; it < GIT; ++it) {
                const int e = tid + it * 256, v = e >> 1;
                const int tw_ = v % TW, th_ = (v / TW) % TH, td_ = v / (TW * TH);
                const int gd = d0 + td_, gh = h0 + th_, gw = w0 + tw_;
                if (gd < p.D && gh < p.H && gw < p.W) {
                    vg[it] = bn_bwd_lazy4(vg[it], vy[it], l_sc, l_sh, l_k0, l_A, l_B);
                    *reinterpret_cast<float4*>(p.lz_out + ((((size_t)n * p.D + gd) * p.H + gh) * p.W + gw) * p.g_cs + half * 4) = vg[it];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < GIT; ++it) {
            const int e = tid + it * 256;
            *reinterpret_cast<float4*>(&sG[(e >> 1) * 8 + half * 4]) = vg[it];
        }
        __syncthreads();
        if (tile + 1 < tile_end) load(tile + 1);
#pragma unroll 4
        for (int ks = 0; ks < NV / 16; ++ks) {
            const int th_ = ks / (TW / 4), tw_ = (ks % (TW / 4)) * 4 + kq;             // td = wave
            const float b = (i < 8) ? sG[((wave * TH + th_) * TW + tw_) * 8 + i] : 0.f;
            const int pb = (wave * HH + th_) * HW + tw_;
#pragma unroll
            for (int mt = 0; mt < MTN; ++mt) {
                const float a = rowok[mt] ? sX[pb + rowoff[mt]] : 0.f;
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[mt], 0, 0, 0);
            }
        }
        ++tile;
    }
    // cross-wave reduction -> one slab [MTN][16 rows][16 co] per block
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MTN; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) sRed[(wave * MTN + mt) * 256 + (kq * 4 + r) * 16 + i] = acc[mt][r];
    __syncthreads();
    float* dst = p.ws + (size_t)blockIdx.x * (MTN * 256);
    for (int e = tid; e < MTN * 256; e += 256)
        dst[e] = (sRed[e] + sRed[MTN * 256 + e]) + (sRed[2 * MTN * 256 + e] + sRed[3 * MTN * 256 + e]);
}

template <int CIN>
__global__ __launch_bounds__(1024) void first_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Co,
                                                                 int gx) {
    __shared__ float red[RPARTS][64];
    first_wgrad_reduce_block<CIN>(ws, dw, Co, gx, blockIdx.x, threadIdx.x, red);
}

// resident blocks per CU of the three kernels (x 256 CUs: the cap of their persistent grids)
constexpr int FWD_PER_CU = 4, DGRAD_PER_CU = 3, WGRAD_PER_CU = 5;

// the 4 x 4 x 32 boxes of a volume and the grid of a kernel over them
Grid fill(FirstP& p, int N, int D, int H, int W, int per_cu) {
    p.N = N; p.D = D; p.H = H; p.W = W;
    p.tiles_d = ceil_div(D, TD); p.tiles_h = ceil_div(H, TH); p.tiles_w = ceil_div(W, 32);
    p.ntiles = N * p.tiles_d * p.tiles_h * p.tiles_w;
    return persist_grid(p.ntiles, 256 * per_cu);
}

}  // namespace

// =================================================================== C ABI
extern "C" int ctu_conv3d_first_supported(int k, int cin, int nout_p, int W) {
    return (k == 3 && (cin == 1 || cin == 2) && nout_p == 8 && W >= 16) ? 1 : 0;
}

extern "C" int ctu_conv3d_first_num_blocks(int N, int D, int H, int W) {
    FirstP p;
    return fill(p, N, D, H, W, FWD_PER_CU).gx;
}

namespace {

template <class T>
int first_fwd_impl(const float* x, int cin, const float* w, const float* bias, int nbias, T* out, int out_cs, int Co, float* stats,
                   int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream) {
    CTU_REQUIRE(!tail || (stats && tail->counter && tail->gamma && tail->beta && tail->scale && tail->shift && tail->mean &&
                          tail->invstd && tail->C > 0 && tail->C <= 8 && tail->count > 0),
                "conv3d_first_fwd: incomplete BatchNorm tail");
    CTU_REQUIRE(x && w && out, "conv3d_first_fwd: null pointer");
    CTU_REQUIRE((cin == 1 || cin == 2) && Co >= 1 && Co <= 8, "conv3d_first_fwd: cin=%d Co=%d unsupported", cin, Co);
    CTU_REQUIRE(out_cs >= 8 && out_cs % 4 == 0 && ((uintptr_t)out & (4 * sizeof(T) - 1)) == 0, "conv3d_first_fwd: output slice alignment");
    FirstP p{};
    p.x = x; p.w = w; p.bias = bias; p.nbias = bias ? nbias : 0; p.out = out; p.out_cs = out_cs; p.Co = Co; p.stats = stats;
    const auto [gx, tpb] = fill(p, N, D, H, W, FWD_PER_CU);
    if (cin == 1) first_fwd_kernel<1, T><<<gx, 256, 0, (hipStream_t)stream>>>(p, tpb, tail_or_off(tail));
    else first_fwd_kernel<2, T><<<gx, 256, 0, (hipStream_t)stream>>>(p, tpb, tail_or_off(tail));
    CTU_CHECK_LAUNCH("conv3d_first_fwd");
    return CTU_OK;
}

template <class T>
int first_bwd_data_impl(const T* g, int g_cs, const float* w, int cin, int Co, float* dx, int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(g && w && dx, "conv3d_first_bwd_data: null pointer");
    CTU_REQUIRE((cin == 1 || cin == 2) && Co >= 1 && Co <= 8 && g_cs >= 8 && g_cs % 4 == 0 && ((uintptr_t)g & (4 * sizeof(T) - 1)) == 0,
                "conv3d_first_bwd_data: bad argument");
    FirstP p{};
    p.g = g; p.g_cs = g_cs; p.w = w; p.out = dx; p.Co = Co;
    const auto [gx, tpb] = fill(p, N, D, H, W, DGRAD_PER_CU);
    if (cin == 1) first_bwd_data_kernel<1, T><<<gx, 256, 0, (hipStream_t)stream>>>(p, tpb);
    else first_bwd_data_kernel<2, T><<<gx, 256, 0, (hipStream_t)stream>>>(p, tpb);
    CTU_CHECK_LAUNCH("conv3d_first_bwd_data");
    return CTU_OK;
}

struct FirstLazy { const float* y; const float* scale; const float* shift; const float* coef; float* out; };

template <class T>
int first_wgrad_impl(const float* x, int cin, const T* g, int g_cs, float* dw, int Co, float* ws, int N, int D, int H, int W,
                     const FirstLazy* lz, void* stream, ctu_wgrad_job* job = nullptr) {
    CTU_REQUIRE(x && g && dw && ws, "conv3d_first_wgrad: null pointer");
    CTU_REQUIRE((cin == 1 || cin == 2) && Co >= 1 && Co <= 8 && g_cs >= 8 && g_cs % 4 == 0 && ((uintptr_t)g & (4 * sizeof(T) - 1)) == 0,
                "conv3d_first_wgrad: bad argument");
    FirstP p{};
    p.x = x; p.g = g; p.g_cs = g_cs; p.ws = ws; p.Co = Co;
    if (lz) { p.lz_y = lz->y; p.lz_out = lz->out; p.lz_scale = lz->scale; p.lz_shift = lz->shift; p.lz_coef = lz->coef; }
    const auto [gx, tpb] = fill(p, N, D, H, W, WGRAD_PER_CU);
    hipStream_t st = (hipStream_t)stream;
    if (cin == 1) {
        if constexpr (std::is_same<T, float>::value) {
            if (lz) first_wgrad_kernel<1, T, true><<<gx, 256, 0, st>>>(p, tpb);
            else first_wgrad_kernel<1, T><<<gx, 256, 0, st>>>(p, tpb);
        } else first_wgrad_kernel<1, T><<<gx, 256, 0, st>>>(p, tpb);
        if (!job) first_wgrad_reduce_kernel<1><<<ceil_div(2 * 256, 64), 1024, 0, st>>>(ws, dw, Co, gx);
    } else {
        if constexpr (std::is_same<T, float>::value) {
            if (lz) first_wgrad_kernel<2, T, true><<<gx, 256, 0, st>>>(p, tpb);
            else first_wgrad_kernel<2, T><<<gx, 256, 0, st>>>(p, tpb);
        } else first_wgrad_kernel<2, T><<<gx, 256, 0, st>>>(p, tpb);
        if (!job) first_wgrad_reduce_kernel<2><<<ceil_div(4 * 256, 64), 1024, 0, st>>>(ws, dw, Co, gx);
    }
    CTU_CHECK_LAUNCH("conv3d_first_wgrad");
    if (job) {                                     // the caller reduces the slabs later (ctu_bn_bwd_finalize_jobs / ctu_wgrad_reduce_jobs)
        *job = ctu_wgrad_job{};
        job->kind = WGJ_FIRST + (cin - 1);
        job->ws = ws; job->dw = dw; job->Co = Co; job->Ci = cin; job->gx = gx; job->pairs = 1; job->nmf = (27 * cin + 15) / 16;
    }
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_conv3d_first_fwd(const float* x, int cin, const float* w, const float* bias, int nbias, float* out,
                                    int out_cs, int Co, float* stats, int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream) {
    return first_fwd_impl<float>(x, cin, w, bias, nbias, out, out_cs, Co, stats, N, D, H, W, tail, stream);
}
extern "C" int ctu_lp_conv3d_first_fwd(int dtype, const float* x, int cin, const float* w, const float* bias, int nbias, void* out,
                                       int out_cs, int Co, float* stats, int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream) {
    CTU_DISPATCH_LP(dtype, return first_fwd_impl<T>(x, cin, w, bias, nbias, (T*)out, out_cs, Co, stats, N, D, H, W, tail, stream));
}

extern "C" int ctu_conv3d_first_bwd_data(const float* g, int g_cs, const float* w, int cin, int Co, float* dx, int N, int D,
                                         int H, int W, void* stream) {
    return first_bwd_data_impl<float>(g, g_cs, w, cin, Co, dx, N, D, H, W, stream);
}
extern "C" int ctu_lp_conv3d_first_bwd_data(int dtype, const void* g, int g_cs, const float* w, int cin, int Co, float* dx, int N,
                                            int D, int H, int W, void* stream) {
    CTU_DISPATCH_LP(dtype, return first_bwd_data_impl<T>((const T*)g, g_cs, w, cin, Co, dx, N, D, H, W, stream));
}

extern "C" size_t ctu_conv3d_first_wgrad_ws_floats(int N, int D, int H, int W, int cin) {
    FirstP p;
    return (size_t)fill(p, N, D, H, W, WGRAD_PER_CU).gx * ((27 * cin + 15) / 16) * 256;
}

extern "C" int ctu_conv3d_first_wgrad(const float* x, int cin, const float* g, int g_cs, float* dw, int Co, float* ws, int N,
                                      int D, int H, int W, void* stream) {
    return first_wgrad_impl<float>(x, cin, g, g_cs, dw, Co, ws, N, D, H, W, nullptr, stream);
}
extern "C" int ctu_conv3d_first_wgrad_bn(const float* x, int cin, const float* ga, int g_cs, const float* y, const float* bn_scale,
                                         const float* bn_shift, const float* coef, float* gy_out, float* dw, int Co, float* ws,
                                         int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(y && bn_scale && bn_shift && coef && gy_out && gy_out != ga, "conv3d_first_wgrad_bn: null pointer / gy_out aliases ga");
    CTU_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)gy_out & 15) == 0, "conv3d_first_wgrad_bn: 16-byte alignment");
    const FirstLazy lz = {y, bn_scale, bn_shift, coef, gy_out};
    return first_wgrad_impl<float>(x, cin, ga, g_cs, dw, Co, ws, N, D, H, W, &lz, stream);
}
extern "C" int ctu_conv3d_first_wgrad_slabs(const float* x, int cin, const float* g, int g_cs, float* dw, int Co, float* ws, int N,
                                            int D, int H, int W, ctu_wgrad_job* job, void* stream) {
    CTU_REQUIRE(job, "conv3d_first_wgrad_slabs: null job");
    return first_wgrad_impl<float>(x, cin, g, g_cs, dw, Co, ws, N, D, H, W, nullptr, stream, job);
}
extern "C" int ctu_conv3d_first_wgrad_bn_slabs(const float* x, int cin, const float* ga, int g_cs, const float* y,
                                               const float* bn_scale, const float* bn_shift, const float* coef, float* gy_out,
                                               float* dw, int Co, float* ws, int N, int D, int H, int W, ctu_wgrad_job* job,
                                               void* stream) {
    CTU_REQUIRE(job, "conv3d_first_wgrad_bn_slabs: null job");
    CTU_REQUIRE(y && bn_scale && bn_shift && coef && gy_out && gy_out != ga, "conv3d_first_wgrad_bn: null pointer / gy_out aliases ga");
    CTU_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)gy_out & 15) == 0, "conv3d_first_wgrad_bn: 16-byte alignment");
    const FirstLazy lz = {y, bn_scale, bn_shift, coef, gy_out};
    return first_wgrad_impl<float>(x, cin, ga, g_cs, dw, Co, ws, N, D, H, W, &lz, stream, job);
}
extern "C" int ctu_lp_conv3d_first_wgrad(int dtype, const float* x, int cin, const void* g, int g_cs, float* dw, int Co, float* ws,
                                         int N, int D, int H, int W, void* stream) {
    CTU_DISPATCH_LP(dtype, return first_wgrad_impl<T>(x, cin, (const T*)g, g_cs, dw, Co, ws, N, D, H, W, nullptr, stream));
}
