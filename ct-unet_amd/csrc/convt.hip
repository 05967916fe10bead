// ConvTranspose3d(kernel 2, stride 2, bias) for gfx950 -- replaces nn.ConvTranspose3d at
// ctunet/pytorch/models.py:37 and :427-429 and its autograd backward.
//
// With kernel == stride every output voxel receives exactly one tap, so the op is a plain GEMM
//   [input voxels x Ci] . [Ci x (8 taps x Co)]  followed by a scatter to (2d+i, 2h+j, 2w+l).
// A block owns 64 consecutive input voxels (4 waves x one 16-voxel M-tile), keeps their
// activated channels in LDS (row stride Ci+4 floats -> conflict-free ds_read_b64) and walks the
// 8 taps, staging one tap's packed weights at a time.  v_mfma_f32_16x16x4_f32, exact fp32.
// The op is HBM-bound (the 8x larger output stream), see DESIGN.md.
#include "common.h"
#include "pack.h"
#include "wgrad_reduce.h"

namespace {

struct CtP {
    const float* in;         // fwd: input [V][in_cs]; bwd-data: gout on the 2x grid
    const float* in_scale;
    const float* in_shift;
    const float* wp;
    const float* bias;
    float* out;              // fwd: output on the 2x grid; bwd-data: gin [V][out_cs]
    int in_cs, rin_p, in_relu, out_cs, nout_p, nbias;
    int ntt_total;           // 16-wide output tiles in the packed weights (power of two)
    int N, D, H, W;          // coarse (input-side) grid
    int64_t nvox;            // N*D*H*W
};

// Fine-grid voxel index of tap 0 for coarse voxel v (32-bit division: emulated 64-bit div/mod by runtime sizes is
// ~10x more expensive and used to dominate these HBM-bound kernels), and the per-tap offset on the fine grid.
__device__ __forceinline__ size_t fine_base(int64_t v, int D, int H, int W) {
    const unsigned u = (unsigned)v;
    const unsigned w = u % (unsigned)W, t1 = u / (unsigned)W;
    const unsigned h = t1 % (unsigned)H, t2 = t1 / (unsigned)H;
    const unsigned d = t2 % (unsigned)D, n = t2 / (unsigned)D;
    return (((size_t)n * (2 * D) + 2 * d) * (2 * H) + 2 * h) * (size_t)(2 * W) + 2 * w;
}
__device__ __forceinline__ int tap_off(int tap, int H, int W) {
    return ((tap >> 2) * (2 * H) + ((tap >> 1) & 1)) * (2 * W) + (tap & 1);
}

// MODE 0: forward (A staged once, one store per tap).  MODE 1: data gradient (A gathered per tap
// from the fine grid, accumulated over the 8 taps, one store).
// The MFMA operands are swapped (weights as the row operand, voxels as the column operand) so that a
// lane ends up with 4 CONSECUTIVE output channels of one voxel: the epilogue is one 16-byte store per
// lane instead of four scattered dword stores.  `tps` taps' weights make one stage.
template <int NTT, int MODE>
__global__ __launch_bounds__(256) void convt2_kernel(CtP p, int tps) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int AS = p.rin_p + 4;                       // LDS row stride (floats)
    float* sA = smem;                                 // [64][AS]
    float* sW = smem + 64 * AS;                       // [tps][rin_p/8][NTT][128]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    const int ng = p.rin_p >> 3;
    const int nq = p.rin_p >> 2;                      // float4 per voxel
    const bool has_xf = p.in_scale != nullptr;
    const int wfl = ng * NTT * 128;                   // this block's share of one tap: NTT of the ntt_total tiles
    const int by = blockIdx.y;
    const int64_t vme = v0 + wave * 16 + m;           // this lane's voxel (column of the MFMA tile)
    const size_t fme = vme < p.nvox ? fine_base(vme, p.D, p.H, p.W) : 0;
    // MODE 1 staging: this thread's gather items (voxel of item k = (tid + 256 k) / nq) and their fine-grid bases
    constexpr int GMAX = 8;                           // 64 * nq / 256 <= 8 for rin_p <= 128 (ct_channels_ok refuses more)
    size_t gbase[GMAX];
    if (MODE == 1) {
#pragma unroll
        for (int k = 0; k < GMAX; ++k) {
            const int it = tid + k * 256;
            const int64_t v = v0 + it / nq;
            gbase[k] = (it < 64 * nq && v < p.nvox) ? fine_base(v, p.D, p.H, p.W) : (size_t)-1;
        }
    }

    f32x4 acc[NTT];
#pragma unroll
    for (int nt = 0; nt < NTT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Staging is all latency here (deep levels: a few hundred blocks, one per CU), so nothing is fetched when it is needed:
    // every batch of loads is issued together, branch-free (items past the end re-read a valid address and are not stored),
    // into registers, one stage ahead of its use, and goes to LDS between two barriers after the MFMAs that read the stage
    // it replaces (the planned LDS holds one weight stage and one A image, so the second stage lives in registers).
    const int tot = tps * wfl;                        // floats of one weight stage
    f32x4 wv[8], vg[GMAX];
    // packed weights: [tap][g][ntt_total][128]; this block takes tiles by*NTT .. by*NTT+NTT-1.  Chunk c of a stage is the
    // floats [c * 8192, c * 8192 + 8192): chunk 0 is the one that is fetched ahead, a 128-channel x 128-channel stage has two.
    auto w_issue = [&](int tap0, int c) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i1 = tid * 4 + (c * 8 + k) * 1024;
            const int i = i1 < tot ? i1 : 0;
            const int tl = i / wfl, rem = i % wfl, g = rem / (NTT * 128), r = rem % (NTT * 128);
            // (a 32-bit offset: the packed weights are at most 512 KB, and 64-bit address arithmetic costs 8 registers)
            wv[k] =*reinterpret_cast<const f32x4*>(p.wp + (unsigned)((((tap0 + tl) * ng + g) * p.ntt_total + by * NTT) * 128 + r));
        }
    };
    auto w_store = [&](int c) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i1 = tid * 4 + (c * 8 + k) * 1024;
            if (i1 < tot) *reinterpret_cast<f32x4*>(&sW[i1]) = wv[k];
        }
    };
    auto w_rest = [&](int tap0) {                     // what chunk 0 does not hold, fetched where it is stored
        for (int c = 1; c * 8192 < tot; ++c) { w_issue(tap0, c); w_store(c); }
    };
    // MODE 0: the block's 64 input voxels; MODE 1: one tap's fine-grid voxels of the block's 64 coarse voxels
    auto a_issue = [&](int tap) {
        const int toff = MODE == 1 ? tap_off(tap, p.H, p.W) : 0;
#pragma unroll
        for (int k = 0; k < GMAX; ++k) {
            const int it = tid + k * 256;
            const int vl = it / nq, qd = it % nq;
            if (MODE == 0) {
                const bool ok = it < 64 * nq && v0 + vl < p.nvox;
                vg[k] = *reinterpret_cast<const f32x4*>(p.in + (ok ? (size_t)(v0 + vl) * p.in_cs : (size_t)0) + qd * 4);
            } else {
                const bool ok = gbase[k] != (size_t)-1;
                vg[k] = *reinterpret_cast<const f32x4*>(p.in + (ok ? (gbase[k] + toff) * p.in_cs : (size_t)0) + qd * 4);
            }
        }
    };
    auto a_store = [&]() {
#pragma unroll
        for (int k = 0; k < GMAX; ++k) {
            const int it = tid + k * 256;
            const int vl = it / nq, qd = it % nq;
            if (it < 64 * nq) {
                if (MODE == 0) {
                    float4 val = make_float4(vg[k][0], vg[k][1], vg[k][2], vg[k][3]);
                    if (has_xf)                       // the transform's rows wait in the weight stage's LDS (below)
                        val = xform4(val, *reinterpret_cast<const float4*>(&sW[qd * 4]),
                                     *reinterpret_cast<const float4*>(&sW[(nq + qd) * 4]), p.in_relu);
                    if (v0 + vl >= p.nvox) val = make_float4(0.f, 0.f, 0.f, 0.f);
                    *reinterpret_cast<float4*>(&sA[vl * AS + qd * 4]) = val;
                } else {
                    const bool ok = gbase[k] != (size_t)-1;
                    *reinterpret_cast<f32x4*>(&sA[vl * AS + qd * 4]) = ok ? vg[k] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    };

    // the bias quads of this lane's output channels (the loop below stores between its loads: it would fetch them per tap)
    float4 bv[NTT];
#pragma unroll
    for (int nt = 0; nt < NTT; ++nt) {
        const int co = (by * NTT + nt) * 16 + kq * 4;
        bv[nt].x = (MODE == 0 && p.bias && co + 0 < p.nbias) ? p.bias[co + 0] : 0.f;
        bv[nt].y = (MODE == 0 && p.bias && co + 1 < p.nbias) ? p.bias[co + 1] : 0.f;
        bv[nt].z = (MODE == 0 && p.bias && co + 2 < p.nbias) ? p.bias[co + 2] : 0.f;
        bv[nt].w = (MODE == 0 && p.bias && co + 3 < p.nbias) ? p.bias[co + 3] : 0.f;
    }
    // The input transform's scale and shift rows (2 * rin_p floats) pass through the start of the weight stage's LDS, which is
    // free until the first stage lands: read from global memory where they are used, each item paid a round trip of its own.
    const bool xf_stage = MODE == 0 && has_xf;
    float4 xfv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xf_stage && tid < 2 * nq) xfv = *reinterpret_cast<const float4*>((tid < nq ? p.in_scale : p.in_shift - p.rin_p) + tid * 4);
    a_issue(0);                                       // the A image and the first weight stage travel together
    w_issue(0, 0);
    if (xf_stage) {
        if (tid < 2 * nq) *reinterpret_cast<float4*>(&sW[tid * 4]) = xfv;
        __syncthreads();
    }
    a_store();
    if (xf_stage) __syncthreads();
    w_store(0);
    w_rest(0);
    __syncthreads();
    const float* arow = &sA[(wave * 16 + m) * AS + kq * 2];
    for (int tap = 0; tap < 8; ++tap) {
        const int tl = tap & (tps - 1);               // tps is a power of two
        const bool swap_w = tl == tps - 1 && tap < 7;
        if (tl == 0 && tap + tps < 8) w_issue(tap + tps, 0);     // the next stage's weights fly under this stage's MFMAs
        if (MODE == 1 && tap < 7) a_issue(tap + 1);             // and so does the next tap's gather
        if (MODE == 0) {
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* brow = &sW[tl * wfl + kq * 32 + m * 2];
        // rows = output channels (weights), columns = voxels; K ascending over the 8-channel groups, .x then .y.  One wave per
        // SIMD: nobody else covers an LDS read, so the fragments of the next pair of groups are read before this pair's MFMAs.
        auto frag = [&](int g, float2& fa, float2 (&fb)[NTT]) {
            fa = *reinterpret_cast<const float2*>(arow + g * 8);
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt) fb[nt] = *reinterpret_cast<const float2*>(brow + (g * NTT + nt) * 128);
        };
        auto mma = [&](const float2& fa, const float2 (&fb)[NTT]) {
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt) {
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[nt].x, fa.x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[nt].y, fa.y, acc[nt], 0, 0, 0);
            }
        };
        const int np = ng >> 1;
        float2 a0, a1, b0[NTT], b1[NTT], c0, c1, d0[NTT], d1[NTT];           // two register sets, used in turn
        if (np) { frag(0, a0, b0); frag(1, a1, b1); }
        int pr = 0;
        for (; pr + 2 <= np; pr += 2) {
            frag(2 * pr + 2, c0, d0);
            frag(2 * pr + 3, c1, d1);
            mma(a0, b0);
            mma(a1, b1);
            const int gn = pr + 2 < np ? 2 * pr + 4 : 2 * pr;     // past the last pair: an earlier one again (inside the stage, unused)
            frag(gn, a0, b0);
            frag(gn + 1, a1, b1);
            mma(c0, d0);
            mma(c1, d1);
        }
        if (pr < np) {                                // an odd number of pairs: the last one is in the first set
            mma(a0, b0);
            mma(a1, b1);
        }
        if (ng & 1) {                                 // ng = 1, odd ng: the last group
            frag(ng - 1, a0, b0);
            mma(a0, b0);
        }
        if (MODE == 0 && vme < p.nvox) {
            float* orow = p.out + (fme + tap_off(tap, p.H, p.W)) * p.out_cs;
#pragma unroll
            for (int nt = 0; nt < NTT; ++nt) {
                const int co = (by * NTT + nt) * 16 + kq * 4;   // this lane: channels co .. co+3 of voxel vme
                if (co < p.nout_p) {
                    *reinterpret_cast<float4*>(orow + co) =
                        make_float4(acc[nt][0] + bv[nt].x, acc[nt][1] + bv[nt].y, acc[nt][2] + bv[nt].z, acc[nt][3] + bv[nt].w);
                }
            }
        }
        if (swap_w || (MODE == 1 && tap < 7)) {
            __syncthreads();                          // every wave is done with the stage that is replaced
            if (swap_w) { w_store(0); w_rest(tap + 1); }
            if (MODE == 1) a_store();
            __syncthreads();
        }
    }
    if (MODE == 1 && vme < p.nvox) {
        float* orow = p.out + (size_t)vme * p.out_cs;
#pragma unroll
        for (int nt = 0; nt < NTT; ++nt) {
            const int co = (by * NTT + nt) * 16 + kq * 4;
            if (co < p.nout_p)
                *reinterpret_cast<float4*>(orow + co) = make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
        }
    }
}

inline int pick_ntt(int nout_p) {
    const int n16 = (nout_p + 15) / 16;
    return n16 <= 1 ? 1 : (n16 <= 2 ? 2 : (n16 <= 4 ? 4 : 8));
}

// wp[tap][g][nt][kq][n][j]; one thread per packed element (gather, no memset needed).
// cinv: padded input-channel position -> logical channel (-1 = padding, NULL = identity).
__global__ void pack_convt_w_kernel(const float* __restrict__ w, float* __restrict__ wp, int Ci, int Co,
                                    const int32_t* __restrict__ cinv, int rin_p, int NTT, int mode) {
    pack_convt_w_elem(blockIdx.x * blockDim.x + threadIdx.x, w, wp, Ci, Co, cinv, rin_p, NTT, mode);
}

// ------------------------------------------------------------------ weight gradient
struct CtWgP {
    const float* in;
    const float* in_scale;
    const float* in_shift;
    const float* g;
    float* ws;
    int in_cs, cin_p, in_relu, g_cs, cout_p;
    int N, D, H, W;
    int64_t nvox;
    int ntiles, n_ci_t;
};

// M = MI x 16 input channels, N = NJ x 16 output channels, K = coarse voxels; one accumulator per (tap, tile pair).
// A block with 2 x 2 tiles reads the (8x larger) fine-grid gradient ONCE for 32 x 32 channels.  The bias gradient
// (sum of gout over voxels) is accumulated by the staging threads from the values they load anyway.
template <int MI, int NJ>
__global__ __launch_bounds__(256) void convt2_wgrad_kernel(CtWgP p, float* __restrict__ wsb) {
    constexpr int CA = 16 * MI, CG = 16 * NJ, QA = 4 * MI, QG = 4 * NJ;
    __shared__ __attribute__((aligned(16))) float sA[64 * CA];
    __shared__ __attribute__((aligned(16))) float sG[8 * 64 * CG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int cig = blockIdx.y % p.n_ci_t, cog = blockIdx.y / p.n_ci_t;
    const int ci0 = cig * CA, co0 = cog * CG;
    const int qa = tid % QA, qg = tid % QG;                    // 256 % QA == 0: fixed channel quad per thread
    const bool a_ok = (ci0 + qa * 4) < p.cin_p, g_ok = (co0 + qg * 4) < p.cout_p;
    const bool has_xf = p.in_scale != nullptr;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_xf && a_ok) {
        sc = *reinterpret_cast<const float4*>(p.in_scale + ci0 + qa * 4);
        sh = *reinterpret_cast<const float4*>(p.in_shift + ci0 + qa * 4);
    }
    f32x4 acc[8][MI][NJ];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int a = 0; a < MI; ++a)
#pragma unroll
            for (int b = 0; b < NJ; ++b) acc[t][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 gsum = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int64_t v0 = (int64_t)tile * 64;
        __syncthreads();
        for (int it = tid; it < 64 * QA; it += 256) {
            const int vl = it / QA;
            const int64_t v = v0 + vl;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a_ok && v < p.nvox) {
                val = *reinterpret_cast<const float4*>(p.in + (size_t)v * p.in_cs + ci0 + qa * 4);
                if (has_xf) val = xform4(val, sc, sh, p.in_relu);
            }
            *reinterpret_cast<float4*>(&sA[vl * CA + qa * 4]) = val;
        }
        // a thread owns channel quad qg of QG/4 voxels (vl = tid / QG + j * (256 / QG)); one 32-bit index decode per voxel
#pragma unroll
        for (int j = 0; j < QG / 4; ++j) {
            const int vl = tid / QG + j * (256 / QG);
            const int64_t v = v0 + vl;
            const bool ok = g_ok && v < p.nvox;
            // the 8 taps' loads are issued together, branch-free (items outside read voxel 0 / quad 0 and are zeroed)
            const float* gsrc = p.g + (ok ? fine_base(v, p.D, p.H, p.W) : 0) * p.g_cs + (g_ok ? co0 + qg * 4 : 0);
            f32x4 gl[8];
#pragma unroll
            for (int tap = 0; tap < 8; ++tap) gl[tap] = *reinterpret_cast<const f32x4*>(gsrc + (size_t)tap_off(tap, p.H, p.W) * p.g_cs);
#pragma unroll
            for (int tap = 0; tap < 8; ++tap) {
                const float4 gv = ok ? make_float4(gl[tap][0], gl[tap][1], gl[tap][2], gl[tap][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(&sG[(tap * 64 + vl) * CG + qg * 4]) = gv;
                gsum.x += gv.x; gsum.y += gv.y; gsum.z += gv.z; gsum.w += gv.w;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int vl = (wave * 4 + ks) * 4 + kq;
            float a[MI];
#pragma unroll
            for (int x = 0; x < MI; ++x) a[x] = sA[vl * CA + x * 16 + i];
#pragma unroll
            for (int tap = 0; tap < 8; ++tap) {
#pragma unroll
                for (int y = 0; y < NJ; ++y) {
                    const float b = sG[(tap * 64 + vl) * CG + y * 16 + i];
#pragma unroll
                    for (int x = 0; x < MI; ++x)
                        acc[tap][x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x], b, acc[tap][x][y], 0, 0, 0);
                }
            }
        }
    }
    // 4 waves -> one slab [8][MI][NJ][16 ci][16 co] per block, through sG (8 taps per round need 4*8*MI*NJ*256 floats)
    float* dst = p.ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (8 * MI * NJ * 256);
    constexpr int TPR = (8 * 64 * CG) / (4 * MI * NJ * 256);        // taps per round that fit in sG
    static_assert(TPR >= 1, "reduction scratch");
    for (int t0 = 0; t0 < 8; t0 += TPR) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (t >= t0 && t < t0 + TPR)
#pragma unroll
                for (int x = 0; x < MI; ++x)
#pragma unroll
                    for (int y = 0; y < NJ; ++y)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            sG[((wave * TPR + (t - t0)) * MI * NJ + x * NJ + y) * 256 + (kq * 4 + r) * 16 + i] = acc[t][x][y][r];
        __syncthreads();
        const int nel = ((8 - t0) < TPR ? (8 - t0) : TPR) * MI * NJ * 256, stride = TPR * MI * NJ * 256;
        for (int e = tid; e < nel; e += 256)
            dst[t0 * MI * NJ * 256 + e] = (sG[e] + sG[stride + e]) + (sG[2 * stride + e] + sG[3 * stride + e]);
    }
    // bias-gradient partials: threads with the same channel quad, only the blocks of the first ci group
    if (cig == 0 && wsb) {
        __syncthreads();
        *reinterpret_cast<float4*>(&sA[tid * 4]) = gsum;
        __syncthreads();
        if (tid < CG) {
            const int q = tid >> 2, c = tid & 3;
            float t = 0.f;
            for (int k = q; k < 256; k += QG) t += sA[k * 4 + c];
            wsb[((size_t)cog * gridDim.x + blockIdx.x) * CG + tid] = t;
        }
    }
}

// dw[ci][co][tap]: a block owns 64 consecutive outputs (co fastest) and sums the gx slabs of their tile group.
template <int MI, int NJ>
__global__ __launch_bounds__(1024) void convt2_wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wsb,
                                                                   float* __restrict__ dw, float* __restrict__ dbias, int Ci,
                                                                   int Co, const int32_t* __restrict__ imap, int n_ci_t,
                                                                   int gx) {
    __shared__ float red[RPARTS][64];
    convt2_wgrad_reduce_block<MI, NJ>(ws, wsb, dw, dbias, Ci, Co, imap, n_ci_t, gx, blockIdx.x, threadIdx.x, red);
}

// ------------------------------------------------------------------ launch plans (host only)
// The plan of a forward / data-gradient launch: ctu_convt2_plan and launch_convt read this one function.
// The kernel stages GMAX = 8 float4 items per thread, which covers 64 voxels x rin_p channels only up to rin_p = 128.
inline bool ct_channels_ok(int rin_p, int nout_p) {
    return rin_p > 0 && rin_p % 8 == 0 && rin_p <= 128 && nout_p > 0 && nout_p % 8 == 0 && nout_p <= 128;
}

struct CtPlan {
    int ntt_total, ntt;      // 16-wide output tiles in the packed weights / per block
    int gx, gy;              // blocks of 64 coarse voxels x groups of ntt tiles
    int tps;                 // taps staged per barrier pair
    size_t lds;              // dynamic LDS bytes
    const char* name;
};

inline CtPlan ct_plan(int mode, int rin_p, int nout_p, int64_t nvox) {
    static const char* const names[2][4] = {
        {"convt2_kernel<1, 0>", "convt2_kernel<2, 0>", "convt2_kernel<4, 0>", "convt2_kernel<8, 0>"},
        {"convt2_kernel<1, 1>", "convt2_kernel<2, 1>", "convt2_kernel<4, 1>", "convt2_kernel<8, 1>"}};
    CtPlan r;
    r.ntt_total = pick_ntt(nout_p);
    r.gx = (int)ceil_div64(nvox, 64);
    r.ntt = r.ntt_total;                                   // tiles per block: split across blockIdx.y until the grid fills the chip
    while (r.ntt > 1 && (long)r.gx * (r.ntt_total / r.ntt) < 256) r.ntt >>= 1;
    r.gy = r.ntt_total / r.ntt;
    const size_t a_b = (size_t)64 * (rin_p + 4) * sizeof(float);
    const size_t w_b = (size_t)(rin_p / 8) * r.ntt * 128 * sizeof(float);      // one tap's share of the packed weights
    r.tps = 8;
    while (r.tps > 1 && a_b + r.tps * w_b > 72 * 1024) r.tps >>= 1;
    r.lds = a_b + r.tps * w_b;
    r.name = names[mode ? 1 : 0][r.ntt == 1 ? 0 : (r.ntt == 2 ? 1 : (r.ntt == 4 ? 2 : 3))];
    return r;
}

// The plan of a weight-gradient launch: ctu_convt2_wgrad_ws_floats, ctu_convt2_wgrad_plan and ctu_convt2_wgrad read it.
struct CtWgPlan {
    int mi, nj;              // 16-channel tiles per block (input side, output side)
    int n_ci_t, n_co_t;      // channel groups: grid.y = n_ci_t * n_co_t
    int ntiles, gx;          // 64-voxel tiles; a block walks tiles blockIdx.x, blockIdx.x + gx, ...
    const char* name;
};

inline CtWgPlan ct_wgrad_plan(int64_t nvox, int cin_p, int cout_p) {
    static const char* const names[2][2] = {{"convt2_wgrad_kernel<1, 1>", "convt2_wgrad_kernel<1, 2>"},
                                            {"convt2_wgrad_kernel<2, 1>", "convt2_wgrad_kernel<2, 2>"}};
    CtWgPlan r;
    r.mi = cin_p > 16 ? 2 : 1;
    r.nj = cout_p > 16 ? 2 : 1;
    r.n_ci_t = ceil_div(cin_p, 16 * r.mi);
    r.n_co_t = ceil_div(cout_p, 16 * r.nj);
    r.ntiles = (int)ceil_div64(nvox, 64);
    r.gx = 512 / (r.n_ci_t * r.n_co_t);
    if (r.gx < 1) r.gx = 1;
    if (r.gx > r.ntiles) r.gx = r.ntiles;
    r.name = names[r.mi - 1][r.nj - 1];
    return r;
}

template <int MODE>
int launch_convt(const CtP& p, hipStream_t st, const char* name) {
    CTU_REQUIRE(p.nvox < (1LL << 31), "%s: more than 2^31 coarse voxels", name);
    const CtPlan r = ct_plan(MODE, p.rin_p, p.nout_p, p.nvox);
    const size_t lds = r.lds;
    const int tps = r.tps;
    CTU_REQUIRE(lds <= 160 * 1024, "%s: rin_p=%d nout_p=%d needs %zu B of LDS", name, p.rin_p, p.nout_p, lds);
    CTU_REQUIRE(p.out_cs % 4 == 0 && ((uintptr_t)p.out & 15) == 0, "%s: output must be 16-byte aligned", name);
    CtP q = p;
    q.ntt_total = r.ntt_total;
    const dim3 grid2(r.gx, r.gy);
#define CT_LAUNCH(N_)                                                                                             \
    do {                                                                                                          \
        if (lds > 64 * 1024)                                                                                      \
            (void)hipFuncSetAttribute((const void*)convt2_kernel<N_, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                      (int)lds);                                                                  \
        convt2_kernel<N_, MODE><<<grid2, 256, lds, st>>>(q, tps);                                                 \
    } while (0)
    switch (r.ntt) {
        case 1: CT_LAUNCH(1); break;
        case 2: CT_LAUNCH(2); break;
        case 4: CT_LAUNCH(4); break;
        default: CT_LAUNCH(8); break;
    }
#undef CT_LAUNCH
    CTU_CHECK_LAUNCH(name);
    return CTU_OK;
}

}  // namespace

// =================================================================== C ABI
extern "C" size_t ctu_convt_packed_floats(int rin_p, int nout_p) {
    if (rin_p <= 0 || nout_p <= 0) return 0;
    return (size_t)8 * (rin_p / 8) * pick_ntt(nout_p) * 128;
}

extern "C" int ctu_pack_convt_weight(const float* w, float* wp, int Ci, int Co, const int32_t* cinv, int rin_p,
                                     int nout_p, int mode, void* stream) {
    CTU_REQUIRE(w && wp && Ci > 0 && Co > 0, "pack_convt_weight: null/empty");
    CTU_REQUIRE(rin_p % 8 == 0 && nout_p % 8 == 0 && nout_p <= 128, "pack_convt_weight: rin_p=%d nout_p=%d", rin_p,
                nout_p);
    hipStream_t st = (hipStream_t)stream;
    const int total = (int)ctu_convt_packed_floats(rin_p, nout_p);
    pack_convt_w_kernel<<<ceil_div(total, 256), 256, 0, st>>>(w, wp, Ci, Co, cinv, rin_p, pick_ntt(nout_p), mode);
    CTU_CHECK_LAUNCH("pack_convt_weight");
    return CTU_OK;
}

extern "C" int ctu_convt2_fwd(const float* in, int in_cs, int rin_p, const float* in_scale, const float* in_shift,
                              int in_relu, const float* wp, const float* bias, int nbias, float* out, int out_cs,
                              int nout_p, int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(in && wp && out, "convt2_fwd: null pointer");
    CTU_REQUIRE(ct_channels_ok(rin_p, nout_p), "convt2_fwd: rin_p=%d nout_p=%d (multiples of 8, at most 128)", rin_p, nout_p);
    CTU_REQUIRE(in_cs >= rin_p && in_cs % 4 == 0 && out_cs >= nout_p, "convt2_fwd: bad stride");
    CTU_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "convt2_fwd: scale/shift must come together");
    CtP p;
    p.in = in; p.in_scale = in_scale; p.in_shift = in_shift; p.wp = wp; p.bias = bias; p.out = out;
    p.in_cs = in_cs; p.rin_p = rin_p; p.in_relu = in_relu; p.out_cs = out_cs; p.nout_p = nout_p;
    p.nbias = bias ? nbias : 0;
    p.N = N; p.D = D; p.H = H; p.W = W; p.nvox = (int64_t)N * D * H * W;
    return launch_convt<0>(p, (hipStream_t)stream, "convt2_fwd");
}

extern "C" int ctu_convt2_bwd_data(const float* gout, int g_cs, int rout_p, const float* wp, float* gin, int gin_cs,
                                   int nin_p, int N, int D, int H, int W, void* stream) {
    CTU_REQUIRE(gout && wp && gin, "convt2_bwd_data: null pointer");
    CTU_REQUIRE(ct_channels_ok(rout_p, nin_p), "convt2_bwd_data: rout_p=%d nin_p=%d (multiples of 8, at most 128)", rout_p, nin_p);
    CTU_REQUIRE(g_cs >= rout_p && g_cs % 4 == 0 && gin_cs >= nin_p, "convt2_bwd_data: bad stride");
    CtP p;
    p.in = gout; p.in_scale = nullptr; p.in_shift = nullptr; p.wp = wp; p.bias = nullptr; p.out = gin;
    p.in_cs = g_cs; p.rin_p = rout_p; p.in_relu = 0; p.out_cs = gin_cs; p.nout_p = nin_p; p.nbias = 0;
    p.N = N; p.D = D; p.H = H; p.W = W; p.nvox = (int64_t)N * D * H * W;
    return launch_convt<1>(p, (hipStream_t)stream, "convt2_bwd_data");
}

extern "C" size_t ctu_convt2_wgrad_ws_floats(int N, int D, int H, int W, int cin_p, int cout_p) {
    const CtWgPlan r = ct_wgrad_plan((int64_t)N * D * H * W, cin_p, cout_p);
    return (size_t)r.n_ci_t * r.n_co_t * r.gx * 8 * r.mi * r.nj * 256 + (size_t)r.n_co_t * r.gx * 16 * r.nj;
}

template <int MI, int NJ>
static int launch_ct_wgrad(CtWgP p, float* dw, float* dbias, int Ci, int Co, const int32_t* imap, int n_co_t, int gx,
                           hipStream_t st, ctu_wgrad_job* job) {
    float* wsb = p.ws + (size_t)p.n_ci_t * n_co_t * gx * 8 * MI * NJ * 256;
    convt2_wgrad_kernel<MI, NJ><<<dim3(gx, p.n_ci_t * n_co_t), 256, 0, st>>>(p, dbias ? wsb : nullptr);
    CTU_CHECK_LAUNCH("convt2_wgrad");
    if (job) {                                     // the caller reduces the slabs later (wsb = ws + pairs * gx * slab floats)
        *job = ctu_wgrad_job{};
        job->kind = WGJ_CONVT + (MI - 1) * 2 + (NJ - 1);
        job->ws = p.ws; job->dw = dw; job->db = dbias; job->cinv = imap;
        job->Co = Co; job->Ci = Ci; job->cin_p = p.cin_p; job->n_ci_g = p.n_ci_t; job->gx = gx; job->pairs = p.n_ci_t * n_co_t;
        job->nmf = 8 * MI * NJ;
        return CTU_OK;
    }
    convt2_wgrad_reduce_kernel<MI, NJ><<<ceil_div(Ci * Co * 8 + Co, 64), 64 * RPARTS, 0, st>>>(p.ws, wsb, dw, dbias, Ci, Co, imap,
                                                                                           p.n_ci_t, gx);
    CTU_CHECK_LAUNCH("convt2_wgrad_reduce");
    return CTU_OK;
}

static int convt2_wgrad_impl(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                             int in_relu, const float* gout, int g_cs, int cout_p, float* dw, float* dbias, int Ci,
                             int Co, const int32_t* imap, float* ws, int N, int D, int H, int W, ctu_wgrad_job* job,
                             void* stream) {
    CTU_REQUIRE(in && gout && dw && ws, "convt2_wgrad: null pointer");
    CTU_REQUIRE(cin_p % 8 == 0 && cout_p % 8 == 0 && cin_p > 0 && cout_p > 0, "convt2_wgrad: padded channels");
    CTU_REQUIRE(in_cs >= cin_p && in_cs % 4 == 0 && g_cs >= cout_p && g_cs % 4 == 0, "convt2_wgrad: bad stride");
    hipStream_t st = (hipStream_t)stream;
    CtWgP p;
    p.in = in; p.in_scale = in_scale; p.in_shift = in_shift; p.g = gout; p.ws = ws;
    p.in_cs = in_cs; p.cin_p = cin_p; p.in_relu = in_relu; p.g_cs = g_cs; p.cout_p = cout_p;
    p.N = N; p.D = D; p.H = H; p.W = W; p.nvox = (int64_t)N * D * H * W;
    CTU_REQUIRE(p.nvox < (1LL << 31), "convt2_wgrad: more than 2^31 coarse voxels");
    const CtWgPlan r = ct_wgrad_plan(p.nvox, cin_p, cout_p);
    p.ntiles = r.ntiles; p.n_ci_t = r.n_ci_t;
    const int mi = r.mi, nj = r.nj, n_co_t = r.n_co_t, gx = r.gx;
    if (mi == 1 && nj == 1) return launch_ct_wgrad<1, 1>(p, dw, dbias, Ci, Co, imap, n_co_t, gx, st, job);
    if (mi == 1) return launch_ct_wgrad<1, 2>(p, dw, dbias, Ci, Co, imap, n_co_t, gx, st, job);
    if (nj == 1) return launch_ct_wgrad<2, 1>(p, dw, dbias, Ci, Co, imap, n_co_t, gx, st, job);
    return launch_ct_wgrad<2, 2>(p, dw, dbias, Ci, Co, imap, n_co_t, gx, st, job);
}

extern "C" int ctu_convt2_wgrad(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                                int in_relu, const float* gout, int g_cs, int cout_p, float* dw, float* dbias, int Ci,
                                int Co, const int32_t* imap, float* ws, int N, int D, int H, int W, void* stream) {
    return convt2_wgrad_impl(in, in_cs, cin_p, in_scale, in_shift, in_relu, gout, g_cs, cout_p, dw, dbias, Ci, Co, imap, ws,
                             N, D, H, W, nullptr, stream);
}

extern "C" int ctu_convt2_wgrad_slabs(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                                      int in_relu, const float* gout, int g_cs, int cout_p, float* dw, float* dbias, int Ci,
                                      int Co, const int32_t* imap, float* ws, int N, int D, int H, int W, ctu_wgrad_job* job,
                                      void* stream) {
    CTU_REQUIRE(job, "convt2_wgrad_slabs: null job");
    return convt2_wgrad_impl(in, in_cs, cin_p, in_scale, in_shift, in_relu, gout, g_cs, cout_p, dw, dbias, Ci, Co, imap, ws,
                             N, D, H, W, job, stream);
}

// Host-only plan queries (no GPU): the instantiation a call of this geometry launches, or NULL where the call is refused.
// plan[4] = grid.x, grid.y, taps staged per barrier pair, dynamic LDS bytes.  mode 0 forward, 1 data gradient
// (rin_p = the reduction side: padded input channels resp. padded channels of the gradient).
extern "C" const char* ctu_convt2_plan(int mode, int rin_p, int nout_p, int N, int D, int H, int W, int* plan) {
    const int64_t nvox = (int64_t)N * D * H * W;
    if ((mode != 0 && mode != 1) || !ct_channels_ok(rin_p, nout_p) || N <= 0 || D <= 0 || H <= 0 || W <= 0 || nvox >= (1LL << 31))
        return nullptr;
    const CtPlan r = ct_plan(mode, rin_p, nout_p, nvox);
    if (r.lds > 160 * 1024) return nullptr;
    if (plan) { plan[0] = r.gx; plan[1] = r.gy; plan[2] = r.tps; plan[3] = (int)r.lds; }
    return r.name;
}

// plan[3] = grid.x (slabs per channel group), grid.y (channel groups), 64-voxel tiles the grid.x blocks share
extern "C" const char* ctu_convt2_wgrad_plan(int cin_p, int cout_p, int N, int D, int H, int W, int* plan) {
    const int64_t nvox = (int64_t)N * D * H * W;
    if (cin_p <= 0 || cin_p % 8 || cout_p <= 0 || cout_p % 8 || N <= 0 || D <= 0 || H <= 0 || W <= 0 || nvox >= (1LL << 31))
        return nullptr;
    const CtWgPlan r = ct_wgrad_plan(nvox, cin_p, cout_p);
    if (plan) { plan[0] = r.gx; plan[1] = r.n_ci_t * r.n_co_t; plan[2] = r.ntiles; }
    return r.name;
}
