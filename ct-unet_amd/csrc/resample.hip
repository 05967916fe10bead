// Resampling of 3-D volumes between voxel grids, gfx950: nearest, trilinear and label-aware trilinear, driven by per-axis
// tables that the host forms in float64 (rule and tables: ctunet_amd/resample.py; tests/resample_ref.py restates them).
//
// One launch per call, no atomics, no host synchronisation.  The output is tiled by chunk_tile.h: a block of 256 threads owns
// 4 planes x 4 rows x 16 chunks; a chunk is the 16 bytes of output that one thread writes (VX = 2 int64 / 4 float, int32 /
// 8 int16 / 16 uint8 voxels) on the 16-byte grid of its output row, so a wave covers four rows of 256 contiguous bytes each.
//   staged route:  the tile's three table ranges span an input box; the block copies that box into LDS once (coalesced along
//                  x, in the input's own dtype: int16 / uint8 are converted when they are read back) and every output reads
//                  its 8 (linear) or 1 (nearest) inputs from there.  label_linear reads the 8 labels once for all classes.
//   gather route:  when the box does not fit the LDS of the launch (steep down-sampling) the same code reads the input
//                  through the tables directly.  The choice is block-uniform: it follows from the tables' first and last
//                  entries of the tile.  The launch's LDS size is only the host's estimate of the box from n / m; a box
//                  that the estimate misses takes the gather route, so the estimate never changes a result.
// Arithmetic of linear / label_linear: trilinear.h (lerp, tri and label_vote, every operation rounded on its own; contraction
// is off there and for this file, and the assembly holds no fused multiply-add).  No one-hot or score volume exists in memory.
// Measured: profiles/resample.md.
//
// No reference counterpart: the reference resizes volumes on the host in its datasets (ctunet/pytorch/datasets.py:89-112).
#include <type_traits>

#include "chunk_tile.h"
#include "common.h"
#include "trilinear.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_tile;
using namespace ctu_tri;

constexpr int LDS_CAP = 64 * 1024;              // dynamic LDS a launch may ask for without raising the limit
constexpr int MAX_BATCH = 65535;                // grid.y

struct RsArgs {
    int D, H, W;                                // input grid
    int d, h, w;                                // output grid
    int ntx, nty;
    int lds_elems;                              // input voxels the launch's LDS holds
    int K;
    const int32_t* i0;                          // [d + h + w]: z, y, x tables
    const float* wt;
    const int32_t* near;
};

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// The thread's chunk of the tile from `p`: the LDS box (origin (oz, oy, ox), extents (ez, ey, ex)) or the item itself
// (origin 0, extents (D, H, W)).  Every index is clamped to the extents, so a table can never take a read outside them.
template <class T, int MODE>
__device__ __forceinline__ void tile_chunk(const RsArgs& a, const T* __restrict__ p, int oz, int oy, int ox, int ez, int ey,
                                           int ex, const Origin& t, typename OutOf<T, MODE>::type* __restrict__ out_item) {
    typedef typename OutOf<T, MODE>::type O;
    constexpr int VX = 16 / (int)sizeof(O);
    int yy, zz;
    row_of(t, yy, zz);
    if (yy >= a.h || zz >= a.d) return;
    O* orow = out_item + ((int64_t)zz * a.h + yy) * a.w;
    const Span s = chunk_of(orow, t.X0, a.w);
    if (s.xa >= s.xb) return;
    const int cx = s.cx;
    const int sy = ex, sz = ex * ey;
    const int32_t* tabx = (MODE == NEAREST ? a.near : a.i0) + a.d + a.h;
    Chunk<O> res;
    if constexpr (MODE == NEAREST) {
        const int row = clampi(a.near[zz] - oz, ez - 1) * sz + clampi(a.near[a.d + yy] - oy, ey - 1) * sy;
#pragma unroll
        for (int u = 0; u < VX; ++u) res.v[u] = p[row + clampi(tabx[clampi(cx + u, a.w - 1)] - ox, ex - 1)];
    } else {
        const int za = a.i0[zz], ya = a.i0[a.d + yy];
        const float wz = a.wt[zz], wy = a.wt[a.d + yy];
        const int z0 = clampi(za - oz, ez - 1) * sz, z1 = clampi(min(za + 1, a.D - 1) - oz, ez - 1) * sz;
        const int y0 = clampi(ya - oy, ey - 1) * sy, y1 = clampi(min(ya + 1, a.H - 1) - oy, ey - 1) * sy;
        const int r00 = z0 + y0, r01 = z0 + y1, r10 = z1 + y0, r11 = z1 + y1;
        const float* wtx = a.wt + a.d + a.h;
#pragma unroll
        for (int u = 0; u < VX; ++u) {
            const int x = clampi(cx + u, a.w - 1);
            const int xi = tabx[x];
            const float wx = wtx[x];
            const int x0 = clampi(xi - ox, ex - 1), x1 = clampi(min(xi + 1, a.W - 1) - ox, ex - 1);
            const T v[8] = {p[r00 + x0], p[r00 + x1], p[r01 + x0], p[r01 + x1], p[r10 + x0], p[r10 + x1], p[r11 + x0], p[r11 + x1]};
            if constexpr (MODE == LINEAR) {
                float c[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) c[j] = (float)v[j];
                res.v[u] = tri(c, wx, wy, wz);
            } else {
                res.v[u] = (O)label_vote(v, a.K, wx, wy, wz);
            }
        }
    }
    store(orow, s, res, true);
}

template <class T, int MODE>
__global__ void __launch_bounds__(SB) resample_kernel(RsArgs a, const T* __restrict__ in,
                                                      typename OutOf<T, MODE>::type* __restrict__ out) {
    typedef typename OutOf<T, MODE>::type O;
    extern __shared__ __align__(16) unsigned char smem[];
    T* box = reinterpret_cast<T*>(smem);
    const Origin t = origin<O>(a.ntx, a.nty);
    int xa, xb;
    block_extent<O>(t.X0, a.w, xa, xb);
    if (xa > xb) return;                                       // block-uniform
    const int yb = min(t.Y0 + TY, a.h) - 1, zb = min(t.Z0 + TZ, a.d) - 1;
    const int32_t* tab = MODE == NEAREST ? a.near : a.i0;
    const int up = MODE == NEAREST ? 0 : 1;                    // linear reads i0 and i0 + 1
    const int oz = clampi(tab[t.Z0], a.D - 1), oy = clampi(tab[a.d + t.Y0], a.H - 1), ox = clampi(tab[a.d + a.h + xa], a.W - 1);
    const int ez = max(clampi(tab[zb] + up, a.D - 1) - oz + 1, 1);
    const int ey = max(clampi(tab[a.d + yb] + up, a.H - 1) - oy + 1, 1);
    const int ex = max(clampi(tab[a.d + a.h + xb] + up, a.W - 1) - ox + 1, 1);
    const T* item = in + (int64_t)blockIdx.y * a.D * a.H * a.W;
    O* out_item = out + (int64_t)blockIdx.y * a.d * a.h * a.w;
    if ((int64_t)ex * ey * ez <= a.lds_elems) {
        // 64 lanes along x, 4 box rows at a time
        const int lane = threadIdx.x & 63;
        for (int r = threadIdx.x >> 6; r < ey * ez; r += SB / 64) {
            const int z = r / ey, y = r - z * ey;
            const T* src = item + ((int64_t)(oz + z) * a.H + (oy + y)) * a.W + ox;
            T* dst = box + r * ex;
            for (int x = lane; x < ex; x += 64) dst[x] = src[x];
        }
        __syncthreads();
        tile_chunk<T, MODE>(a, box, oz, oy, ox, ez, ey, ex, t, out_item);
    } else {
        tile_chunk<T, MODE>(a, item, 0, 0, 0, a.D, a.H, a.W, t, out_item);
    }
}

// input voxels along one axis that `t` output voxels of an n -> m axis span, from n / m alone (the kernel decides from the
// tables; this only sizes the LDS)
int span(int t, int n, int m) {
    const int64_t s = ((int64_t)(t < m ? t : m) * n + m - 1) / m + 3;
    return (int)(s < n ? s : n);
}

template <class T, int MODE>
int launch(const void* in, int64_t N, int D, int H, int W, int d, int h, int w, int K, const int32_t* i0, const float* wt,
           const int32_t* near, void* out, hipStream_t st) {
    typedef typename OutOf<T, MODE>::type O;
    constexpr int VX = 16 / (int)sizeof(O);
    constexpr int TXO = LXN * VX;
    RsArgs a;
    a.D = D; a.H = H; a.W = W; a.d = d; a.h = h; a.w = w;
    a.K = K; a.i0 = i0; a.wt = wt; a.near = near;
    const Tiles tl = tiles(d, h, w, out, sizeof(O));
    a.ntx = tl.ntx;
    a.nty = tl.nty;
    const int64_t est = (int64_t)span(TXO + VX - 1, W, w) * span(TY, H, h) * span(TZ, D, d) * (int64_t)sizeof(T);
    const size_t lds = est <= LDS_CAP ? (size_t)est : 0;       // 0: every block gathers
    a.lds_elems = (int)(lds / sizeof(T));
    const int64_t vin = (int64_t)D * H * W, vout = (int64_t)d * h * w;
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const int64_t nb = N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH;
        const dim3 grid((unsigned)tl.blocks, (unsigned)nb);
        resample_kernel<T, MODE><<<grid, SB, lds, st>>>(a, (const T*)in + n0 * vin, (O*)out + n0 * vout);
        CTU_CHECK_LAUNCH("resample");
    }
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W, int d,
                            int h, int w, const int32_t* i0, const float* wt, const int32_t* near, void* out, void* stream) {
    CTU_REQUIRE(in && out && i0 && wt && near, "resample: null pointer");
    CTU_REQUIRE(mode >= NEAREST && mode <= LABEL, "resample: unknown mode %d", mode);
    CTU_REQUIRE(N > 0 && grid_ok(D, H, W) && grid_ok(d, h, w),
                "resample: bad shape N=%lld in=%dx%dx%d out=%dx%dx%d (every side >= 1, D*H*W < 2^31 on either grid)",
                (long long)N, D, H, W, d, h, w);
    if (mode == LABEL)
        CTU_REQUIRE(num_classes >= 2 && num_classes <= 16, "resample: num_classes must lie in 2..16, got %d", num_classes);
    hipStream_t st = (hipStream_t)stream;
#define RS(T, MODE) return launch<T, MODE>(in, N, D, H, W, d, h, w, num_classes, i0, wt, near, out, st)
    if (mode == NEAREST) {                                      // a copy of bits: by element size
        if (dtype == CTU_U8) RS(uint8_t, NEAREST);
        if (dtype == CTU_I16) RS(uint16_t, NEAREST);
        if (dtype == CTU_I32 || dtype == CTU_F32) RS(uint32_t, NEAREST);
        if (dtype == CTU_I64) RS(unsigned long long, NEAREST);
        CTU_REQUIRE(false, "resample: unsupported dtype %d for nearest (uint8, int16, int32, int64 or float32)", dtype);
    }
    if (mode == LINEAR) {
        if (dtype == CTU_F32) RS(float, LINEAR);
        if (dtype == CTU_I16) RS(int16_t, LINEAR);
        if (dtype == CTU_U8) RS(uint8_t, LINEAR);
        CTU_REQUIRE(false, "resample: unsupported dtype %d for linear (float32, int16 or uint8)", dtype);
    }
    if (dtype == CTU_U8) RS(uint8_t, LABEL);
    if (dtype == CTU_I64) RS(long long, LABEL);
#undef RS
    CTU_REQUIRE(false, "resample: unsupported dtype %d for label_linear (uint8 or int64)", dtype);
}
