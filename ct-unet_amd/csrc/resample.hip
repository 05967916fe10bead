// Resampling of 3-D volumes between voxel grids, gfx950: nearest, trilinear and label-aware trilinear, driven by per-axis
// tables that the host forms in float64 (rule and tables: ctunet_amd/resample.py; tests/resample_ref.py restates them).
//
// One launch per call, no atomics, no host synchronisation.  A block of 256 threads owns an output tile of 4 planes x 4 rows
// x 16 chunks; a chunk is the 16 bytes of output that one thread writes (VX = 2 int64 / 4 float, int32 / 8 int16 / 16 uint8
// voxels), so a wave covers four rows of 256 contiguous bytes each.  Chunks are laid on the 16-byte grid of each output row
// (row r of tile column X0 starts its chunks at X0 - e_r, e_r = the row's misalignment in voxels), so every whole chunk is
// one 16-byte store whatever the row length; the clipped chunks at a row's two ends are stored voxel by voxel.
//   staged route:  the tile's three table ranges span an input box; the block copies that box into LDS once (coalesced along
//                  x, in the input's own dtype: int16 / uint8 are converted when they are read back) and every output reads
//                  its 8 (linear) or 1 (nearest) inputs from there.  label_linear reads the 8 labels once for all classes.
//   gather route:  when the box does not fit the LDS of the launch (steep down-sampling) the same code reads the input
//                  through the tables directly.  The choice is block-uniform: it follows from the tables' first and last
//                  entries of the tile.  The launch's LDS size is only the host's estimate of the box from n / m; a box
//                  that the estimate misses takes the gather route, so the estimate never changes a result.
// Arithmetic of linear / label_linear: lerp(p, q, w) = p + w (q - p), every operation rounded on its own (contraction is
// off for the file; the assembly holds no fused multiply-add), four lerps along x, two along y, one along z.
// label_linear evaluates only the classes present among the 8 corner labels, in increasing order, and keeps the first
// strict maximum starting from (class 0, score 0): an absent class scores exactly 0 and no score is negative, so this is
// the smallest class of the largest score over all K classes.  No one-hot or score volume exists in memory.
// Measured: profiles/resample.md.
//
// No reference counterpart: the reference resizes volumes on the host in its datasets (ctunet/pytorch/datasets.py:89-112).
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SB = 256;
constexpr int LXN = 16;                         // chunks of a tile along x
constexpr int TY = 4, TZ = 4;                   // rows and planes of a tile: LXN * TY * TZ = SB, one chunk per thread
constexpr int LDS_CAP = 64 * 1024;              // dynamic LDS a launch may ask for without raising the limit
constexpr int MAX_BATCH = 65535;                // grid.y
constexpr int NEAREST = CTU_RESAMPLE_NEAREST, LINEAR = CTU_RESAMPLE_LINEAR, LABEL = CTU_RESAMPLE_LABEL_LINEAR;
constexpr int NO_CLASS = 31;                    // a label >= K: belongs to no class

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

template <class T, int MODE> struct OutOf { typedef T type; };
template <class T> struct OutOf<T, LINEAR> { typedef float type; };

template <class O> struct alignas(16) Chunk { O v[16 / sizeof(O)]; };

// plain operators under this file's contract(off): the __f*_rn functions of the HIP headers are compiled under the
// headers' own contraction setting, and a multiplication and an addition inlined from them were fused into one FMA here
__device__ __forceinline__ float lerp(float p, float q, float w) {
    const float d = q - p;
    const float t = w * d;
    return p + t;
}

__device__ __forceinline__ float tri(const float c[8], float wx, float wy, float wz) {
    const float c00 = lerp(c[0], c[1], wx), c01 = lerp(c[2], c[3], wx), c10 = lerp(c[4], c[5], wx), c11 = lerp(c[6], c[7], wx);
    return lerp(lerp(c00, c01, wy), lerp(c10, c11, wy), wz);
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// The thread's chunk of the tile from `p`: the LDS box (origin (oz, oy, ox), extents (ez, ey, ex)) or the item itself
// (origin 0, extents (D, H, W)).  Every index is clamped to the extents, so a table can never take a read outside them.
template <class T, int MODE>
__device__ __forceinline__ void tile_chunk(const RsArgs& a, const T* __restrict__ p, int oz, int oy, int ox, int ez, int ey,
                                           int ex, int X0, int Y0, int Z0, typename OutOf<T, MODE>::type* __restrict__ out_item) {
    typedef typename OutOf<T, MODE>::type O;
    constexpr int VX = 16 / (int)sizeof(O);
    const int lane = threadIdx.x % LXN, rs = threadIdx.x / LXN;
    const int yy = Y0 + rs % TY, zz = Z0 + rs / TY;
    if (yy >= a.h || zz >= a.d) return;
    O* orow = out_item + ((int64_t)zz * a.h + yy) * a.w;
    const int e = (int)(((uintptr_t)(orow + X0) / sizeof(O)) % VX);
    const int cx = X0 + lane * VX - e;
    const int xa = max(cx, 0), xb = min(cx + VX, a.w);
    if (xa >= xb) return;
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
                typedef typename std::make_unsigned<T>::type UT;
                int l[8];
                uint32_t present = 0;
                bool same = true;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    l[j] = (UT)v[j] < (UT)a.K ? (int)v[j] : NO_CLASS;
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
                res.v[u] = (O)best;
            }
        }
    }
    if (xb - xa == VX) {
        *reinterpret_cast<Chunk<O>*>(orow + cx) = res;
    } else {
#pragma unroll
        for (int u = 0; u < VX; ++u)
            if (cx + u >= xa && cx + u < xb) orow[cx + u] = res.v[u];
    }
}

template <class T, int MODE>
__global__ void __launch_bounds__(SB) resample_kernel(RsArgs a, const T* __restrict__ in,
                                                      typename OutOf<T, MODE>::type* __restrict__ out) {
    typedef typename OutOf<T, MODE>::type O;
    constexpr int VX = 16 / (int)sizeof(O);
    constexpr int TXO = LXN * VX;
    extern __shared__ __align__(16) unsigned char smem[];
    T* box = reinterpret_cast<T*>(smem);
    int bi = blockIdx.x;
    const int tx = bi % a.ntx;
    bi /= a.ntx;
    const int ty = bi % a.nty, tz = bi / a.nty;
    const int X0 = tx * TXO, Y0 = ty * TY, Z0 = tz * TZ;
    // output voxels the tile may touch: its rows start up to VX - 1 voxels left of X0
    const int xa = max(X0 - (VX - 1), 0), xb = min(X0 + TXO, a.w) - 1;
    if (xa > xb) return;                                       // block-uniform
    const int yb = min(Y0 + TY, a.h) - 1, zb = min(Z0 + TZ, a.d) - 1;
    const int32_t* tab = MODE == NEAREST ? a.near : a.i0;
    const int up = MODE == NEAREST ? 0 : 1;                    // linear reads i0 and i0 + 1
    const int oz = clampi(tab[Z0], a.D - 1), oy = clampi(tab[a.d + Y0], a.H - 1), ox = clampi(tab[a.d + a.h + xa], a.W - 1);
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
        tile_chunk<T, MODE>(a, box, oz, oy, ox, ez, ey, ex, X0, Y0, Z0, out_item);
    } else {
        tile_chunk<T, MODE>(a, item, 0, 0, 0, a.D, a.H, a.W, X0, Y0, Z0, out_item);
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
    // rows whose chunks all start at a tile's X0 need no tile column for the shifted remainder
    const bool aligned = w % VX == 0 && (uintptr_t)out % 16 == 0;
    a.ntx = ceil_div(w + (aligned ? 0 : VX - 1), TXO);
    a.nty = ceil_div(h, TY);
    const int64_t est = (int64_t)span(TXO + VX - 1, W, w) * span(TY, H, h) * span(TZ, D, d) * (int64_t)sizeof(T);
    const size_t lds = est <= LDS_CAP ? (size_t)est : 0;       // 0: every block gathers
    a.lds_elems = (int)(lds / sizeof(T));
    const int64_t vin = (int64_t)D * H * W, vout = (int64_t)d * h * w;
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const int64_t nb = N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH;
        const dim3 grid((unsigned)(a.ntx * a.nty * ceil_div(d, TZ)), (unsigned)nb);
        resample_kernel<T, MODE><<<grid, SB, lds, st>>>(a, (const T*)in + n0 * vin, (O*)out + n0 * vout);
        CTU_CHECK_LAUNCH("resample");
    }
    return CTU_OK;
}

bool grid_ok(int D, int H, int W) { return D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < ((int64_t)1 << 31); }

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
