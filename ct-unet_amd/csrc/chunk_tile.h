// The output tiling of the gather kernels (resample, affine_resample, spatial_warp): a block of SB = 256 threads owns a tile
// of TZ = 4 planes x TY = 4 rows x LXN = 16 chunks of a [d][h][w] output.  A chunk is the 16 bytes one thread writes
// (VX = 16 / sizeof(O) voxels), laid on the 16-byte grid of its own output row: row r of tile column X0 starts its chunks
// at X0 - e_r, e_r = the misalignment of r's voxel X0 in voxels.  So every whole chunk is one 16-byte store whatever the row
// length or the alignment of `out`, and the clipped chunks at a row's two ends are stored voxel by voxel.  Nothing is
// written outside [0, w) of a row: a Span with xa >= xb owns nothing and its thread must leave.  affine_kernel writes
// store() out in its own file (profiles/shared_volume_helpers.md says why) and takes everything else from here.
#pragma once
#include "common.h"

namespace ctu_tile {

constexpr int SB = 256;
constexpr int LXN = 16;                         // chunks of a tile along x
constexpr int TY = 4, TZ = 4;                   // rows and planes of a tile: LXN * TY * TZ = SB, one chunk per thread
static_assert(LXN * TY * TZ == SB, "one chunk per thread");

template <class O> struct alignas(16) Chunk { O v[16 / sizeof(O)]; };

// host: tile columns, tile rows and blocks (grid.x) of one item of `osize`-byte voxels at `out`
struct Tiles { int ntx, nty, blocks; };
inline Tiles tiles(int d, int h, int w, const void* out, int osize) {
    const int VX = 16 / osize;
    // rows whose chunks all start at a tile's X0 need no tile column for the shifted remainder
    const bool aligned = w % VX == 0 && (uintptr_t)out % 16 == 0;
    const int ntx = ceil_div(w + (aligned ? 0 : VX - 1), LXN * VX), nty = ceil_div(h, TY);
    return {ntx, nty, ntx * nty * ceil_div(d, TZ)};
}

// the block's tile (first voxel, row and plane) from blockIdx.x
struct Origin { int X0, Y0, Z0; };
template <class O> __device__ __forceinline__ Origin origin(int ntx, int nty) {
    int bi = blockIdx.x;
    const int tx = bi % ntx;
    bi /= ntx;
    return {tx * LXN * (16 / (int)sizeof(O)), bi % nty * TY, bi / nty * TZ};
}

// the thread's row and plane of the tile; the caller leaves when they lie outside the output
__device__ __forceinline__ void row_of(const Origin& t, int& yy, int& zz) {
    const int rs = threadIdx.x / LXN;
    yy = t.Y0 + rs % TY;
    zz = t.Z0 + rs / TY;
}

// output voxels [xa, xb] the block's tile may touch: its rows start up to VX - 1 voxels left of X0.  Empty when xa > xb.
template <class O> __device__ __forceinline__ void block_extent(int X0, int w, int& xa, int& xb) {
    constexpr int VX = 16 / (int)sizeof(O);
    xa = max(X0 - (VX - 1), 0);
    xb = min(X0 + LXN * VX, w) - 1;
}

// the thread's chunk [cx, cx + VX) of the row at `orow` (w voxels) and the part [xa, xb) of it inside the row
struct Span { int cx, xa, xb; };
template <class O> __device__ __forceinline__ Span chunk_of(const O* orow, int X0, int w) {
    constexpr int VX = 16 / (int)sizeof(O);
    const int e = (int)(((uintptr_t)(orow + X0) / sizeof(O)) % VX);
    const int cx = X0 + (int)(threadIdx.x % LXN) * VX - e;
    return {cx, max(cx, 0), min(cx + VX, w)};
}

// `aligned`: orow + s.cx is a multiple of 16 bytes.  True for the row chunk_of() saw; a caller that reuses the span for rows
// at another offset (the later channels of spatial_warp) passes the test of that row's address.
template <class O> __device__ __forceinline__ void store(O* orow, const Span& s, const Chunk<O>& res, bool aligned) {
    constexpr int VX = 16 / (int)sizeof(O);
    if (s.xb - s.xa == VX && aligned) {
        *reinterpret_cast<Chunk<O>*>(orow + s.cx) = res;
    } else {
#pragma unroll
        for (int v = 0; v < VX; ++v)
            if (s.cx + v >= s.xa && s.cx + v < s.xb) orow[s.cx + v] = res.v[v];
    }
}

}  // namespace ctu_tile
