// Local thickness of 3-D masks (Hildebrand and Ruegsegger 1997), gfx950: every foreground voxel gets the diameter of the
// largest inscribed ball that contains it, from the exact squared distance map of distance.hip, and a per-item summary
// (count, min, max, mean, voxels below a minimum).  Definition and the voxel-centre bias: ctunet_amd/postprocess.py.
//
//   centre q covers p  iff  dd(p, q) < D2(q)  (the open ball; p covers itself),   R2(p) = max {D2(q) : q covers p},
//   thickness(p) = 2 sqrtf(R2(p)), 0 on background, +inf in an item without background.
//   dd: unit spacing the integer dz^2 + dy^2 + dx^2; otherwise fp32 with t_a = float(k_a) s_a and
//   dd = (t_z t_z + t_y t_y) + t_x t_x, every product and sum rounded on its own: the file is compiled with contraction of
//   multiply-adds switched off (the pragma below; HIP's __fmul_rn / __fadd_rn are plain operators and would be contracted).
//
// Form: GATHER.  A block of 512 threads owns a tile of 8^3 output voxels, one voxel per thread with its running maximum in a
// register, and reads the candidate centres cell by cell (cells are the same 8^3 boxes) through a compacted LDS list of
// (z, y, x, D2), which every thread walks as broadcast reads.  No atomics anywhere, so the result does not depend on any order.
// Three launches per chunk of items, all grids fixed by the shape:
//   1. prune:  per cell, a candidate q is dropped iff one of its 26 neighbours q' has D(q') >= D(q) + |q - q'| (every voxel q
//              covers is then covered by q' at a value at least as large; the relation is transitive and has no cycles, so a
//              kept dominator always remains).  Unit spacing: exact in int64, A - B - o >= 0 and (A - B - o)^2 >= 4 B o with
//              A = D2(q'), B = D2(q), o = |q - q'|^2.  Otherwise in fp64 with a relative margin of 1e-5 on the distance, two
//              orders above the rounding of dd; in doubt the candidate stays.  Writes the pruned map and the cell's maximum.
//   2. item max of the cell maxima (one block per item).
//   3. search: bands of D2, (hi / 4, hi] from the item's maximum downwards.  A band's window around the tile is what a ball of
//              radius sqrt(hi) can reach, so it halves from band to band.  A cell of the band is read only if its maximum
//              exceeds the smallest running value of the tile (nothing in it could raise any voxel otherwise) and its box lies
//              nearer than its largest radius; a candidate is staged only if it exceeds that smallest value too.  The bands
//              end as soon as hi is no larger than the tile's smallest value.
// What bounds the search radius: the largest D2 of the item (first band), then hi of each band.
// Cost.  Thin shell (thickness t << 8): every foreground tile reads its 27 nearest cells in two or three bands: about
//   27 x (kept candidates per cell) pair tests per voxel, independent of the volume.  Solid body of radius R: the first
//   bands hold the few cells around the medial axis, whose balls raise nearly every voxel to nearly its final value, after
//   which almost every other cell fails the maximum test; what remains is the window scan of (2 R / 8)^3 cell maxima per
//   tile in the first band, (R / 8)^3 in the second and so on: tiles x R^3 / 64 cheap tests, and pair tests only against the
//   cells near the axis.  The worst case is a body whose pruned candidates all matter (cost ~ voxels x R^3 / (pruning gain)).
// Limits: those of the distance transform: every side <= 1024, D*H*W < 2^31, N <= 65535.
// No host synchronisation, allocation or copy: capture-safe; two calls are bit-equal.
//
// Replaces: nothing in the reference; users would run ImageJ's / BoneJ's local thickness or a Python loop on the host.
#include "common.h"
#include "scan.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)              // the fp32 rule of dd is product by product: no fused multiply-add in this file

namespace {

using ctu_vox::MAX_SIDE;
using ctu_vox::sides_ok;

constexpr int CS = 8;                       // side of a cell and of a tile
constexpr int TB = CS * CS * CS;            // threads per block: one per voxel of the cell / tile
constexpr int HS = CS + 2;                  // side of the prune kernel's halo box
constexpr int CAP = 2048;                   // staged candidates per pass over the LDS list (32 KB)
constexpr int MAXG = 64;                    // items per launch with a spacing table in the kernel arguments
constexpr int MAXU = 65535;                 // items per launch at unit spacing (grid.y)
constexpr uint32_t NOFG = 0xffffffffu;      // "no foreground voxel" in a minimum of keys
constexpr uint32_t INF_KEY_I = 0x7fffffffu; // INT32_MAX: the int32 map of an item without background
constexpr int SB = 256;                     // summary block
constexpr int SPB_MAX = 512;                // summary partial blocks per item

// A squared distance travels as its 32-bit pattern (a "key"): the int32 value, or the bits of the non-negative float32,
// which order like the value.  0 is background in both.
struct TArgs {
    int D, H, W;
    int n0;                                 // first item of this launch (blockIdx.y counts from it)
    int ncz, ncy, ncx;                      // cells per axis
    float sp[MAXG][3];                      // (z, y, x) spacing of each item of the launch (read on the fp32 path only)
};

template <bool FLT> __device__ __forceinline__ float key_value(uint32_t k) {
    if (FLT) return __uint_as_float(k);
    return k == INF_KEY_I ? __builtin_inff() : (float)(int)k;                  // exact below 2^24 (3 * 1023^2 is)
}
template <bool FLT> __device__ __forceinline__ float key_thickness(uint32_t k) {   // 2 sqrt, as distance.hip's finish kernel
    if (FLT) return 2.f * sqrtf(__uint_as_float(k));
    const int n = (int)k;
    if (k == INF_KEY_I) return __builtin_inff();
    return 2.f * (n < (1 << 24) ? sqrtf((float)n) : (float)sqrt((double)n));
}
// the pinned fp32 offset length: products and sums rounded one by one
__device__ __forceinline__ float dd_f32(int kz, int ky, int kx, float sz, float sy, float sx) {
    const float tz = (float)kz * sz, ty = (float)ky * sy, tx = (float)kx * sx;
    const float zz = tz * tz, yy = ty * ty, xx = tx * tx;
    return (zz + yy) + xx;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
// minimum over the block, the same value in every thread; red: one entry per wave.  Every thread must call (two barriers).
__device__ __forceinline__ uint32_t block_min_u32(uint32_t v, uint32_t* red) {
    v = wave_min_u32(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t m = NOFG;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) m = min(m, red[i]);
    __syncthreads();
    return m;
}

// ------------------------------------------------------------------------------------------------ 1. prune + cell maxima
template <bool FLT>
__global__ void __launch_bounds__(TB) thick_prune_kernel(TArgs a, const uint32_t* __restrict__ d2, uint32_t* __restrict__ cand,
                                                         uint32_t* __restrict__ cmax) {
    __shared__ uint32_t halo[HS * HS * HS];
    __shared__ uint32_t red[TB / 64];
    __shared__ double olen[27];             // |o| of the 27 offsets in the item's units (fp32 path)
    const int t = threadIdx.x, il = blockIdx.y;
    const int D = a.D, H = a.H, W = a.W;
    const int cell = blockIdx.x;
    const int cx = cell % a.ncx, cy = (cell / a.ncx) % a.ncy, cz = cell / (a.ncx * a.ncy);
    const int64_t V = (int64_t)D * H * W;
    const int64_t item = (int64_t)(a.n0 + il) * V;
    for (int i = t; i < HS * HS * HS; i += TB) {
        const int hx = i % HS, hy = (i / HS) % HS, hz = i / (HS * HS);
        const int z = cz * CS + hz - 1, y = cy * CS + hy - 1, x = cx * CS + hx - 1;
        uint32_t v = 0;                     // outside the volume: never a dominator
        if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) v = d2[item + ((int64_t)z * H + y) * W + x];
        halo[i] = v;
    }
    if (FLT && t < 27) {
        const double oz = (double)(t / 9 - 1) * (double)a.sp[il][0], oy = (double)((t / 3) % 3 - 1) * (double)a.sp[il][1],
                     ox = (double)(t % 3 - 1) * (double)a.sp[il][2];
        olen[t] = sqrt(oz * oz + oy * oy + ox * ox);
    }
    __syncthreads();
    const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
    const int z = cz * CS + lz, y = cy * CS + ly, x = cx * CS + lx;
    const bool inside = z < D && y < H && x < W;
    const uint32_t B = halo[((lz + 1) * HS + ly + 1) * HS + lx + 1];
    bool keep = inside && B != 0;
    if (keep) {
        double sb = 0.0;
        if (FLT) sb = sqrt((double)__uint_as_float(B));
        for (int n = 0; n < 27 && keep; ++n) {
            if (n == 13) continue;
            const int oz = n / 9 - 1, oy = (n / 3) % 3 - 1, ox = n % 3 - 1;
            const uint32_t A = halo[((lz + 1 + oz) * HS + ly + 1 + oy) * HS + lx + 1 + ox];
            if (A <= B) continue;           // keys order like the values
            if (FLT) {
                const float af = __uint_as_float(A);
                if (af < __builtin_inff() && sqrt((double)af) >= (sb + olen[n]) * (1.0 + 1e-5)) keep = false;
            } else {
                const long long o = oz * oz + oy * oy + ox * ox;
                const long long d = (long long)A - (long long)B - o;
                if (d >= 0 && d * d >= 4ll * (long long)B * o) keep = false;
            }
        }
    }
    const uint32_t k = keep ? B : 0u;
    if (inside) cand[item + ((int64_t)z * H + y) * W + x] = k;
    const uint32_t wm = wave_max_u32(k);
    if ((t & 63) == 0) red[t >> 6] = wm;
    __syncthreads();
    if (t == 0) {
        uint32_t m = 0;
        for (int i = 0; i < TB / 64; ++i) m = max(m, red[i]);
        cmax[(int64_t)(a.n0 + il) * gridDim.x + cell] = m;
    }
}

// ------------------------------------------------------------------------------------------------ 2. item maxima
__global__ void __launch_bounds__(1024) thick_item_max_kernel(const uint32_t* __restrict__ cmax, int ncells, int n0,
                                                               uint32_t* __restrict__ imax) {
    __shared__ uint32_t red[1024 / 64];
    const int n = n0 + blockIdx.x;
    const uint32_t* c = cmax + (int64_t)n * ncells;
    uint32_t m = 0;
    for (int i = threadIdx.x; i < ncells; i += 1024) m = max(m, c[i]);
    m = wave_max_u32(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 1024 / 64; ++i) m = max(m, red[i]);
        imax[n] = m;
    }
}

// ------------------------------------------------------------------------------------------------ 3. search
template <bool FLT>
__global__ void __launch_bounds__(TB) thick_search_kernel(TArgs a, const uint32_t* __restrict__ d2, const uint32_t* __restrict__ cand,
                                                          const uint32_t* __restrict__ cmax, const uint32_t* __restrict__ imax,
                                                          float* __restrict__ out) {
    __shared__ int4 buf[CAP];               // staged candidates: (z, y, x, key)
    __shared__ int clist[TB];               // the cells of one window pass that need reading, and their maxima
    __shared__ uint32_t clmax[TB];
    __shared__ int scan_lds[TB / 64];
    __shared__ uint32_t red[TB / 64];
    const int t = threadIdx.x, il = blockIdx.y;
    const int D = a.D, H = a.H, W = a.W;
    const int ncz = a.ncz, ncy = a.ncy, ncx = a.ncx;
    const int tile = blockIdx.x;
    const int cx = tile % ncx, cy = (tile / ncx) % ncy, cz = tile / (ncx * ncy);
    const int64_t V = (int64_t)D * H * W;
    const int64_t item = (int64_t)(a.n0 + il) * V;
    const uint32_t* cd = cand + item;
    const uint32_t* cm = cmax + (int64_t)(a.n0 + il) * ((int64_t)ncz * ncy * ncx);
    float sz = 1.f, sy = 1.f, sx = 1.f;
    if (FLT) { sz = a.sp[il][0]; sy = a.sp[il][1]; sx = a.sp[il][2]; }
    const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
    const int z = cz * CS + lz, y = cy * CS + ly, x = cx * CS + lx;
    const bool inside = z < D && y < H && x < W;
    const int64_t v = ((int64_t)z * H + y) * W + x;
    const uint32_t own = inside ? d2[item + v] : 0u;
    uint32_t cur = own;                     // a voxel covers itself
    uint32_t tilemin = block_min_u32(own ? own : NOFG, red);
    if (tilemin == NOFG) {                  // block-uniform: a tile of background
        if (inside) out[item + v] = 0.f;
        return;
    }
    int nbuf = 0;
    // every thread of the block calls; all arguments of the control flow are block-uniform
    auto process = [&]() {
        __syncthreads();
        if (own) {
#pragma unroll 4
            for (int e = 0; e < nbuf; ++e) {
                const int4 c = buf[e];
                const uint32_t B = (uint32_t)c.w;
                if (B > cur) {
                    bool in;
                    if (FLT) in = dd_f32(z - c.x, y - c.y, x - c.z, sz, sy, sx) < __uint_as_float(B);
                    else {
                        const int kz = z - c.x, ky = y - c.y, kx = x - c.z;
                        in = (uint32_t)(kz * kz + ky * ky + kx * kx) < B;
                    }
                    if (in) cur = B;
                }
            }
        }
        tilemin = block_min_u32(own ? cur : NOFG, red);     // its barriers also free buf
        nbuf = 0;
    };
    uint32_t hi = imax[a.n0 + il];
    while (hi > tilemin) {
        const uint32_t lo = FLT ? __float_as_uint(__uint_as_float(hi) * 0.25f) : (hi >> 2);
        // cells a ball of radius sqrt(hi) around a voxel of the tile can come from
        const float r = sqrtf(key_value<FLT>(hi));
        const int wz = ((int)fminf(r / sz, 2048.f) + 1 + CS - 1) / CS, wy = ((int)fminf(r / sy, 2048.f) + 1 + CS - 1) / CS,
                  wx = ((int)fminf(r / sx, 2048.f) + 1 + CS - 1) / CS;
        const int z0 = max(cz - wz, 0), y0 = max(cy - wy, 0), x0 = max(cx - wx, 0);
        const int nwz = min(cz + wz, ncz - 1) - z0 + 1, nwy = min(cy + wy, ncy - 1) - y0 + 1, nwx = min(cx + wx, ncx - 1) - x0 + 1;
        const int nwin = nwz * nwy * nwx;
        for (int base = 0; base < nwin; base += TB) {
            const int i = base + t;
            int pass = 0, cidx = 0;
            uint32_t c = 0;
            if (i < nwin) {
                const int qz = z0 + i / (nwx * nwy), qy = y0 + (i / nwx) % nwy, qx = x0 + i % nwx;
                cidx = (qz * ncy + qy) * ncx + qx;
                c = cm[cidx];
                if (c > lo && c <= hi && c > tilemin) {
                    // gap between the two boxes in voxels: 0 for the same or a touching index, else (n - 1) 8 + 1
                    const int gz = max(abs(qz - cz) - 1, 0) * CS + (qz != cz), gy = max(abs(qy - cy) - 1, 0) * CS + (qy != cy),
                              gx = max(abs(qx - cx) - 1, 0) * CS + (qx != cx);
                    if (FLT) pass = dd_f32(gz, gy, gx, sz, sy, sx) * (1.f - 1e-5f) < __uint_as_float(c);
                    else pass = (uint32_t)(gz * gz + gy * gy + gx * gx) < c;
                }
            }
            int total;
            const int off = block_exclusive_scan<int>(pass, scan_lds, total);
            if (pass) { clist[off] = cidx; clmax[off] = c; }
            __syncthreads();
            for (int j = 0; j < total; ++j) {
                if (clmax[j] <= tilemin) continue;          // the tile has risen past this cell meanwhile
                const int cc = clist[j];
                const int qz = cc / (ncx * ncy), qy = (cc / ncx) % ncy, qx = cc % ncx;
                const int pz = qz * CS + lz, py = qy * CS + ly, px = qx * CS + lx;
                uint32_t k = 0;
                if (pz < D && py < H && px < W) k = cd[((int64_t)pz * H + py) * W + px];
                const int keep = k > tilemin;               // a candidate at or below it raises no voxel of the tile
                int added;
                const int o2 = block_exclusive_scan<int>(keep, scan_lds, added);
                if (keep) buf[nbuf + o2] = make_int4(pz, py, px, (int)k);
                nbuf += added;
                if (nbuf > CAP - TB) process();
            }
        }
        if (nbuf) process();
        hi = lo;
    }
    if (inside) out[item + v] = own ? key_thickness<FLT>(cur) : 0.f;
}

// ------------------------------------------------------------------------------------------------ summary
struct Stat {
    double cnt, mn, mx, sum, below;
};
__device__ __forceinline__ Stat stat_merge(const Stat& p, const Stat& q) {
    return {p.cnt + q.cnt, fmin(p.mn, q.mn), fmax(p.mx, q.mx), p.sum + q.sum, p.below + q.below};
}
// fixed order: butterfly inside the wave, then the waves in index order; valid in thread 0
__device__ __forceinline__ Stat stat_block(Stat s, Stat* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const Stat q = {__shfl_xor(s.cnt, o), __shfl_xor(s.mn, o), __shfl_xor(s.mx, o), __shfl_xor(s.sum, o), __shfl_xor(s.below, o)};
        s = stat_merge(s, q);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < SB / 64; ++i) s = stat_merge(s, red[i]);
    return s;
}

// partial[n][b]: block b's grid-stride share of item n, each thread's voxels in index order
__global__ void __launch_bounds__(SB) thick_summary_partial_kernel(const float* __restrict__ th, int64_t V, float min_thickness,
                                                                   Stat* __restrict__ partial) {
    __shared__ Stat red[SB / 64];
    const float* p = th + (int64_t)blockIdx.y * V;
    Stat s = {0.0, (double)__builtin_inff(), 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < V; i += (int64_t)gridDim.x * SB) {
        const float tv = p[i];
        if (tv > 0.f) {
            s.cnt += 1.0;
            s.mn = fmin(s.mn, (double)tv);
            s.mx = fmax(s.mx, (double)tv);
            s.sum += (double)tv;
            if (tv < min_thickness) s.below += 1.0;
        }
    }
    s = stat_block(s, red);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void __launch_bounds__(SB) thick_summary_final_kernel(const Stat* __restrict__ partial, int nb, double* __restrict__ out) {
    __shared__ Stat red[SB / 64];
    const Stat* p = partial + (int64_t)blockIdx.x * nb;
    Stat s = {0.0, (double)__builtin_inff(), 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += SB) s = stat_merge(s, p[b]);
    s = stat_block(s, red);
    if (threadIdx.x == 0) {
        double* o = out + (int64_t)blockIdx.x * 5;
        o[0] = s.cnt;
        o[1] = s.mn;
        o[2] = s.mx;
        o[3] = s.cnt > 0.0 ? s.sum / s.cnt : __builtin_nan("");
        o[4] = s.below;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct Layout {
    size_t cand, cmax, imax, total;
    int ncz, ncy, ncx;
};

Layout layout(int N, int D, int H, int W) {
    Layout l;
    l.ncz = ceil_div(D, CS); l.ncy = ceil_div(H, CS); l.ncx = ceil_div(W, CS);
    const size_t NV = (size_t)N * D * H * W, NC = (size_t)N * l.ncz * l.ncy * l.ncx;
    l.cand = 0;
    l.cmax = align256(NV * 4);
    l.imax = l.cmax + align256(NC * 4);
    l.total = l.imax + align256((size_t)N * 4);
    return l;
}

bool shape_ok(int N, int D, int H, int W) { return geometry_ok(N, D, H, W) && sides_ok(D, H, W); }

int summary_blocks(int64_t V) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div64(V, (int64_t)SB * 8), 1), SPB_MAX); }

template <bool FLT>
int run_chunk(const TArgs& a, int np, const uint32_t* d2, float* out, uint8_t* ws, const Layout& lay, hipStream_t st) {
    uint32_t* cand = (uint32_t*)(ws + lay.cand);
    uint32_t* cmax = (uint32_t*)(ws + lay.cmax);
    uint32_t* imax = (uint32_t*)(ws + lay.imax);
    const int ncells = a.ncz * a.ncy * a.ncx;
    thick_prune_kernel<FLT><<<dim3((unsigned)ncells, (unsigned)np), TB, 0, st>>>(a, d2, cand, cmax);
    CTU_CHECK_LAUNCH("local_thickness prune");
    thick_item_max_kernel<<<(unsigned)np, 1024, 0, st>>>(cmax, ncells, a.n0, imax);
    CTU_CHECK_LAUNCH("local_thickness item max");
    thick_search_kernel<FLT><<<dim3((unsigned)ncells, (unsigned)np), TB, 0, st>>>(a, d2, cand, cmax, imax, out);
    CTU_CHECK_LAUNCH("local_thickness search");
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_thickness_ws_bytes(int N, int D, int H, int W, int is_float) {
    if (!shape_ok(N, D, H, W) || (is_float != 0 && is_float != 1)) return 0;
    return layout(N, D, H, W).total;
}

extern "C" int ctu_local_thickness(const void* d2, int is_float, int N, int D, int H, int W, const float* spacing, void* out,
                                   void* ws, void* stream) {
    CTU_REQUIRE(d2 && out && ws, "local_thickness: null pointer");
    CTU_REQUIRE(is_float == 0 || is_float == 1, "local_thickness: is_float must be 0 (int32 map) or 1 (float32 map), got %d",
                is_float);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "local_thickness: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)", N, D, H,
                W);
    CTU_REQUIRE(sides_ok(D, H, W), "local_thickness: volume side above %d (shape %d %d %d)", MAX_SIDE, D, H, W);
    bool unit = true;
    if (spacing) {
        for (int i = 0; i < 3 * N; ++i) {
            CTU_REQUIRE(spacing[i] > 0.f && spacing[i] < __builtin_inff(), "local_thickness: spacing must be positive and finite");
            unit = unit && spacing[i] == 1.f;
        }
    }
    CTU_REQUIRE(is_float || unit, "local_thickness: an int32 squared map goes with unit spacing only");
    hipStream_t st = (hipStream_t)stream;
    const Layout lay = layout(N, D, H, W);
    TArgs a;
    a.D = D; a.H = H; a.W = W;
    a.ncz = lay.ncz; a.ncy = lay.ncy; a.ncx = lay.ncx;
    const int chunk = is_float ? MAXG : MAXU;
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int np = std::min(chunk, N - n0);
        a.n0 = n0;
        for (int i = 0; i < MAXG; ++i)
            for (int k = 0; k < 3; ++k) a.sp[i][k] = (spacing && is_float) ? spacing[3 * (n0 + std::min(i, np - 1)) + k] : 1.f;
        const int rc = is_float ? run_chunk<true>(a, np, (const uint32_t*)d2, (float*)out, (uint8_t*)ws, lay, st)
                                : run_chunk<false>(a, np, (const uint32_t*)d2, (float*)out, (uint8_t*)ws, lay, st);
        if (rc != CTU_OK) return rc;
    }
    return CTU_OK;
}

extern "C" size_t ctu_thickness_summary_ws_bytes(int N, int64_t V) {
    if (N < 1 || N > 65535 || V < 1) return 0;
    return align256((size_t)N * summary_blocks(V) * sizeof(Stat));
}

extern "C" int ctu_thickness_summary(const float* thickness, int N, int64_t V, float min_thickness, double* out, void* ws,
                                     void* stream) {
    CTU_REQUIRE(thickness && out && ws, "thickness_summary: null pointer");
    CTU_REQUIRE(N >= 1 && N <= 65535 && V >= 1, "thickness_summary: bad shape N=%d V=%lld (N in 1..65535, V >= 1)", N, (long long)V);
    CTU_REQUIRE(min_thickness >= 0.f, "thickness_summary: min_thickness must be >= 0 and not NaN");
    hipStream_t st = (hipStream_t)stream;
    const int nb = summary_blocks(V);
    thick_summary_partial_kernel<<<dim3((unsigned)nb, (unsigned)N), SB, 0, st>>>(thickness, V, min_thickness, (Stat*)ws);
    CTU_CHECK_LAUNCH("thickness_summary partial");
    thick_summary_final_kernel<<<(unsigned)N, SB, 0, st>>>((const Stat*)ws, nb, out);
    CTU_CHECK_LAUNCH("thickness_summary final");
    return CTU_OK;
}
