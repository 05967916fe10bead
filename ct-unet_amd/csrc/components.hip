// Connected components of 3-D label maps, gfx950: labelling (scipy.ndimage.label numbering) and the two clean-ups of
// segmentations, keep-the-k-largest per class and remove-small-objects (definitions: ctunet_amd/postprocess.py).
//
// Foreground: label != 0, or label in the applied list when one is given.  Two neighbours (6 / 18 / 26-neighbourhood,
// nothing across the border) are connected iff both are foreground and carry the same label.  Union-find over
// parent[v] (item-local linear index, -1 = background) with the invariant parent[v] <= v, so a component's root is its
// first voxel in C order.  One launch per phase, no host synchronisation:
//   1. init:    one block per 8x8x32 tile: labels read with vector loads (uint8 or int64, no one-hot copy), union-find
//               inside the tile in LDS (LDS atomics), parent[v] = global index of the tile-local root.  All-background
//               tiles only write -1 and clear their tile flag, and every later tile pass skips them.
//   2. merge:   the tile-border voxels union with each backward neighbour that lies in another tile: find() with
//               agent-scope relaxed loads (other CUs rewrite parent during the launch), link with atomicMin on the larger
//               root.  Parents only decrease and stay inside their component, so a stale read is still an ancestor; every
//               loop ends because the larger index of the pair strictly decreases.
//   3. flatten: parent[v] = root (the kernel boundary published the merged parents) and, for the filters, the voxel
//               count per root: a per-tile LDS hash of the distinct roots, then one global atomic per (tile, root).
//   4. number (labelling): roots counted per 4096-voxel chunk of C order, the chunk counts scanned in a fixed order per
//               item (-> num[n]), roots ranked within their chunk: component number = 1 + rank of its root in C order.
//   5. select (keep-largest): k rounds of a 64-bit max per (item, class slot) over the roots' keys
//               size << 32 | (INT32_MAX - root) below the previous round's maximum (ties go to the earlier component).
//   6. apply:   foreground voxels of dropped components become 0, every other voxel keeps its label.
// Everything is integer and every order is fixed: two calls are bit-equal.  Workspace: 8 bytes per voxel (parent, size)
// plus per-tile / per-chunk tables.
//
// Fill holes (ctu_fill_holes): phases 1-3 on the complement mask (one byte per voxel, written first), the size array as a
// per-root flag (init zeroes it at every root): the background voxels of the six faces set their root's flag, the apply pass
// writes in OR (background AND root not flagged).
//
// Replaces: nothing in the reference; users would copy the label map to the host for scipy.ndimage.label.
#include "common.h"
#include "scan.h"
#include "voxel_rows.h"

namespace {

constexpr int TZ = 8, TY = 8, TX = 32, TV = TZ * TY * TX;   // tile of 2048 voxels
constexpr int TB = 256;                                     // tile block: 8 x-consecutive voxels per thread
constexpr int VPT = 8;
constexpr int CH = 4096;                                    // numbering chunk: 16 C-order voxels per thread
constexpr int CB = 256;
constexpr int SB = 1024;                                    // scan block
constexpr int MAXAL = 16;                                   // applied labels
constexpr int NSLOT = 256;                                  // class slots of the largest-k selection
constexpr int MAXK = 8;
constexpr int HS = 4096;                                    // LDS hash slots of the size pass (>= 2 x tile voxels)
constexpr int MODE_LARGEST = 0, MODE_MIN_SIZE = 1;

struct CcArgs {
    const void* in;
    int64_t V;                                              // voxels per item (< 2^31)
    int D, H, W;
    int ntx, nty, ntiles;                                   // tiles per item
    int conn, nal;
    long long al[MAXAL];
};

using ctu_vox::i64x2;

__device__ __forceinline__ long long fg_code(long long v, const CcArgs& a) {
    if (v == 0) return 0;
    if (a.nal == 0) return v;
    bool in = false;
#pragma unroll
    for (int i = 0; i < MAXAL; ++i) in |= (i < a.nal) && a.al[i] == v;
    return in ? v : 0;
}

// class slot of a foreground label for the largest-k selection: index in the applied list, or the label itself
// when it lies in 1..255 (-1: no slot, the component is never dropped)
__device__ __forceinline__ int slot_of(long long v, const CcArgs& a) {
    if (a.nal) {
        int s = -1;
#pragma unroll
        for (int i = MAXAL - 1; i >= 0; --i)
            if (i < a.nal && a.al[i] == v) s = i;
        return s;
    }
    return (v >= 1 && v < NSLOT) ? (int)v : -1;
}

// nv (<= 8) x-consecutive values at p (the rest 0)
__device__ __forceinline__ void load8(const uint8_t* p, int nv, long long v[VPT]) {
    if (nv == VPT && ((uintptr_t)p & 7) == 0) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = (w.x >> (8 * u)) & 0xff;
            v[4 + u] = (w.y >> (8 * u)) & 0xff;
        }
    } else {
#pragma unroll
        for (int u = 0; u < VPT; ++u) v[u] = u < nv ? p[u] : 0;
    }
}
__device__ __forceinline__ void load8(const long long* p, int nv, long long v[VPT]) {
    if (nv == VPT && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i64x2 w = reinterpret_cast<const i64x2*>(p)[j];
            v[2 * j] = w.x;
            v[2 * j + 1] = w.y;
        }
    } else {
#pragma unroll
        for (int u = 0; u < VPT; ++u) v[u] = u < nv ? p[u] : 0;
    }
}
__device__ __forceinline__ void store8(int* p, int nv, const int v[VPT]) {
    if (nv == VPT && ((uintptr_t)p & 15) == 0) {
        reinterpret_cast<int4*>(p)[0] = make_int4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<int4*>(p)[1] = make_int4(v[4], v[5], v[6], v[7]);
    } else {
        for (int u = 0; u < nv; ++u) p[u] = v[u];
    }
}
__device__ __forceinline__ void store8(uint8_t* p, int nv, const long long v[VPT]) {
    if (nv == VPT && ((uintptr_t)p & 7) == 0) {
        uint2 w = make_uint2(0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            w.x |= ((uint32_t)v[u] & 0xffu) << (8 * u);
            w.y |= ((uint32_t)v[4 + u] & 0xffu) << (8 * u);
        }
        *reinterpret_cast<uint2*>(p) = w;
    } else {
        for (int u = 0; u < nv; ++u) p[u] = (uint8_t)v[u];
    }
}
__device__ __forceinline__ void store8(long long* p, int nv, const long long v[VPT]) {
    if (nv == VPT && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) reinterpret_cast<i64x2*>(p)[j] = i64x2{v[2 * j], v[2 * j + 1]};
    } else {
        for (int u = 0; u < nv; ++u) p[u] = v[u];
    }
}

// backward neighbour offsets (before the voxel in C order); the first 3 / 9 / 13 ... are filtered by rank below
__device__ __forceinline__ void backward_offset(int i, int& dz, int& dy, int& dx) {
    if (i < 9) { dz = -1; dy = i / 3 - 1; dx = i % 3 - 1; }
    else if (i < 12) { dz = 0; dy = -1; dx = i - 10; }
    else { dz = 0; dy = 0; dx = -1; }
}
__device__ __forceinline__ int offset_rank(int dz, int dy, int dx) { return (dz != 0) + (dy != 0) + (dx != 0); }

// this thread's place in its tile: 4 threads per tile row of 32 x voxels
struct TilePos {
    int lz, ly, lx0;            // tile-local
    int z, y, x;                // item-local
    int z0, y0, x0;             // tile origin
    int nv;                     // voxels of this thread inside the volume
    int64_t v;                  // item-local index of the first one
};

__device__ __forceinline__ TilePos tile_pos(const CcArgs& a) {
    TilePos t;
    int b = blockIdx.x;
    const int tx = b % a.ntx;
    b /= a.ntx;
    const int ty = b % a.nty, tz = b / a.nty;
    t.z0 = tz * TZ; t.y0 = ty * TY; t.x0 = tx * TX;
    const int r = threadIdx.x >> 2;
    t.lz = r / TY; t.ly = r % TY; t.lx0 = (threadIdx.x & 3) * VPT;
    t.z = t.z0 + t.lz; t.y = t.y0 + t.ly; t.x = t.x0 + t.lx0;
    t.nv = (t.z < a.D && t.y < a.H && t.x < a.W) ? min(a.W - t.x, VPT) : 0;
    t.v = ((int64_t)t.z * a.H + t.y) * a.W + t.x;
    return t;
}

// ------------------------------------------------------------------------------------------------ union-find
__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ int lfind(int* p, int i) {
    int q = lds_load(p + i);
    while (q != i) { i = q; q = lds_load(p + i); }
    return i;
}

__device__ void lunion(int* p, int a, int b) {
    while (true) {
        a = lfind(p, a);
        b = lfind(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

// agent scope: the merge pass reads parents that blocks on other CUs are linking (L1 is not refreshed by their stores)
__device__ __forceinline__ int g_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int gfind(int* p, int i) {
    int q = g_load(p + i);
    while (q != i) { i = q; q = g_load(p + i); }
    return i;
}

__device__ void gunion(int* p, int a, int b) {
    while (true) {
        a = gfind(p, a);
        b = gfind(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;          // a was linked meanwhile: join its new parent with b (max of the pair strictly decreases)
    }
}

// ------------------------------------------------------------------------------------------------ 1. init
template <class T>
__global__ void __launch_bounds__(TB) cc_init_kernel(CcArgs a, int* __restrict__ parent, int* __restrict__ size,
                                                     int* __restrict__ tflag) {
    __shared__ long long code[TV];
    __shared__ int lp[TV];
    const int n = blockIdx.y;
    const TilePos t = tile_pos(a);
    long long c[VPT];
    load8((const T*)a.in + n * a.V + t.v, t.nv, c);
    int any = 0;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        c[u] = fg_code(c[u], a);
        any |= c[u] != 0;
    }
    int* P = parent + n * a.V;
    if (!__syncthreads_or(any)) {
        const int m1[VPT] = {-1, -1, -1, -1, -1, -1, -1, -1};
        store8(P + t.v, t.nv, m1);
        if (threadIdx.x == 0) tflag[(int64_t)n * a.ntiles + blockIdx.x] = 0;
        return;
    }
    const int li0 = (t.lz * TY + t.ly) * TX + t.lx0;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        code[li0 + u] = c[u];
        lp[li0 + u] = c[u] ? li0 + u : -1;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        if (!c[u]) continue;
        const int lx = t.lx0 + u;
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            int dz, dy, dx;
            backward_offset(i, dz, dy, dx);
            if (offset_rank(dz, dy, dx) > a.conn) continue;
            const int nz = t.lz + dz, ny = t.ly + dy, nx = lx + dx;
            if (nz < 0 || ny < 0 || ny >= TY || nx < 0 || nx >= TX) continue;   // other tile: merge pass
            const int j = (nz * TY + ny) * TX + nx;
            if (code[j] == c[u]) lunion(lp, li0 + u, j);                       // outside the volume: code 0
        }
    }
    __syncthreads();
    int out[VPT];
    const int HW = a.H * a.W;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        out[u] = -1;
        if (!c[u]) continue;
        const int r = lfind(lp, li0 + u);
        const int rz = r / (TY * TX), ry = (r / TX) % TY, rx = r % TX;
        out[u] = (t.z0 + rz) * HW + (t.y0 + ry) * a.W + t.x0 + rx;
        if (size && r == li0 + u) size[n * a.V + t.v + u] = 0;   // every global root is a tile-local root
    }
    store8(P + t.v, t.nv, out);
    if (threadIdx.x == 0) tflag[(int64_t)n * a.ntiles + blockIdx.x] = 1;
}

// ------------------------------------------------------------------------------------------------ 2. merge
template <class T>
__global__ void __launch_bounds__(TB) cc_merge_kernel(CcArgs a, int* __restrict__ parent, const int* __restrict__ tflag) {
    const int n = blockIdx.y;
    if (!tflag[(int64_t)n * a.ntiles + blockIdx.x]) return;
    const TilePos t = tile_pos(a);
    if (!t.nv) return;
    const T* src = (const T*)a.in + n * a.V;
    long long c[VPT];
    load8(src + t.v, t.nv, c);
    int* P = parent + n * a.V;
    const bool zyb = t.lz == 0 || t.ly == 0 || t.ly == TY - 1;
    const int HW = a.H * a.W;
    for (int u = 0; u < t.nv; ++u) {
        const long long cu = fg_code(c[u], a);
        const int lx = t.lx0 + u;
        if (!cu || !(zyb || lx == 0 || lx == TX - 1)) continue;
        const int v = (int)(t.v + u);
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            int dz, dy, dx;
            backward_offset(i, dz, dy, dx);
            if (offset_rank(dz, dy, dx) > a.conn) continue;
            const int nz = t.lz + dz, ny = t.ly + dy, nx = lx + dx;
            if (nz >= 0 && ny >= 0 && ny < TY && nx >= 0 && nx < TX) continue;   // same tile: done in init
            const int gz = t.z + dz, gy = t.y + dy, gx = t.x + u + dx;
            if (gz < 0 || gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
            const int w = v + dz * HW + dy * a.W + dx;
            if (fg_code((long long)src[w], a) == cu) gunion(P, v, w);
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. flatten (+ sizes)
__device__ __forceinline__ void hash_add(int* hk, int* hc, int key, int cnt) {
    int h = (int)(((uint32_t)key * 2654435761u) >> 20) & (HS - 1);
    while (true) {
        const int k = atomicCAS(hk + h, -1, key);
        if (k == -1 || k == key) {
            atomicAdd(hc + h, cnt);
            return;
        }
        h = (h + 1) & (HS - 1);
    }
}

template <bool SIZES>
__global__ void __launch_bounds__(TB) cc_flatten_kernel(CcArgs a, int* __restrict__ parent, int* __restrict__ size,
                                                        const int* __restrict__ tflag) {
    __shared__ int hk[SIZES ? HS : 1];
    __shared__ int hc[SIZES ? HS : 1];
    const int n = blockIdx.y;
    if (!tflag[(int64_t)n * a.ntiles + blockIdx.x]) return;    // block-uniform
    if (SIZES) {
        for (int i = threadIdx.x; i < HS; i += TB) { hk[i] = -1; hc[i] = 0; }
        __syncthreads();
    }
    const TilePos t = tile_pos(a);
    int* P = parent + n * a.V;
    int cur = -1, cnt = 0;
    for (int u = 0; u < t.nv; ++u) {
        const int v = (int)(t.v + u);
        const int p = P[v];
        if (p < 0) continue;
        const int r = gfind(P, p);
        if (r != p) P[v] = r;
        if (SIZES) {
            if (r != cur) {
                if (cnt) hash_add(hk, hc, cur, cnt);
                cur = r;
                cnt = 0;
            }
            ++cnt;
        }
    }
    if (SIZES) {
        if (cnt) hash_add(hk, hc, cur, cnt);
        __syncthreads();
        int* S = size + n * a.V;
        for (int i = threadIdx.x; i < HS; i += TB)
            if (hk[i] >= 0) __hip_atomic_fetch_add(S + hk[i], hc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------ 4. number
// block_exclusive_scan: scan.h
// 16 C-order voxels of chunk blockIdx.x: root flags
__device__ __forceinline__ uint32_t root_flags(const int* P, int64_t V, int64_t v0) {
    uint32_t f = 0;
    if (v0 + 16 <= V && ((uintptr_t)(P + v0) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 q = reinterpret_cast<const int4*>(P + v0)[j];
            const int64_t b = v0 + 4 * j;
            f |= (uint32_t)(q.x == b) << (4 * j) | (uint32_t)(q.y == b + 1) << (4 * j + 1) |
                 (uint32_t)(q.z == b + 2) << (4 * j + 2) | (uint32_t)(q.w == b + 3) << (4 * j + 3);
        }
    } else {
        for (int i = 0; i < 16 && v0 + i < V; ++i) f |= (uint32_t)(P[v0 + i] == v0 + i) << i;
    }
    return f;
}

__global__ void __launch_bounds__(CB) cc_count_kernel(const int* __restrict__ parent, int64_t V, int nch, int* __restrict__ ccnt) {
    __shared__ int lds[CB / 64];
    const int n = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * CH + threadIdx.x * 16;
    const int c = __popc(root_flags(parent + n * V, V, v0));
    int total;
    block_exclusive_scan(c, lds, total);
    if (threadIdx.x == 0) ccnt[(int64_t)n * nch + blockIdx.x] = total;
}

// one block per item: exclusive offsets of the chunk counts in chunk order, num[n] = the total
__global__ void __launch_bounds__(SB) cc_scan_kernel(const int* __restrict__ ccnt, int nch, int* __restrict__ coff,
                                                     int* __restrict__ num) {
    __shared__ int lds[SB / 64];
    const int n = blockIdx.x;
    const int per = (nch + SB - 1) / SB;
    const int c0 = min(threadIdx.x * per, nch), c1 = min(c0 + per, nch);
    const int* cc = ccnt + (int64_t)n * nch;
    int s = 0;
    for (int c = c0; c < c1; ++c) s += cc[c];
    int total;
    int off = block_exclusive_scan(s, lds, total);
    int* co = coff + (int64_t)n * nch;
    for (int c = c0; c < c1; ++c) {
        co[c] = off;
        off += cc[c];
    }
    if (threadIdx.x == 0) num[n] = total;
}

// out[root] = 1 + rank of the root in C order
__global__ void __launch_bounds__(CB) cc_rank_kernel(const int* __restrict__ parent, int64_t V, int nch,
                                                     const int* __restrict__ coff, int* __restrict__ out) {
    __shared__ int lds[CB / 64];
    const int n = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * CH + threadIdx.x * 16;
    uint32_t f = root_flags(parent + n * V, V, v0);
    int total;
    int r = 1 + coff[(int64_t)n * nch + blockIdx.x] + block_exclusive_scan(__popc(f), lds, total);
    int* O = out + n * V;
    while (f) {
        const int i = __ffs(f) - 1;
        f &= f - 1;
        O[v0 + i] = r++;
    }
}

// out[v] = out[root(v)], 0 for background (root entries were written by the previous launch and do not change)
__global__ void __launch_bounds__(CB) cc_final_kernel(const int* __restrict__ parent, int64_t V, int* __restrict__ out) {
    const int n = blockIdx.y;
    const int64_t v0 = (int64_t)blockIdx.x * CH + threadIdx.x * 16;
    const int* P = parent + n * V;
    int* O = out + n * V;
    if (v0 + 16 <= V && ((uintptr_t)(P + v0) & 15) == 0 && ((uintptr_t)(O + v0) & 15) == 0) {
        // roots rewrite their own number: every O[p] read is a root's entry, which holds the same value throughout
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 q = reinterpret_cast<const int4*>(P + v0)[j];
            reinterpret_cast<int4*>(O + v0)[j] = make_int4(q.x < 0 ? 0 : O[q.x], q.y < 0 ? 0 : O[q.y],
                                                           q.z < 0 ? 0 : O[q.z], q.w < 0 ? 0 : O[q.w]);
        }
        return;
    }
    for (int i = 0; i < 16 && v0 + i < V; ++i) {
        const int p = P[v0 + i];
        if (p != v0 + i) O[v0 + i] = p < 0 ? 0 : O[p];
    }
}

// ------------------------------------------------------------------------------------------------ 5. select
__device__ __forceinline__ unsigned long long comp_key(int size, int root) {
    return (unsigned long long)(uint32_t)size << 32 | (uint32_t)(0x7fffffff - root);
}

template <class T>
__global__ void __launch_bounds__(TB) cc_select_kernel(CcArgs a, const int* __restrict__ parent, const int* __restrict__ size,
                                                       const int* __restrict__ tflag, unsigned long long* __restrict__ sel,
                                                       int round) {
    const int n = blockIdx.y;
    if (!tflag[(int64_t)n * a.ntiles + blockIdx.x]) return;    // block-uniform
    const TilePos t = tile_pos(a);
    const int* P = parent + n * a.V;
    const int* S = size + n * a.V;
    unsigned long long* sl = sel + (int64_t)n * NSLOT * MAXK;
    long long c[VPT];
    load8((const T*)a.in + n * a.V + t.v, t.nv, c);
    unsigned long long best = 0;
    int bs = -1;
    for (int u = 0; u < t.nv; ++u) {
        const int v = (int)(t.v + u);
        if (P[v] != v) continue;                                // roots only
        const int s = slot_of(c[u], a);                         // a root is foreground
        if (s < 0) continue;
        const unsigned long long key = comp_key(S[v], v);
        if (round > 0 && !(key < sl[s * MAXK + round - 1])) continue;
        if (bs < 0 || s == bs) {
            bs = s;
            best = key > best ? key : best;
        } else {
            atomicMax(sl + s * MAXK + round, key);
        }
    }
    // one atomic per (wave, slot)
    while (true) {
        const unsigned long long m = __ballot(bs >= 0);
        if (!m) break;
        const int lead = __ffsll((long long)m) - 1;
        const int s0 = __shfl(bs, lead);
        const bool mine = bs == s0;
        unsigned long long k = mine ? best : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(k, o);
            k = y > k ? y : k;
        }
        if ((int)(threadIdx.x & 63) == lead) atomicMax(sl + s0 * MAXK + round, k);
        if (mine) bs = -1;
    }
}

// ------------------------------------------------------------------------------------------------ 6. apply
template <class T>
__global__ void __launch_bounds__(TB) cc_apply_kernel(CcArgs a, const int* __restrict__ parent, const int* __restrict__ size,
                                                      const int* __restrict__ tflag, const unsigned long long* __restrict__ sel,
                                                      int mode, int param, T* out) {
    const int n = blockIdx.y;
    const bool inplace = (const void*)out == a.in;
    const bool fg_tile = tflag[(int64_t)n * a.ntiles + blockIdx.x] != 0;
    if (!fg_tile && inplace) return;                            // block-uniform
    const TilePos t = tile_pos(a);
    if (!t.nv) return;
    const T* src = (const T*)a.in + n * a.V;
    long long c[VPT];
    load8(src + t.v, t.nv, c);
    bool dropped = false;
    if (fg_tile) {
        const int* P = parent + n * a.V;
        const int* S = size + n * a.V;
        const unsigned long long* sl = sel + (int64_t)n * NSLOT * MAXK;
        for (int u = 0; u < t.nv; ++u) {
            if (!fg_code(c[u], a)) continue;
            const int r = P[t.v + u];
            bool keep;
            if (mode == MODE_MIN_SIZE) {
                keep = S[r] >= param;
            } else {
                const int s = slot_of(c[u], a);
                keep = s < 0 || comp_key(S[r], r) >= sl[s * MAXK + param - 1];
            }
            if (!keep) {
                c[u] = 0;
                dropped = true;
            }
        }
    }
    if (!inplace || dropped) store8(out + n * a.V + t.v, t.nv, c);
}

// ------------------------------------------------------------------------------------------------ host
struct Layout {
    size_t parent, size, tflag, ccnt, coff, sel, total;
    int ntz, nty, ntx, ntiles, nch;
};

Layout layout(int N, int D, int H, int W) {
    Layout l;
    const int64_t V = (int64_t)D * H * W;
    l.ntz = ceil_div(D, TZ); l.nty = ceil_div(H, TY); l.ntx = ceil_div(W, TX);
    l.ntiles = l.ntz * l.nty * l.ntx;
    l.nch = (int)ceil_div64(V, CH);
    size_t o = 0;
    l.parent = o; o = align256(o + (size_t)N * V * 4);
    l.size = o; o = align256(o + (size_t)N * V * 4);
    l.tflag = o; o = align256(o + (size_t)N * l.ntiles * 4);
    l.ccnt = o; o = align256(o + (size_t)N * l.nch * 4);
    l.coff = o; o = align256(o + (size_t)N * l.nch * 4);
    l.sel = o; o = align256(o + (size_t)N * NSLOT * MAXK * 8);
    l.total = o;
    return l;
}

int make_args(CcArgs& a, const void* in, int dtype, int N, int D, int H, int W, int conn, const int64_t* applied,
              int n_applied, void* ws, const char* what) {
    CTU_REQUIRE(in && ws, "%s: null pointer", what);
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64, "%s: unsupported dtype %d (uint8 or int64)", what, dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "%s: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)", what, N,
                D, H, W);
    CTU_REQUIRE(conn >= 1 && conn <= 3, "%s: connectivity must be 1, 2 or 3, got %d", what, conn);
    CTU_REQUIRE(n_applied >= 0 && n_applied <= MAXAL && (n_applied == 0 || applied),
                "%s: 0 to %d applied labels, got %d", what, MAXAL, n_applied);
    for (int i = 0; i < n_applied; ++i) {
        CTU_REQUIRE(applied[i] != 0, "%s: applied labels must be nonzero", what);
        for (int j = 0; j < i; ++j) CTU_REQUIRE(applied[i] != applied[j], "%s: applied labels must be distinct", what);
    }
    const Layout l = layout(N, D, H, W);
    a.in = in;
    a.V = (int64_t)D * H * W;
    a.D = D; a.H = H; a.W = W;
    a.ntx = l.ntx; a.nty = l.nty; a.ntiles = l.ntiles;
    a.conn = conn;
    a.nal = n_applied;
    for (int i = 0; i < MAXAL; ++i) a.al[i] = i < n_applied ? applied[i] : 0;
    return CTU_OK;
}

// phases 1-3
template <class T>
int run_union_find(const CcArgs& a, int N, const Layout& l, uint8_t* w, bool sizes, hipStream_t st) {
    int* parent = (int*)(w + l.parent);
    int* size = (int*)(w + l.size);
    int* tflag = (int*)(w + l.tflag);
    const dim3 grid((unsigned)l.ntiles, (unsigned)N);
    cc_init_kernel<T><<<grid, TB, 0, st>>>(a, parent, sizes ? size : nullptr, tflag);
    CTU_CHECK_LAUNCH("components init");
    cc_merge_kernel<T><<<grid, TB, 0, st>>>(a, parent, tflag);
    CTU_CHECK_LAUNCH("components merge");
    if (sizes) cc_flatten_kernel<true><<<grid, TB, 0, st>>>(a, parent, size, tflag);
    else cc_flatten_kernel<false><<<grid, TB, 0, st>>>(a, parent, size, tflag);
    CTU_CHECK_LAUNCH("components flatten");
    return CTU_OK;
}

template <class T>
int run_filter(const CcArgs& a, int N, const Layout& l, uint8_t* w, int mode, int param, void* out, hipStream_t st) {
    const int rc = run_union_find<T>(a, N, l, w, true, st);
    if (rc != CTU_OK) return rc;
    const int* parent = (const int*)(w + l.parent);
    const int* size = (const int*)(w + l.size);
    const int* tflag = (const int*)(w + l.tflag);
    unsigned long long* sel = (unsigned long long*)(w + l.sel);
    const dim3 grid((unsigned)l.ntiles, (unsigned)N);
    if (mode == MODE_LARGEST) {
        if (hipMemsetAsync(sel, 0, (size_t)N * NSLOT * MAXK * 8, st) != hipSuccess) {
            ctu_set_error("filter_components: memset failed");
            return CTU_ELAUNCH;
        }
        for (int r = 0; r < param; ++r) {
            cc_select_kernel<T><<<grid, TB, 0, st>>>(a, parent, size, tflag, sel, r);
            CTU_CHECK_LAUNCH("components select");
        }
    }
    cc_apply_kernel<T><<<grid, TB, 0, st>>>(a, parent, size, tflag, sel, mode, param, (T*)out);
    CTU_CHECK_LAUNCH("components apply");
    return CTU_OK;
}

// ------------------------------------------------------------------------------------------------ fill holes
constexpr int FB = 256;                                     // 16 C-order voxels per thread

// comp[v] = 1 where the input is background (the union-find then runs on the complement)
template <class T>
__global__ void __launch_bounds__(FB) fh_complement_kernel(const T* __restrict__ in, int64_t V, int has_label, long long label,
                                                           uint8_t* __restrict__ comp) {
    const int n = blockIdx.y;
    const int64_t v0 = ((int64_t)blockIdx.x * FB + threadIdx.x) * 16;
    if (v0 >= V) return;
    const T* src = in + n * V + v0;
    uint8_t* dst = comp + n * V + v0;
    const int nv = (int)(V - v0 < 16 ? V - v0 : 16);
    long long c[16];
    load8(src, nv < VPT ? nv : VPT, c);
    load8(src + VPT, nv > VPT ? nv - VPT : 0, c + VPT);
    const ctu_vox::Foreground fg{has_label, label};
#pragma unroll
    for (int u = 0; u < 16; ++u) c[u] = fg(c[u]) ? 0 : 1;
    store8(dst, nv < VPT ? nv : VPT, c);
    store8(dst + VPT, nv > VPT ? nv - VPT : 0, c + VPT);
}

// flag[root] = 1 for every background voxel on one of the six faces (flag: the size array, 0 at every root after init)
__global__ void __launch_bounds__(FB) fh_faces_kernel(const int* __restrict__ parent, int* __restrict__ flag, int64_t V, int D,
                                                      int H, int W) {
    const int n = blockIdx.y;
    const int64_t fz = (int64_t)H * W, fy = (int64_t)D * W, fx = (int64_t)D * H;
    int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (i >= 2 * (fz + fy + fx)) return;
    int z, y, x;
    if (i < 2 * fz) {
        z = i < fz ? 0 : D - 1;
        i %= fz;
        y = (int)(i / W); x = (int)(i % W);
    } else if (i < 2 * (fz + fy)) {
        i -= 2 * fz;
        y = i < fy ? 0 : H - 1;
        i %= fy;
        z = (int)(i / W); x = (int)(i % W);
    } else {
        i -= 2 * (fz + fy);
        x = i < fx ? 0 : W - 1;
        i %= fx;
        z = (int)(i / H); y = (int)(i % H);
    }
    const int p = parent[n * V + ((int64_t)z * H + y) * W + x];
    if (p >= 0) flag[n * V + p] = 1;
}

// out = in OR (background whose component touches no face)
__global__ void __launch_bounds__(FB) fh_apply_kernel(const uint8_t* __restrict__ comp, const int* __restrict__ parent,
                                                      const int* __restrict__ flag, int64_t V, uint8_t* __restrict__ out) {
    const int n = blockIdx.y;
    const int64_t v0 = ((int64_t)blockIdx.x * FB + threadIdx.x) * 16;
    if (v0 >= V) return;
    const int nv = (int)(V - v0 < 16 ? V - v0 : 16);
    const int* P = parent + n * V;
    const int* F = flag + n * V;
    long long c[16];
    load8(comp + n * V + v0, nv < VPT ? nv : VPT, c);
    load8(comp + n * V + v0 + VPT, nv > VPT ? nv - VPT : 0, c + VPT);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        long long o = 1;
        if (u < nv && c[u]) o = F[P[v0 + u]] ? 0 : 1;
        c[u] = o;
    }
    uint8_t* dst = out + n * V + v0;
    store8(dst, nv < VPT ? nv : VPT, c);
    store8(dst + VPT, nv > VPT ? nv - VPT : 0, c + VPT);
}

template <class T>
int run_fill_holes(const void* in, int N, int D, int H, int W, int conn, int has_label, long long label, uint8_t* out,
                   uint8_t* w, hipStream_t st) {
    const Layout l = layout(N, D, H, W);
    const int64_t V = (int64_t)D * H * W;
    uint8_t* comp = w + align256(l.total);
    CcArgs a;
    const int rc = make_args(a, comp, CTU_U8, N, D, H, W, conn, nullptr, 0, w, "fill_holes");
    if (rc != CTU_OK) return rc;
    const dim3 flat((unsigned)ceil_div64(V, FB * 16), (unsigned)N);
    fh_complement_kernel<T><<<flat, FB, 0, st>>>((const T*)in, V, has_label, label, comp);
    CTU_CHECK_LAUNCH("fill_holes complement");
    int* parent = (int*)(w + l.parent);
    int* flag = (int*)(w + l.size);
    int* tflag = (int*)(w + l.tflag);
    const dim3 grid((unsigned)l.ntiles, (unsigned)N);
    cc_init_kernel<uint8_t><<<grid, TB, 0, st>>>(a, parent, flag, tflag);      // flag[root] = 0
    CTU_CHECK_LAUNCH("fill_holes init");
    cc_merge_kernel<uint8_t><<<grid, TB, 0, st>>>(a, parent, tflag);
    CTU_CHECK_LAUNCH("fill_holes merge");
    cc_flatten_kernel<false><<<grid, TB, 0, st>>>(a, parent, flag, tflag);
    CTU_CHECK_LAUNCH("fill_holes flatten");
    const int64_t faces = 2 * ((int64_t)H * W + (int64_t)D * W + (int64_t)D * H);
    fh_faces_kernel<<<dim3((unsigned)ceil_div64(faces, FB), (unsigned)N), FB, 0, st>>>(parent, flag, V, D, H, W);
    CTU_CHECK_LAUNCH("fill_holes faces");
    fh_apply_kernel<<<flat, FB, 0, st>>>(comp, parent, flag, V, out);
    CTU_CHECK_LAUNCH("fill_holes apply");
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_components_ws_bytes(int N, int D, int H, int W) {
    if (!geometry_ok(N, D, H, W)) return 0;
    return layout(N, D, H, W).total;
}

extern "C" int ctu_label_components(const void* in, int dtype, int N, int D, int H, int W, int connectivity,
                                    const int64_t* applied, int n_applied, int32_t* labels, int32_t* num, void* ws,
                                    void* stream) {
    CcArgs a;
    const int rc0 = make_args(a, in, dtype, N, D, H, W, connectivity, applied, n_applied, ws, "label_components");
    if (rc0 != CTU_OK) return rc0;
    CTU_REQUIRE(num, "label_components: null num");
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(N, D, H, W);
    uint8_t* w = (uint8_t*)ws;
    const int rc = dtype == CTU_U8 ? run_union_find<uint8_t>(a, N, l, w, false, st)
                                   : run_union_find<long long>(a, N, l, w, false, st);
    if (rc != CTU_OK) return rc;
    const int* parent = (const int*)(w + l.parent);
    int* ccnt = (int*)(w + l.ccnt);
    int* coff = (int*)(w + l.coff);
    const dim3 grid((unsigned)l.nch, (unsigned)N);
    cc_count_kernel<<<grid, CB, 0, st>>>(parent, a.V, l.nch, ccnt);
    CTU_CHECK_LAUNCH("components count");
    cc_scan_kernel<<<N, SB, 0, st>>>(ccnt, l.nch, coff, num);
    CTU_CHECK_LAUNCH("components scan");
    if (labels) {
        cc_rank_kernel<<<grid, CB, 0, st>>>(parent, a.V, l.nch, coff, labels);
        CTU_CHECK_LAUNCH("components rank");
        cc_final_kernel<<<grid, CB, 0, st>>>(parent, a.V, labels);
        CTU_CHECK_LAUNCH("components final");
    }
    return CTU_OK;
}

extern "C" int ctu_filter_components(const void* in, int dtype, int N, int D, int H, int W, int connectivity,
                                     const int64_t* applied, int n_applied, int mode, int param, void* out, void* ws,
                                     void* stream) {
    CcArgs a;
    const int rc0 = make_args(a, in, dtype, N, D, H, W, connectivity, applied, n_applied, ws, "filter_components");
    if (rc0 != CTU_OK) return rc0;
    CTU_REQUIRE(out, "filter_components: null output");
    CTU_REQUIRE(mode == MODE_LARGEST || mode == MODE_MIN_SIZE, "filter_components: unknown mode %d", mode);
    CTU_REQUIRE(mode != MODE_LARGEST || (param >= 1 && param <= MAXK),
                "filter_components: keep-largest count must lie in 1..%d, got %d", MAXK, param);
    CTU_REQUIRE(mode != MODE_MIN_SIZE || param >= 0, "filter_components: min_size must be >= 0, got %d", param);
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(N, D, H, W);
    uint8_t* w = (uint8_t*)ws;
    return dtype == CTU_U8 ? run_filter<uint8_t>(a, N, l, w, mode, param, out, st)
                           : run_filter<long long>(a, N, l, w, mode, param, out, st);
}

extern "C" int ctu_fill_holes(const void* in, int dtype, int N, int D, int H, int W, int connectivity, int has_label,
                              int64_t label, uint8_t* out, void* ws, void* stream) {
    CTU_REQUIRE(in && out && ws, "fill_holes: null pointer");
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64, "fill_holes: unsupported dtype %d (uint8 or int64)", dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "fill_holes: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)", N, D, H,
                W);
    CTU_REQUIRE(connectivity >= 1 && connectivity <= 3, "fill_holes: connectivity must be 1, 2 or 3, got %d", connectivity);
    hipStream_t st = (hipStream_t)stream;
    return dtype == CTU_U8 ? run_fill_holes<uint8_t>(in, N, D, H, W, connectivity, has_label != 0, label, out, (uint8_t*)ws, st)
                           : run_fill_holes<long long>(in, N, D, H, W, connectivity, has_label != 0, label, out, (uint8_t*)ws, st);
}
