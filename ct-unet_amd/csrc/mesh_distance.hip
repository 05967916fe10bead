// Exact distances from points to a surface mesh, gfx950: a uniform grid of face lists and a nearest-triangle query in
// float64 (rule pinned in ctunet_amd/mesh.py; tests/mesh_distance_ref.py restates it in numpy as brute force over all faces).
//
// Face grid, over the bounding box of the vertices of the accepted faces; a face with an index outside [0, V) or a vertex
// that is not finite is refused: counted in the workspace head, listed in no cell and never read through.
//   1. corners  a thread per face: its nine coordinates as one 48-byte record (the query then reads three 16-byte words per
//               face and neither the index nor the vertex array), and per block the box of the accepted corners and the sum of
//               the faces' largest extents (shuffles, then one partial per block: no float atomics).
//   2. frame    one block folds the partials in a fixed order and fixes the grid: lower corner, cell size h (given, or twice
//               the mean largest extent of a face, doubled until the grid has at most max_cells cells) and n_a =
//               floor(extent_a / h) + 1 cells per axis, 1 for an axis without extent.  A given h that needs more than
//               max_cells cells sets the head's overflow word; the grid is then one cell and the host refuses it.
//   3. count    a thread per face: cnt[cell] += 1 for every cell its bounding box overlaps (integer atomics: the final value
//               does not depend on arrival order).  A face far larger than the cells is walked by its one lane, here and in
//               the fill; with the default cell size (a multiple of the faces' own extent) such faces are the exception.
//   4. scan     exclusive scan of cnt over the cells (block_exclusive_scan of scan.h: chunk sums, one block over the chunk
//               sums, the chunks again with their bases) -> the cursor of every cell, and the pair count in the head.
//   -- the host reads the head here (pairs, refused faces, cells, overflow, n, frame): the build's one synchronisation --
//   5. emit     offsets = the cursors, offsets[cells] = pairs; a thread per face: faces[cursor[cell]++] = f.  The order
//               within a cell depends on arrival; the query's minimum and its lowest-index tie rule do not.
// Query: a lane per point (explicit float32 points, or the centres of a (shape, spacing, origin) grid formed as voxelize forms
// them).  From the point's cell, clamped into the grid, shells of cells of growing Chebyshev radius r.  Every cell outside
// the block of radius r - 1 lies behind one of the block's inner planes, so the smallest distance to those planes bounds
// shell r and everything behind it from below; a cell (and a row of cells) is bounded by the distance to its box.  Border
// cells count as unbounded outward, and MARGIN (2^-45 of the coordinates' magnitude, some 100 ulp) is taken off every gap
// before it is squared, which covers the rounding of both this arithmetic and the cell indices of the faces: rounding can
// only lower a bound.  A cell is skipped and the search stops only where the bound exceeds the best squared distance so far
// (or max_distance^2), strictly, so every face that attains the minimum is evaluated and the result does not depend on the
// cell size.  A face is evaluated from its record alone, with the same arithmetic wherever it is met.
// Lanes of a wave that are done wait for the others: queries in mesh or voxel order are neighbours in space and do much
// the same work.  Contraction is off, as in mesh_voxelize.hip.  Measured: profiles/mesh_distance.md.
//
// No reference counterpart: the reference writes NIfTI volumes only.
#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int FB = 256;                         // block of the per-face and per-query kernels
constexpr int SCB = 1024;                       // scan block
constexpr int SCI = 4;                          // cells of a scan thread
constexpr int SCAN_CHUNK = SCB * SCI;
constexpr int RB = 1024;                        // block of the frame kernel
constexpr int64_t LIMIT = (int64_t)1 << 31;
constexpr int64_t MAX_CELLS = CTU_MESH_GRID_MAX_CELLS;
constexpr double MARGIN = 0x1p-45;
constexpr double SHRINK = 1.0 - 0x1p-50;
constexpr double INF = __builtin_inf();

// at the start of the workspace (256 bytes reserved); the host reads the first 13 words
struct Head {
    long long pairs, refused, cells, overflow, n[3];
    double lo[3], h[3];
    long long accepted;
};
static_assert(sizeof(Head) <= 256, "the head has 256 bytes");

struct Partial { double lo[3], hi[3], ext, count; };

struct Layout { size_t part, cnt, cursor, bsum, total; };
Layout layout(int64_t F, int64_t max_cells) {
    Layout l;
    size_t o = 256;
    l.part = o;   o += align256((size_t)ceil_div64(F, FB) * sizeof(Partial));
    l.cnt = o;    o += align256((size_t)max_cells * 4);
    l.cursor = o; o += align256((size_t)max_cells * 4);
    l.bsum = o;   o += align256((size_t)ceil_div64(max_cells, SCAN_CHUNK) * 8);
    l.total = o;
    return l;
}

bool sizes_ok(int64_t F, int64_t max_cells) { return F >= 0 && F < LIMIT && max_cells >= 1 && max_cells <= MAX_CELLS; }

struct Frame {
    double lo[3], h[3];
    int n[3];
};

// the cell of coordinate x on axis a, clamped into the grid in floating point (x may be 1e30 or, for a corrupted frame, NaN)
__device__ __forceinline__ int cell_of(const Frame& g, int a, double x) {
    double t = floor((x - g.lo[a]) / g.h[a]);
    t = t >= 0.0 ? t : 0.0;
    const double top = (double)(g.n[a] - 1);
    t = t <= top ? t : top;
    return (int)t;
}

__device__ __forceinline__ Frame frame_of(const Head* head) {
    Frame g;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = head->lo[a];
        g.h[a] = head->h[a];
        const long long n = head->n[a];
        g.n[a] = n >= 1 && n <= MAX_CELLS ? (int)n : 1;
    }
    return g;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// the lanes' values added in one fixed tree: two calls are bit-equal
__device__ __forceinline__ double wave_add(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------ corners / frame
__global__ void __launch_bounds__(FB) grid_corners_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                                          int64_t F, float4* __restrict__ corners, Partial* __restrict__ part,
                                                          Head* head) {
    __shared__ Partial lds[FB / 64];
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    double lo[3] = {INF, INF, INF}, hi[3] = {-INF, -INF, -INF}, ext = 0.0, count = 0.0;
    if (t < F) {
        const int i[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
        float p[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool ok = (unsigned)i[0] < (unsigned)V && (unsigned)i[1] < (unsigned)V && (unsigned)i[2] < (unsigned)V;
        if (ok) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = vert[(int64_t)i[q] * 3 + a];
                    p[3 * q + a] = x;
                    ok = ok && x - x == 0.f;
                }
        }
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = (double)fminf(p[a], fminf(p[3 + a], p[6 + a]));
                hi[a] = (double)fmaxf(p[a], fmaxf(p[3 + a], p[6 + a]));
            }
            ext = fmax(hi[0] - lo[0], fmax(hi[1] - lo[1], hi[2] - lo[2]));
            count = 1.0;
            corners[3 * t] = make_float4(p[0], p[1], p[2], p[3]);
            corners[3 * t + 1] = make_float4(p[4], p[5], p[6], p[7]);
            corners[3 * t + 2] = make_float4(p[8], 0.f, 0.f, 0.f);
        } else {
            atomicAdd((unsigned long long*)&head->refused, 1ull);
            const float nan = __builtin_nanf("");                   // a refused face's record: listed nowhere, never read
            corners[3 * t] = corners[3 * t + 1] = corners[3 * t + 2] = make_float4(nan, nan, nan, nan);
        }
    }
    Partial w;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w.lo[a] = wave_min(lo[a]);
        w.hi[a] = wave_max(hi[a]);
    }
    w.ext = wave_add(ext);
    w.count = wave_add(count);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial b = lds[0];
        for (int k = 1; k < FB / 64; ++k) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                b.lo[a] = fmin(b.lo[a], lds[k].lo[a]);
                b.hi[a] = fmax(b.hi[a], lds[k].hi[a]);
            }
            b.ext = b.ext + lds[k].ext;
            b.count = b.count + lds[k].count;
        }
        part[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(RB) grid_frame_kernel(const Partial* __restrict__ part, int64_t nb, double cell_size,
                                                        long long max_cells, Head* head) {
    __shared__ Partial lds[RB / 64];
    Partial p = {{INF, INF, INF}, {-INF, -INF, -INF}, 0.0, 0.0};
    for (int64_t k = threadIdx.x; k < nb; k += RB) {                 // a fixed subset per thread, in ascending order
        const Partial q = part[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = fmin(p.lo[a], q.lo[a]);
            p.hi[a] = fmax(p.hi[a], q.hi[a]);
        }
        p.ext = p.ext + q.ext;
        p.count = p.count + q.count;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p.lo[a] = wave_min(p.lo[a]);
        p.hi[a] = wave_max(p.hi[a]);
    }
    p.ext = wave_add(p.ext);
    p.count = wave_add(p.count);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < RB / 64; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = fmin(p.lo[a], lds[k].lo[a]);
            p.hi[a] = fmax(p.hi[a], lds[k].hi[a]);
        }
        p.ext = p.ext + lds[k].ext;
        p.count = p.count + lds[k].count;
    }
    double ext[3] = {0.0, 0.0, 0.0};
    if (p.count > 0.0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) ext[a] = p.hi[a] - p.lo[a];
    } else {
        p.lo[0] = p.lo[1] = p.lo[2] = 0.0;                           // no accepted face: one cell, nothing listed
    }
    double h = cell_size > 0.0 ? cell_size : 2.0 * (p.ext / fmax(p.count, 1.0));
    if (!(h > 0.0 && h < INF)) h = 1.0;                              // every face a point: any size gives one cell
    const double top = (double)MAX_CELLS;
    double n[3];
    long long overflow = 0;
    for (;;) {
        double cells = 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q = ext[a] > 0.0 ? floor(ext[a] / h) + 1.0 : 1.0;   // an axis without extent: one cell, no division
            n[a] = q <= top + 1.0 ? q : top + 1.0;                           // clamped before it becomes an integer
            cells *= n[a];
        }
        if (cells <= (double)max_cells) break;
        if (cell_size > 0.0) {                                       // the caller's size does not fit: the host refuses it
            overflow = 1;
            n[0] = n[1] = n[2] = 1.0;
            break;
        }
        h = h * 2.0;
    }
    head->overflow = overflow;
    head->accepted = (long long)p.count;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        head->n[a] = (long long)n[a];
        head->lo[a] = p.lo[a];
        head->h[a] = h;
    }
    head->cells = (long long)n[0] * (long long)n[1] * (long long)n[2];
}

// ------------------------------------------------------------------------------------------------ count / fill
__global__ void __launch_bounds__(FB) grid_clear_kernel(const Head* head, int* __restrict__ cnt, int64_t max_cells) {
    const int64_t cells = head->cells < max_cells ? head->cells : max_cells;
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i < cells; i += (int64_t)gridDim.x * FB) cnt[i] = 0;
}

// FILL: offsets hold the cells' first positions, cursor the next free ones
template <bool FILL>
__global__ void __launch_bounds__(FB) grid_pairs_kernel(const float4* __restrict__ corners, int64_t F, const Head* head,
                                                        int64_t max_cells, int* __restrict__ cnt_or_cursor, int64_t pairs,
                                                        int* __restrict__ items) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    const float4 c0 = corners[3 * t], c1 = corners[3 * t + 1], c2 = corners[3 * t + 2];
    if (!(c0.x - c0.x == 0.f)) return;                               // a refused face
    const Frame g = frame_of(head);
    if ((int64_t)g.n[0] * g.n[1] * g.n[2] > max_cells) return;
    const float p[9] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x};
    int k0[3], k1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        k0[a] = cell_of(g, a, (double)fminf(p[a], fminf(p[3 + a], p[6 + a])));
        k1[a] = cell_of(g, a, (double)fmaxf(p[a], fmaxf(p[3 + a], p[6 + a])));
    }
    for (int z = k0[0]; z <= k1[0]; ++z)
        for (int y = k0[1]; y <= k1[1]; ++y)
            for (int x = k0[2]; x <= k1[2]; ++x) {
                const int64_t cell = ((int64_t)z * g.n[1] + y) * g.n[2] + x;
                const int pos = atomicAdd(cnt_or_cursor + cell, 1);
                if (FILL && pos >= 0 && pos < pairs) items[pos] = (int)t;
            }
}

// ------------------------------------------------------------------------------------------------ scan over the cells
__device__ __forceinline__ void load_items(const int* __restrict__ x, int64_t i0, int64_t n, int (&w)[SCI]) {
#pragma unroll
    for (int u = 0; u < SCI; ++u) w[u] = i0 + u < n ? x[i0 + u] : 0;
}

__global__ void __launch_bounds__(SCB) grid_scan_sums_kernel(const int* __restrict__ x, const Head* head, int64_t max_cells,
                                                             long long* __restrict__ bsum) {
    __shared__ long long lds[SCB / 64];
    const int64_t n = head->cells < max_cells ? head->cells : max_cells;
    if ((int64_t)blockIdx.x * SCAN_CHUNK >= n) return;               // the whole block leaves
    int w[SCI];
    load_items(x, (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCI, n, w);
    long long total;
    block_exclusive_scan((long long)w[0] + w[1] + w[2] + w[3], lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCB) grid_scan_chunks_kernel(long long* __restrict__ bsum, Head* head, int64_t max_cells) {
    __shared__ long long lds[SCB / 64];
    const int64_t n = head->cells < max_cells ? head->cells : max_cells;
    const int nb = (int)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    const int per = (nb + SCB - 1) / SCB;
    const int r0 = min((int)threadIdx.x * per, nb), r1 = min(r0 + per, nb);
    long long s = 0;
    for (int r = r0; r < r1; ++r) s += bsum[r];
    long long t;
    long long o = block_exclusive_scan(s, lds, t);
    for (int r = r0; r < r1; ++r) {
        const long long b = bsum[r];
        bsum[r] = o;
        o += b;
    }
    if (threadIdx.x == 0) head->pairs = t;
}

__global__ void __launch_bounds__(SCB) grid_scan_apply_kernel(const int* __restrict__ x, const Head* head, int64_t max_cells,
                                                              const long long* __restrict__ bsum, int* __restrict__ y) {
    __shared__ long long lds[SCB / 64];
    const int64_t n = head->cells < max_cells ? head->cells : max_cells;
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCI;
    if ((int64_t)blockIdx.x * SCAN_CHUNK >= n) return;
    int w[SCI];
    load_items(x, i0, n, w);
    long long total;
    long long o = bsum[blockIdx.x] + block_exclusive_scan((long long)w[0] + w[1] + w[2] + w[3], lds, total);
#pragma unroll
    for (int u = 0; u < SCI; ++u) {
        if (i0 + u < n) y[i0 + u] = o < LIMIT ? (int)o : (int)(LIMIT - 1);   // 2^31 pairs or more: the host refuses the grid
        o += w[u];
    }
}

__global__ void __launch_bounds__(FB) grid_offsets_kernel(const int* __restrict__ cursor, int64_t cells, int64_t pairs,
                                                          int* __restrict__ offsets) {
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i <= cells; i += (int64_t)gridDim.x * FB)
        offsets[i] = i < cells ? cursor[i] : (int)pairs;
}

// ------------------------------------------------------------------------------------------------ the rule
struct Tri { double a[3], b[3], c[3]; };

__device__ __forceinline__ Tri load_tri(const float4* __restrict__ corners, int64_t f) {
    const float4 c0 = corners[3 * f], c1 = corners[3 * f + 1], c2 = corners[3 * f + 2];
    Tri t;
    t.a[0] = (double)c0.x; t.a[1] = (double)c0.y; t.a[2] = (double)c0.z;
    t.b[0] = (double)c0.w; t.b[1] = (double)c1.x; t.b[2] = (double)c1.y;
    t.c[0] = (double)c1.z; t.c[1] = (double)c1.w; t.c[2] = (double)c2.x;
    return t;
}

__device__ __forceinline__ double dot3(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ void cross3(const double (&u)[3], const double (&v)[3], double (&w)[3]) {
    w[0] = u[1] * v[2] - u[2] * v[1];
    w[1] = u[2] * v[0] - u[0] * v[2];
    w[2] = u[0] * v[1] - u[1] * v[0];
}

// squared distance from p to the segment a-b; the closest point to `cp` if WANT
template <bool WANT>
__device__ __forceinline__ double segment_d2(const double (&p)[3], const double (&a)[3], const double (&b)[3], double (&cp)[3]) {
    double ab[3], ap[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ap[k] = p[k] - a[k];
    }
    const double len = dot3(ab, ab);
    double t = 0.0;                                                  // a segment of zero length is its endpoint
    if (len > 0.0) {
        t = dot3(ap, ab) / len;
        t = t >= 0.0 ? t : 0.0;
        t = t <= 1.0 ? t : 1.0;
    }
    double c[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = a[k] + t * ab[k];
        d[k] = p[k] - c[k];
        if (WANT) cp[k] = c[k];
    }
    return dot3(d, d);
}

// squared distance from p to a face: the nearest of its three edge segments (the first wins a tie) and, where the normal
// is not zero and the three edge functions are >= 0, the plane term if it is smaller
template <bool WANT>
__device__ __forceinline__ double face_d2(const double (&p)[3], const Tri& t, double (&cp)[3]) {
    double c1[3], c2[3];
    double best = segment_d2<WANT>(p, t.a, t.b, cp);
    const double d1 = segment_d2<WANT>(p, t.b, t.c, c1);
    const double d2 = segment_d2<WANT>(p, t.c, t.a, c2);
    if (d1 < best) {
        best = d1;
        if (WANT) { cp[0] = c1[0]; cp[1] = c1[1]; cp[2] = c1[2]; }
    }
    if (d2 < best) {
        best = d2;
        if (WANT) { cp[0] = c2[0]; cp[1] = c2[1]; cp[2] = c2[2]; }
    }
    double ab[3], bc[3], ca[3], ac[3], pa[3], pb[3], pc[3], n[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = t.b[k] - t.a[k];
        bc[k] = t.c[k] - t.b[k];
        ca[k] = t.a[k] - t.c[k];
        ac[k] = t.c[k] - t.a[k];
        pa[k] = p[k] - t.a[k];
        pb[k] = p[k] - t.b[k];
        pc[k] = p[k] - t.c[k];
    }
    cross3(ab, ac, n);
    const double nn = dot3(n, n);
    if (nn > 0.0) {
        cross3(ab, pa, w);
        const double e0 = dot3(w, n);
        cross3(bc, pb, w);
        const double e1 = dot3(w, n);
        cross3(ca, pc, w);
        const double e2 = dot3(w, n);
        if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
            const double s = dot3(pa, n);
            const double dp = (s * s) / nn;
            if (dp < best) {
                best = dp;
                if (WANT) {
                    const double u = s / nn;
#pragma unroll
                    for (int k = 0; k < 3; ++k) cp[k] = p[k] - u * n[k];
                }
            }
        }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------ query
struct Axes {
    double o[3], s[3];                          // origin and spacing of the query grid in (z, y, x), widened
    int n[3];                                   // D, H, W
};

// the gap between p and the plane x_a = lo_a + k h_a, lowered by MARGIN of the magnitudes involved; `above`: the plane
// lies above p's side (gap = plane - p), else below (gap = p - plane).  Never negative.
__device__ __forceinline__ double gap(const Frame& g, int a, int k, double p, bool above) {
    const double plane = g.lo[a] + (double)k * g.h[a];
    const double raw = above ? plane - p : p - plane;
    const double m = MARGIN * (fabs(p) + fabs(g.lo[a]) + fabs((double)g.n[a] * g.h[a]));
    const double v = raw - m;
    return v > 0.0 ? v : 0.0;
}

// lower bound of the distance from p to cell k of axis a along that axis; border cells are unbounded outward
__device__ __forceinline__ double axis_bound(const Frame& g, int a, int k, double p) {
    const double below = k > 0 ? gap(g, a, k, p, true) : 0.0;               // p under the cell's lower plane
    const double over = k < g.n[a] - 1 ? gap(g, a, k + 1, p, false) : 0.0;  // p over its upper plane
    return below > over ? below : over;
}

__global__ void __launch_bounds__(FB) distance_query_kernel(const float4* __restrict__ corners, int64_t F,
                                                            const int* __restrict__ offsets, const int* __restrict__ items,
                                                            int64_t pairs, const double* __restrict__ frame, int nz, int ny, int nx,
                                                            const float* __restrict__ points, int64_t Q, Axes ax, double max2,
                                                            float far_value, float* __restrict__ dist, int* __restrict__ face,
                                                            float* __restrict__ closest) {
    const int64_t q = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (q >= Q) return;
    double p[3];
    if (points) {
        p[0] = (double)points[3 * q];
        p[1] = (double)points[3 * q + 1];
        p[2] = (double)points[3 * q + 2];
    } else {
        const int64_t hw = (int64_t)ax.n[1] * ax.n[2];
        const int i = (int)(q / hw), j = (int)((q - i * hw) / ax.n[2]), k = (int)(q - i * hw - (int64_t)j * ax.n[2]);
        p[0] = ax.o[0] + (double)i * ax.s[0];
        p[1] = ax.o[1] + (double)j * ax.s[1];
        p[2] = ax.o[2] + (double)k * ax.s[2];
    }
    const float nan = __builtin_nanf("");
    if (!(p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0)) {         // a point that is not finite
        dist[q] = nan;
        if (face) face[q] = -1;
        if (closest) closest[3 * q] = closest[3 * q + 1] = closest[3 * q + 2] = nan;
        return;
    }
    Frame g;
    g.n[0] = nz; g.n[1] = ny; g.n[2] = nx;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = frame[a];
        g.h[a] = frame[3 + a];
    }
    int c[3], rmax = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = cell_of(g, a, p[a]);
        rmax = max(rmax, max(c[a], g.n[a] - 1 - c[a]));
    }
    double best = max2, unused[3];
    unsigned bestf = 0xffffffffu;
    for (int r = 0; r <= rmax; ++r) {
        if (r > 0) {
            // every cell of shell r and beyond lies behind one of the inner planes of the block of radius r - 1
            double lb = INF;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (c[a] + r <= g.n[a] - 1) lb = fmin(lb, gap(g, a, c[a] + r, p[a], true));
                if (c[a] - r >= 0) lb = fmin(lb, gap(g, a, c[a] - r + 1, p[a], false));
            }
            if ((lb * lb) * SHRINK > best) break;
        }
        const int z0 = max(c[0] - r, 0), z1 = min(c[0] + r, g.n[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
        for (int z = z0; z <= z1; ++z) {
            const double bz = axis_bound(g, 0, z, p[0]);
            if ((bz * bz) * SHRINK > best) continue;
            const bool zshell = z == c[0] - r || z == c[0] + r;
            for (int y = y0; y <= y1; ++y) {
                const double by = axis_bound(g, 1, y, p[1]);
                const double bzy = bz * bz + by * by;
                if (bzy * SHRINK > best) continue;
                const bool whole = zshell || y == c[1] - r || y == c[1] + r;     // the row lies on the shell
                const int xa = c[2] - r, xb = c[2] + r;
                // on the shell: every x of the block; inside it: its two ends
                const int step = whole || r == 0 ? 1 : 2 * r;
                for (int x = xa; x <= xb; x += step) {
                    if (x < 0 || x > g.n[2] - 1) continue;
                    const double bx = axis_bound(g, 2, x, p[2]);
                    if ((bzy + bx * bx) * SHRINK > best) continue;
                    const int64_t cell = ((int64_t)z * g.n[1] + y) * g.n[2] + x;
                    const int o0 = offsets[cell], o1 = offsets[cell + 1];
                    if (o0 < 0 || o1 > pairs) continue;                          // a corrupted table: wrong, never a fault
                    for (int o = o0; o < o1; ++o) {
                        const unsigned f = (unsigned)items[o];
                        if (f >= (unsigned long long)F) continue;
                        const Tri t = load_tri(corners, f);
                        const double d2 = face_d2<false>(p, t, unused);
                        if (d2 < best || (d2 == best && f < bestf)) {
                            best = d2;
                            bestf = f;
                        }
                    }
                }
            }
        }
    }
    if (bestf == 0xffffffffu) {                                       // nothing within max_distance (or an empty grid)
        dist[q] = far_value;
        if (face) face[q] = -1;
        if (closest) closest[3 * q] = closest[3 * q + 1] = closest[3 * q + 2] = nan;
        return;
    }
    dist[q] = (float)sqrt(best);
    if (face) face[q] = (int)bestf;
    if (closest) {
        double cp[3];
        const Tri t = load_tri(corners, bestf);
        face_d2<true>(p, t, cp);
        closest[3 * q] = (float)cp[0];
        closest[3 * q + 1] = (float)cp[1];
        closest[3 * q + 2] = (float)cp[2];
    }
}

}  // namespace

extern "C" size_t ctu_mesh_grid_ws_bytes(int64_t F, int64_t max_cells) { return sizes_ok(F, max_cells) ? layout(F, max_cells).total : 0; }

extern "C" int ctu_mesh_grid_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, float cell_size,
                                   int64_t max_cells, float* corners, void* ws, void* stream) {
    CTU_REQUIRE(V >= 0 && V < LIMIT && F >= 1 && F < LIMIT, "mesh_grid_build: V must lie in [0, 2^31) and F in [1, 2^31), got V = %lld, F = %lld",
                (long long)V, (long long)F);
    CTU_REQUIRE(V > 0, "mesh_grid_build: faces without vertices");
    CTU_REQUIRE(max_cells >= 1 && max_cells <= MAX_CELLS, "mesh_grid_build: max_cells must lie in 1..%lld, got %lld",
                (long long)MAX_CELLS, (long long)max_cells);
    CTU_REQUIRE(cell_size == 0.f || (cell_size > 0.f && cell_size < __builtin_inff()),
                "mesh_grid_build: cell_size must be 0 (the default) or positive and finite, got %g", (double)cell_size);
    CTU_REQUIRE(vertices && faces && corners && ws, "mesh_grid_build: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0 && (uintptr_t)corners % 16 == 0, "mesh_grid_build: the workspace and the corners must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(F, max_cells);
    unsigned char* b = (unsigned char*)ws;
    Head* head = (Head*)b;
    Partial* part = (Partial*)(b + l.part);
    int* cnt = (int*)(b + l.cnt);
    int* cursor = (int*)(b + l.cursor);
    long long* bsum = (long long*)(b + l.bsum);
    CTU_REQUIRE(hipMemsetAsync(ws, 0, 256, st) == hipSuccess, "mesh_grid_build: cannot clear the workspace head");
    const int64_t fblocks = ceil_div64(F, FB);
    const unsigned fgrid = (unsigned)fblocks;
    const unsigned cgrid = (unsigned)(ceil_div64(max_cells, FB) < 2048 ? ceil_div64(max_cells, FB) : 2048);
    const unsigned sgrid = (unsigned)ceil_div64(max_cells, SCAN_CHUNK);
    grid_corners_kernel<<<fgrid, FB, 0, st>>>(vertices, (int)V, faces, F, (float4*)corners, part, head);
    CTU_CHECK_LAUNCH("mesh grid corners");
    grid_frame_kernel<<<1, RB, 0, st>>>(part, fblocks, (double)cell_size, (long long)max_cells, head);
    CTU_CHECK_LAUNCH("mesh grid frame");
    grid_clear_kernel<<<cgrid, FB, 0, st>>>(head, cnt, max_cells);
    CTU_CHECK_LAUNCH("mesh grid clear");
    grid_pairs_kernel<false><<<fgrid, FB, 0, st>>>((const float4*)corners, F, head, max_cells, cnt, 0, nullptr);
    CTU_CHECK_LAUNCH("mesh grid count");
    grid_scan_sums_kernel<<<sgrid, SCB, 0, st>>>(cnt, head, max_cells, bsum);
    CTU_CHECK_LAUNCH("mesh grid scan sums");
    grid_scan_chunks_kernel<<<1, SCB, 0, st>>>(bsum, head, max_cells);
    CTU_CHECK_LAUNCH("mesh grid scan chunks");
    grid_scan_apply_kernel<<<sgrid, SCB, 0, st>>>(cnt, head, max_cells, bsum, cursor);
    CTU_CHECK_LAUNCH("mesh grid scan apply");
    return CTU_OK;
}

extern "C" int ctu_mesh_grid_emit(const float* corners, int64_t F, int64_t max_cells, int64_t cells, int64_t pairs,
                                  int32_t* offsets, int32_t* items, void* ws, void* stream) {
    CTU_REQUIRE(F >= 1 && F < LIMIT, "mesh_grid_emit: F must lie in [1, 2^31), got %lld", (long long)F);
    CTU_REQUIRE(max_cells >= 1 && max_cells <= MAX_CELLS && cells >= 1 && cells <= max_cells,
                "mesh_grid_emit: cells = %lld must lie in 1..max_cells = %lld <= %lld", (long long)cells, (long long)max_cells,
                (long long)MAX_CELLS);
    CTU_REQUIRE(pairs >= 0 && pairs < LIMIT, "mesh_grid_emit: pairs = %lld must lie in [0, 2^31); choose a larger cell_size", (long long)pairs);
    CTU_REQUIRE(corners && offsets && ws && (pairs == 0 || items), "mesh_grid_emit: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0 && (uintptr_t)corners % 16 == 0, "mesh_grid_emit: the workspace and the corners must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(F, max_cells);
    unsigned char* b = (unsigned char*)ws;
    int* cursor = (int*)(b + l.cursor);
    const unsigned ogrid = (unsigned)(ceil_div64(cells + 1, FB) < 2048 ? ceil_div64(cells + 1, FB) : 2048);
    grid_offsets_kernel<<<ogrid, FB, 0, st>>>(cursor, cells, pairs, offsets);
    CTU_CHECK_LAUNCH("mesh grid offsets");
    if (pairs == 0) return CTU_OK;
    grid_pairs_kernel<true><<<(unsigned)ceil_div64(F, FB), FB, 0, st>>>((const float4*)corners, F, (const Head*)b, max_cells, cursor, pairs, items);
    CTU_CHECK_LAUNCH("mesh grid fill");
    return CTU_OK;
}

extern "C" int ctu_mesh_distance(const float* corners, int64_t F, const int32_t* offsets, const int32_t* items, int64_t pairs,
                                 const double* frame, int nz, int ny, int nx, const float* points, int64_t Q, int D, int H, int W,
                                 const float* spacing, const float* origin, float max_distance, float far_value, float* dist,
                                 int32_t* face, float* closest, void* stream) {
    CTU_REQUIRE(F >= 1 && F < LIMIT && pairs >= 0 && pairs < LIMIT, "mesh_distance: F must lie in [1, 2^31) and pairs in [0, 2^31), got F = %lld, pairs = %lld",
                (long long)F, (long long)pairs);
    CTU_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1 && (int64_t)nz * ny <= MAX_CELLS && (int64_t)nz * ny * nx <= MAX_CELLS,
                "mesh_distance: the face grid must have 1..%lld cells, got %dx%dx%d", (long long)MAX_CELLS, nz, ny, nx);
    CTU_REQUIRE(max_distance == 0.f || (max_distance > 0.f && max_distance < __builtin_inff()),
                "mesh_distance: max_distance must be 0 (none) or positive and finite, got %g", (double)max_distance);
    Axes ax = {{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, {1, 1, 1}};
    if (points) {
        CTU_REQUIRE(Q >= 0 && Q < LIMIT, "mesh_distance: Q must lie in [0, 2^31), got %lld", (long long)Q);
    } else {
        CTU_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= 1024 && H <= 1024 && W <= 1024 && (int64_t)D * H * W < LIMIT,
                    "mesh_distance: bad shape %dx%dx%d (every side in 1..1024, D*H*W < 2^31); without points the queries are a grid's centres",
                    D, H, W);
        for (int a = 0; a < 3; ++a) {
            const float s = spacing ? spacing[a] : 1.f, o = origin ? origin[a] : 0.f;
            CTU_REQUIRE(s > 0.f && s < __builtin_inff() && o - o == 0.f, "mesh_distance: spacing must be positive and finite, origin finite");
            ax.s[a] = (double)s;
            ax.o[a] = (double)o;
        }
        ax.n[0] = D;
        ax.n[1] = H;
        ax.n[2] = W;
        Q = (int64_t)D * H * W;
    }
    if (Q == 0) return CTU_OK;
    CTU_REQUIRE(corners && offsets && frame && dist && (pairs == 0 || items), "mesh_distance: null pointer");
    CTU_REQUIRE((uintptr_t)corners % 16 == 0, "mesh_distance: the corners must be 16-byte aligned");
    const double max2 = max_distance > 0.f ? (double)max_distance * (double)max_distance : INF;
    distance_query_kernel<<<(unsigned)ceil_div64(Q, FB), FB, 0, (hipStream_t)stream>>>(
        (const float4*)corners, F, offsets, items, pairs, frame, nz, ny, nx, points, Q, ax, max2, far_value, dist, face, closest);
    CTU_CHECK_LAUNCH("mesh distance query");
    return CTU_OK;
}
