// Decimation of surface meshes by vertex clustering on a uniform grid, gfx950 (rule pinned in ctunet_amd/simplify.py;
// tests/simplify_ref.py restates it in numpy).
//
// A face with an index outside [0, V) or a vertex that is not finite is refused by every kernel that meets it: counted in
// bounds, skipped everywhere, never read through.  A member is a vertex of an accepted face.
//   bounds     the box of the members.  Minimum and maximum per thread, wave (shuffles) and block, then integer atomicMax on
//              an order-preserving image of the float (the lower corner on its complement), once per block of a grid that
//              strides over the faces; the result does not depend on arrival order.  One thread turns the images back
//              into floats.
//   -- the host reads the refused count and the box here, and fixes the grid (synchronisation 1) --
//   mark       a thread per face: member[v] = 1, a plain byte store.
//   cells      a thread per vertex: the cell of a member, occ[cell] = 1.
//   scan       chunked_exclusive_scan of scan.h over occ (one byte per cell): the occupied cells numbered in ascending
//              order.  From here on a vertex carries its compact cell number and everything is sized by V and F.
//   count      a thread per face: the faces whose corners lie in three different cells, counted per lowest cell (integer
//   scan       atomics), scanned, and listed per lowest cell as 16-byte records (face, middle and highest cell, orientation)
//   fill       through cursors.  The order within a bucket depends on arrival; nothing that is read from it does.
//   survive    a lane per face walks its bucket: p and q, the positive and negative faces of its key, and its own rank among
//              those of its key and orientation with a lower index; no sort.  A bucket of more than MAX_BUCKET records is not
//              walked: the face sets the overflow word and the host refuses the mesh.  A survivor marks its three cells used.
//              Without cancellation count / scan / fill / survive are one kernel: every face with three cells survives.
//   scan x 2   the used cells numbered in ascending order (V'), the survivors numbered in input order (F').
//   sums       a thread per vertex: a member of a used cell adds its quantised offset from the lower corner (int64 per axis)
//              and 1 into its cell's accumulators: integer atomics, exact, so the order of arrival does not show.  Runs of
//              consecutive lanes with the same cell are added up in the wave first.
//   -- the host reads V', F' and the overflow word here and allocates the result (synchronisation 2) --
//   emit       vertices (a thread per used cell: lo + (sum / count) / S in float64, rounded to float32 once), faces (a thread
//              per input face: the survivor's corners renumbered) and the map (a thread per input vertex).
// The kernels move 12-byte vertices and faces and 4-byte numbers; their bound is HBM and atomic traffic.  Contraction is off,
// as in mesh_voxelize.hip.  Measured: profiles/simplify.md.
//
// No reference counterpart: the reference writes NIfTI volumes only.
#include <math.h>

#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int FB = 256;                         // block of the per-face and per-vertex kernels
constexpr int64_t LIMIT = (int64_t)1 << 31;
constexpr int64_t MAX_CELLS = CTU_MESH_DECIMATE_MAX_CELLS;
constexpr int MAX_BUCKET = CTU_MESH_DECIMATE_MAX_BUCKET;
constexpr int BOUNDS_BLOCKS = 2048;             // 8 blocks of 256 threads on each of the 256 CUs

// the workspace of bounds (256 bytes); the host reads the first 32
struct BoundsHead {
    long long refused;
    float lo[3], hi[3];
    unsigned key[6];                             // the images of hi (3..5) and the complemented images of lo (0..2); 0: none yet
};
// at the start of the workspace of build and emit (256 bytes reserved); the host reads the first 24
struct Head { long long vp, fp, overflow, occupied, listed; };
static_assert(sizeof(BoundsHead) <= 256 && sizeof(Head) <= 256, "the heads have 256 bytes");

// the arrays sized by V and F come first: emit finds them without knowing the cells
struct Layout { size_t member, cnt, used, sum, num, zero_end, vocc, cursor, newid, surv, fpos, bucket, occ, cid, bsum, total; };
Layout layout(int64_t V, int64_t F, int64_t cells) {
    Layout l;
    size_t o = 256;
    l.member = o;  o += align256((size_t)V);                      // head .. num: cleared by one memset
    l.cnt = o;     o += align256((size_t)V * 4);
    l.used = o;    o += align256((size_t)V * 4);
    l.sum = o;     o += align256((size_t)V * 24);
    l.num = o;     o += align256((size_t)V * 4);
    l.zero_end = o;
    l.vocc = o;    o += align256((size_t)V * 4);
    l.cursor = o;  o += align256((size_t)V * 4);
    l.newid = o;   o += align256((size_t)V * 4);
    l.surv = o;    o += align256((size_t)F * 4);
    l.fpos = o;    o += align256((size_t)F * 4);
    l.bucket = o;  o += align256((size_t)F * 16);
    l.occ = o;     o += align256((size_t)cells);
    l.cid = o;     o += align256((size_t)cells * 4);
    const int64_t most = V > F ? (V > cells ? V : cells) : (F > cells ? F : cells);
    l.bsum = o;    o += align256((size_t)ceil_div64(most, CSCAN_CHUNK) * 8);
    l.total = o;
    return l;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V < LIMIT && F < LIMIT; }

struct Frame {
    double lo[3], cell[3], top[3], S;           // top = n - 1
    int n[3];
};

// S = 2^(30 - e) with the largest extent = m 2^e, 0.5 <= m < 1: a member's offset times S is at most 2^30
double scale_of(const float* lo, const float* hi) {
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = fmax(ext, (double)hi[a] - (double)lo[a]);
    int e = 0;
    frexp(ext, &e);
    return ldexp(1.0, 30 - e);
}

// lo <= hi and cell > 0, all finite: the grid of the rule; false if it has more than MAX_CELLS cells
bool frame_of(const float* lo, const float* hi, const float* cell, Frame* g, int64_t* cells) {
    double total = 1.0;
    for (int a = 0; a < 3; ++a) {
        g->lo[a] = (double)lo[a];
        g->cell[a] = (double)cell[a];
        const double d = (double)hi[a] - (double)lo[a];
        const double n = floor(d / (double)cell[a]) + 1.0;
        if (!(n <= (double)MAX_CELLS)) return false;
        g->n[a] = (int)n;
        g->top[a] = n - 1.0;
        total *= n;
    }
    if (total > (double)MAX_CELLS) return false;
    *cells = (int64_t)g->n[0] * g->n[1] * g->n[2];
    g->S = scale_of(lo, hi);
    return true;
}

bool finite3(const float* v) { return v[0] - v[0] == 0.f && v[1] - v[1] == 0.f && v[2] - v[2] == 0.f; }

// ------------------------------------------------------------------------------------------------ bounds
// an image of a finite float whose unsigned order is the float's order; never 0
__device__ __forceinline__ unsigned image_of(float x) {
    const unsigned u = __float_as_uint(x + 0.f);                   // -0 becomes +0
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float float_of(unsigned k) { return __uint_as_float(k & 0x80000000u ? k & 0x7fffffffu : ~k); }

// the three indices of face t if all lie in [0, V) and all nine coordinates are finite
__device__ __forceinline__ bool accepted(const float* __restrict__ vert, int V, const int* __restrict__ faces, int64_t t, int (&i)[3],
                                         float (&p)[9]) {
    i[0] = faces[3 * t]; i[1] = faces[3 * t + 1]; i[2] = faces[3 * t + 2];
    if ((unsigned)i[0] >= (unsigned)V || (unsigned)i[1] >= (unsigned)V || (unsigned)i[2] >= (unsigned)V) return false;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = vert[(int64_t)i[q] * 3 + a];
            p[3 * q + a] = x;
            ok = ok && x - x == 0.f;
        }
    return ok;
}

// A block strides over the faces and issues its box once, so the launch puts at most 6 x BOUNDS_BLOCKS atomics on the six
// words of the head.  A wave per 64 faces doing so queued 680 k of them on one cache line: 7.7 ms of an 8.8 ms call on
// 7.3 M faces, and still 1.9 ms with a read of the word in front of every atomic.
__global__ void __launch_bounds__(FB) dec_bounds_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int64_t F,
                                                        BoundsHead* head) {
    __shared__ float lds[FB / 64][6];
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    unsigned refused = 0;
    for (int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x; t < F; t += (int64_t)gridDim.x * FB) {
        int i[3];
        float p[9];
        if (accepted(vert, V, faces, t, i, p)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], fminf(p[a], fminf(p[3 + a], p[6 + a])));
                hi[a] = fmaxf(hi[a], fmaxf(p[a], fmaxf(p[3 + a], p[6 + a])));
            }
        } else {
            ++refused;
        }
    }
    if (refused) atomicAdd((unsigned long long*)&head->refused, (unsigned long long)refused);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
        }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lds[threadIdx.x >> 6][a] = lo[a];
            lds[threadIdx.x >> 6][3 + a] = hi[a];
        }
    }
    __syncthreads();
    if (threadIdx.x >= 3) return;
    const int a = threadIdx.x;
    float l = lds[0][a], h = lds[0][3 + a];
    for (int w = 1; w < FB / 64; ++w) {
        l = fminf(l, lds[w][a]);
        h = fmaxf(h, lds[w][3 + a]);
    }
    if (l <= h) {                                                   // the block met an accepted face
        atomicMax(&head->key[a], ~image_of(l));
        atomicMax(&head->key[3 + a], image_of(h));
    }
}

__global__ void dec_bounds_final_kernel(BoundsHead* head) {
    const int a = threadIdx.x;
    if (a >= 3) return;
    const unsigned kl = head->key[a], kh = head->key[3 + a];
    head->lo[a] = kl ? float_of(~kl) : 0.f;                         // no accepted face: the box is the origin
    head->hi[a] = kh ? float_of(kh) : 0.f;
}

// ------------------------------------------------------------------------------------------------ cells
__global__ void __launch_bounds__(FB) dec_mark_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces, int64_t F,
                                                      uint8_t* __restrict__ member) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    int i[3];
    float p[9];
    if (!accepted(vert, V, faces, t, i, p)) return;
    member[i[0]] = 1;
    member[i[1]] = 1;
    member[i[2]] = 1;
}

__global__ void __launch_bounds__(FB) dec_cells_kernel(const float* __restrict__ vert, int V, const uint8_t* __restrict__ member, Frame g,
                                                       int* __restrict__ vocc, uint8_t* __restrict__ occ) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= V) return;
    if (!member[v]) {
        vocc[v] = -1;
        return;
    }
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = (double)vert[3 * v + a] - g.lo[a];
        double t = floor(d / g.cell[a]);
        t = t >= 0.0 ? t : 0.0;                                     // only a frame that is not the members' own gets here
        t = t <= g.top[a] ? t : g.top[a];
        c[a] = (int)t;
    }
    const int id = (int)(((int64_t)c[0] * g.n[1] + c[1]) * g.n[2] + c[2]);
    vocc[v] = id;
    occ[id] = 1;
}

__global__ void __launch_bounds__(FB) dec_compact_kernel(int V, const int* __restrict__ cid, int* __restrict__ vocc) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= V) return;
    const int id = vocc[v];
    if (id < 0) return;
    const int k = cid[id];
    vocc[v] = (unsigned)k < (unsigned)V ? k : -1;                   // at most one occupied cell per member: k < V
}

// ------------------------------------------------------------------------------------------------ faces
struct Key { int s, mn, mx, positive; };

// the compact cells of face t's corners; false for a face that is skipped (refused, or fewer than three different cells)
__device__ __forceinline__ bool face_cells(const int* __restrict__ faces, int64_t t, int V, const int* __restrict__ vocc, int (&g)[3]) {
    const int i[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    if ((unsigned)i[0] >= (unsigned)V || (unsigned)i[1] >= (unsigned)V || (unsigned)i[2] >= (unsigned)V) return false;
    g[0] = vocc[i[0]]; g[1] = vocc[i[1]]; g[2] = vocc[i[2]];
    if (g[0] < 0 || g[1] < 0 || g[2] < 0) return false;              // a vertex that is no member: the face was refused
    return g[0] != g[1] && g[1] != g[2] && g[2] != g[0];
}

// rotated so that the lowest cell comes first: (s, x, y); positive if x < y
__device__ __forceinline__ Key key_of(const int (&g)[3]) {
    const int r = g[0] < g[1] ? (g[0] < g[2] ? 0 : 2) : (g[1] < g[2] ? 1 : 2);
    const int s = g[r], x = g[r == 2 ? 0 : r + 1], y = g[r == 0 ? 2 : r - 1];
    return {s, x < y ? x : y, x < y ? y : x, x < y ? 1 : 0};
}

__device__ __forceinline__ void mark_used(int* __restrict__ used, const int (&g)[3]) {
    used[g[0]] = 1;
    used[g[1]] = 1;
    used[g[2]] = 1;
}

// cancel off: every face with three different cells survives
__global__ void __launch_bounds__(FB) dec_keep_kernel(const int* __restrict__ faces, int64_t F, int V, const int* __restrict__ vocc,
                                                      int* __restrict__ surv, int* __restrict__ used) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    int g[3];
    const bool ok = face_cells(faces, t, V, vocc, g);
    surv[t] = ok ? 1 : 0;
    if (ok) mark_used(used, g);
}

// FILL: cursor holds the buckets' next free positions
template <bool FILL>
__global__ void __launch_bounds__(FB) dec_bucket_kernel(const int* __restrict__ faces, int64_t F, int V, const int* __restrict__ vocc,
                                                        int* __restrict__ cnt_or_cursor, int4* __restrict__ bucket) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    int g[3];
    if (!face_cells(faces, t, V, vocc, g)) return;
    const Key k = key_of(g);
    const int pos = atomicAdd(cnt_or_cursor + k.s, 1);
    if (FILL && (unsigned)pos < (unsigned)F) bucket[pos] = make_int4((int)t, k.mn, k.mx, k.positive);
}

__global__ void __launch_bounds__(FB) dec_survive_kernel(const int* __restrict__ faces, int64_t F, int V, const int* __restrict__ vocc,
                                                         const int* __restrict__ cnt, const int* __restrict__ cursor,
                                                         const int4* __restrict__ bucket, int* __restrict__ surv,
                                                         int* __restrict__ used, Head* head) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F) return;
    int g[3];
    int alive = 0;
    if (face_cells(faces, t, V, vocc, g)) {
        const Key k = key_of(g);
        const int n = cnt[k.s];
        const int64_t end = cursor[k.s], start = end - n;           // after the fill a cursor is its bucket's end
        if (n > MAX_BUCKET) {
            head->overflow = 1;                                     // every writer stores the same value
        } else if (n > 0 && start >= 0 && end <= F) {
            int p = 0, q = 0, rank = 0;
            for (int64_t j = start; j < end; ++j) {
                const int4 e = bucket[j];
                if (e.y != k.mn || e.z != k.mx) continue;
                if (e.w) ++p; else ++q;
                if ((e.w != 0) == (k.positive != 0) && e.x < (int)t) ++rank;
            }
            alive = k.positive ? (p > q && rank < p - q) : (q > p && rank < q - p);
        }
    }
    surv[t] = alive;
    if (alive) mark_used(used, g);
}

// ------------------------------------------------------------------------------------------------ positions
// Vertices that follow each other in the array often share a cluster (extract_surface numbers them cell by cell), so a wave
// first adds up every run of consecutive lanes with the same cluster (a segmented scan by shuffles) and the last lane of a
// run issues its four atomics.  The sums are integers: how they are grouped does not show.
__global__ void __launch_bounds__(FB) dec_sums_kernel(const float* __restrict__ vert, int V, const int* __restrict__ vocc,
                                                      const int* __restrict__ used, const int* __restrict__ newid, Frame g,
                                                      long long* __restrict__ sum, int* __restrict__ num) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int j = -1;                                                     // -1: this lane adds nothing
    long long q[3] = {0, 0, 0};
    int n = 0;
    if (v < V) {
        const int k = vocc[v];
        if (k >= 0 && used[k]) {
            const int id = newid[k];
            if ((unsigned)id < (unsigned)V) {
                j = id;
                n = 1;
#pragma unroll
                for (int a = 0; a < 3; ++a) q[a] = (long long)rint(((double)vert[3 * v + a] - g.lo[a]) * g.S);
            }
        }
    }
    const int before = __shfl_up(j, 1), after = __shfl_down(j, 1);
    const bool first = lane == 0 || before != j, last = lane == 63 || after != j;
    const unsigned long long firsts = __ballot(first);
    const int run = __popcll(firsts & (~0ull >> (63 - lane)));      // the number of this lane's run: runs are contiguous
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int r = __shfl_up(run, o), m = __shfl_up(n, o);
        const long long x = __shfl_up(q[0], o), y = __shfl_up(q[1], o), z = __shfl_up(q[2], o);
        if (lane >= o && r == run) {
            q[0] += x; q[1] += y; q[2] += z;
            n += m;
        }
    }
    if (j < 0 || !last) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd((unsigned long long*)&sum[3 * (int64_t)j + a], (unsigned long long)q[a]);
    atomicAdd(num + j, n);
}

__global__ void __launch_bounds__(FB) dec_vertices_kernel(int64_t Vp, const long long* __restrict__ sum, const int* __restrict__ num,
                                                          Frame g, float* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (j >= Vp) return;
    const double n = (double)num[j];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double mean = (double)sum[3 * j + a] / n;
        const double off = mean / g.S;
        out[3 * j + a] = (float)(g.lo[a] + off);
    }
}

__global__ void __launch_bounds__(FB) dec_faces_kernel(const int* __restrict__ faces, int64_t F, int V, const int* __restrict__ vocc,
                                                       const int* __restrict__ surv, const int* __restrict__ fpos,
                                                       const int* __restrict__ newid, int64_t Fp, int* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (t >= F || !surv[t]) return;
    const int64_t p = fpos[t];
    int g[3];
    if (p < 0 || p >= Fp || !face_cells(faces, t, V, vocc, g)) return;
    out[3 * p] = newid[g[0]];
    out[3 * p + 1] = newid[g[1]];
    out[3 * p + 2] = newid[g[2]];
}

__global__ void __launch_bounds__(FB) dec_map_kernel(int V, const int* __restrict__ vocc, const int* __restrict__ used,
                                                     const int* __restrict__ newid, int* __restrict__ map) {
    const int64_t v = (int64_t)blockIdx.x * FB + threadIdx.x;
    if (v >= V) return;
    const int k = vocc[v];
    map[v] = k >= 0 && used[k] ? newid[k] : -1;
}

}  // namespace

extern "C" size_t ctu_mesh_decimate_ws_bytes(int64_t V, int64_t F, int64_t cells) {
    if (!sizes_ok(V, F) || cells < 0 || cells > MAX_CELLS) return 0;
    return cells == 0 ? 256 : layout(V, F, cells).total;
}

extern "C" int ctu_mesh_decimate_bounds(const float* vertices, int64_t V, const int32_t* faces, int64_t F, void* ws, void* stream) {
    CTU_REQUIRE(sizes_ok(V, F), "mesh_decimate_bounds: V and F must lie in [0, 2^31), got V = %lld, F = %lld", (long long)V, (long long)F);
    CTU_REQUIRE(F >= 1 && V >= 1, "mesh_decimate_bounds: takes at least one face and one vertex (an empty mesh decimates to itself)");
    CTU_REQUIRE(vertices && faces && ws, "mesh_decimate_bounds: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_decimate_bounds: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    CTU_REQUIRE(hipMemsetAsync(ws, 0, 256, st) == hipSuccess, "mesh_decimate_bounds: cannot clear the workspace");
    const int64_t blocks = ceil_div64(F, FB);
    dec_bounds_kernel<<<(unsigned)(blocks < BOUNDS_BLOCKS ? blocks : BOUNDS_BLOCKS), FB, 0, st>>>(vertices, (int)V, faces, F, (BoundsHead*)ws);
    CTU_CHECK_LAUNCH("mesh decimate bounds");
    dec_bounds_final_kernel<<<1, 64, 0, st>>>((BoundsHead*)ws);
    CTU_CHECK_LAUNCH("mesh decimate bounds final");
    return CTU_OK;
}

extern "C" int ctu_mesh_decimate_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                                       const float* cell_size, int64_t cells, int cancel, void* ws, void* stream) {
    CTU_REQUIRE(sizes_ok(V, F), "mesh_decimate_build: V and F must lie in [0, 2^31), got V = %lld, F = %lld", (long long)V, (long long)F);
    CTU_REQUIRE(F >= 1 && V >= 1, "mesh_decimate_build: takes at least one face and one vertex (an empty mesh decimates to itself)");
    CTU_REQUIRE(lo && hi && cell_size, "mesh_decimate_build: null lo, hi or cell_size");
    CTU_REQUIRE(finite3(lo) && finite3(hi) && lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2],
                "mesh_decimate_build: lo and hi must be finite with lo <= hi on every axis");
    CTU_REQUIRE(finite3(cell_size) && cell_size[0] > 0.f && cell_size[1] > 0.f && cell_size[2] > 0.f,
                "mesh_decimate_build: cell_size must be positive and finite, got (%g, %g, %g)", (double)cell_size[0],
                (double)cell_size[1], (double)cell_size[2]);
    Frame g;
    int64_t need = 0;
    CTU_REQUIRE(frame_of(lo, hi, cell_size, &g, &need), "mesh_decimate_build: the grid has more than %lld cells; choose a larger cell_size",
                (long long)MAX_CELLS);
    CTU_REQUIRE(cells == need, "mesh_decimate_build: cells = %lld is not the grid of this box and cell_size (%d x %d x %d = %lld)",
                (long long)cells, g.n[0], g.n[1], g.n[2], (long long)need);
    CTU_REQUIRE(vertices && faces && ws, "mesh_decimate_build: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_decimate_build: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(V, F, cells);
    unsigned char* b = (unsigned char*)ws;
    Head* head = (Head*)b;
    uint8_t* member = b + l.member;
    int* cnt = (int*)(b + l.cnt);
    int* used = (int*)(b + l.used);
    long long* sum = (long long*)(b + l.sum);
    int* num = (int*)(b + l.num);
    int* vocc = (int*)(b + l.vocc);
    int* cursor = (int*)(b + l.cursor);
    int* newid = (int*)(b + l.newid);
    int* surv = (int*)(b + l.surv);
    int* fpos = (int*)(b + l.fpos);
    int4* bucket = (int4*)(b + l.bucket);
    uint8_t* occ = b + l.occ;
    int* cid = (int*)(b + l.cid);
    long long* bsum = (long long*)(b + l.bsum);
    CTU_REQUIRE(hipMemsetAsync(ws, 0, l.zero_end, st) == hipSuccess && hipMemsetAsync(occ, 0, (size_t)cells, st) == hipSuccess,
                "mesh_decimate_build: cannot clear the workspace");
    const unsigned fgrid = (unsigned)ceil_div64(F, FB), vgrid = (unsigned)ceil_div64(V, FB);
    dec_mark_kernel<<<fgrid, FB, 0, st>>>(vertices, (int)V, faces, F, member);
    CTU_CHECK_LAUNCH("mesh decimate mark");
    dec_cells_kernel<<<vgrid, FB, 0, st>>>(vertices, (int)V, member, g, vocc, occ);
    CTU_CHECK_LAUNCH("mesh decimate cells");
    int rc = chunked_exclusive_scan(occ, cells, bsum, cid, &head->occupied, nullptr, st, "mesh decimate cell scan");
    if (rc != CTU_OK) return rc;
    dec_compact_kernel<<<vgrid, FB, 0, st>>>((int)V, cid, vocc);
    CTU_CHECK_LAUNCH("mesh decimate compact");
    if (cancel) {
        dec_bucket_kernel<false><<<fgrid, FB, 0, st>>>(faces, F, (int)V, vocc, cnt, bucket);
        CTU_CHECK_LAUNCH("mesh decimate count");
        rc = chunked_exclusive_scan(cnt, V, bsum, cursor, &head->listed, nullptr, st, "mesh decimate bucket scan");
        if (rc != CTU_OK) return rc;
        dec_bucket_kernel<true><<<fgrid, FB, 0, st>>>(faces, F, (int)V, vocc, cursor, bucket);
        CTU_CHECK_LAUNCH("mesh decimate fill");
        dec_survive_kernel<<<fgrid, FB, 0, st>>>(faces, F, (int)V, vocc, cnt, cursor, bucket, surv, used, head);
        CTU_CHECK_LAUNCH("mesh decimate survive");
    } else {
        dec_keep_kernel<<<fgrid, FB, 0, st>>>(faces, F, (int)V, vocc, surv, used);
        CTU_CHECK_LAUNCH("mesh decimate keep");
    }
    rc = chunked_exclusive_scan(used, V, bsum, newid, &head->vp, nullptr, st, "mesh decimate cluster scan");
    if (rc != CTU_OK) return rc;
    rc = chunked_exclusive_scan(surv, F, bsum, fpos, &head->fp, nullptr, st, "mesh decimate face scan");
    if (rc != CTU_OK) return rc;
    dec_sums_kernel<<<vgrid, FB, 0, st>>>(vertices, (int)V, vocc, used, newid, g, sum, num);
    CTU_CHECK_LAUNCH("mesh decimate sums");
    return CTU_OK;
}

extern "C" int ctu_mesh_decimate_emit(const int32_t* faces, int64_t V, int64_t F, int64_t Vp, int64_t Fp, const float* lo, const float* hi,
                                      float* out_vertices, int32_t* out_faces, int32_t* out_map, void* ws, void* stream) {
    CTU_REQUIRE(sizes_ok(V, F), "mesh_decimate_emit: V and F must lie in [0, 2^31), got V = %lld, F = %lld", (long long)V, (long long)F);
    CTU_REQUIRE(F >= 1 && V >= 1, "mesh_decimate_emit: takes at least one face and one vertex (an empty mesh decimates to itself)");
    CTU_REQUIRE(Vp >= 0 && Vp <= V && Fp >= 0 && Fp <= F, "mesh_decimate_emit: V' = %lld and F' = %lld are not the totals of a build of %lld "
                "vertices and %lld faces", (long long)Vp, (long long)Fp, (long long)V, (long long)F);
    CTU_REQUIRE(lo && hi, "mesh_decimate_emit: null lo or hi");
    CTU_REQUIRE(finite3(lo) && finite3(hi) && lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2],
                "mesh_decimate_emit: lo and hi must be finite with lo <= hi on every axis");
    CTU_REQUIRE(faces && ws && (Vp == 0 || out_vertices) && (Fp == 0 || out_faces), "mesh_decimate_emit: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_decimate_emit: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    Frame g = {};                                                   // the positions need lo and S of the frame, not its cells
    for (int a = 0; a < 3; ++a) g.lo[a] = (double)lo[a];
    g.S = scale_of(lo, hi);
    const Layout l = layout(V, F, 1);
    unsigned char* b = (unsigned char*)ws;
    const int* vocc = (const int*)(b + l.vocc);
    const int* used = (const int*)(b + l.used);
    const int* newid = (const int*)(b + l.newid);
    if (Vp) {
        dec_vertices_kernel<<<(unsigned)ceil_div64(Vp, FB), FB, 0, st>>>(Vp, (const long long*)(b + l.sum), (const int*)(b + l.num), g,
                                                                         out_vertices);
        CTU_CHECK_LAUNCH("mesh decimate vertices");
    }
    if (Fp) {
        dec_faces_kernel<<<(unsigned)ceil_div64(F, FB), FB, 0, st>>>(faces, F, (int)V, vocc, (const int*)(b + l.surv),
                                                                     (const int*)(b + l.fpos), newid, Fp, out_faces);
        CTU_CHECK_LAUNCH("mesh decimate faces");
    }
    if (out_map) {
        dec_map_kernel<<<(unsigned)ceil_div64(V, FB), FB, 0, st>>>((int)V, vocc, used, newid, out_map);
        CTU_CHECK_LAUNCH("mesh decimate map");
    }
    return CTU_OK;
}
