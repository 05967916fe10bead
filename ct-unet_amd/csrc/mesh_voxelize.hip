// Voxelisation of surface meshes, gfx950: mesh in, winding numbers or a mask out, on any grid; the inverse of mesh.hip's
// extraction (rule pinned in ctunet_amd/mesh.py; tests/mesh_voxelize_ref.py restates it in numpy).
//
// The value of a voxel is the winding number of the mesh around its centre, evaluated with one ray along x per (z, y) row:
// a face the ray crosses at depth x_c weighs +1 or -1 on every voxel of the row with x_k > x_c.
//   1. clear    one memset of the workspace: the head (the count of refused faces) and an int32 delta volume.
//   2. scatter  a lane per face: its edge functions in the (z, y) projection, its plane and the rows of the grid whose centres
//               lie in its bounding box (first_index(): an estimate, then corrected by explicit comparison, so the box is
//               exact).  Per row of the box: the three edge signs with the tie rule, the depth, the first voxel behind it, and
//               an integer atomicAdd of the weight on delta[i, j, k_first].  Integer adds commute: the result does not
//               depend on arrival order, two calls are bit-equal (the convention of mesh_smooth.hip's atomics).  A face with
//               more than COOP_ROWS rows in its box (one of an imported coarse mesh can cover 10^5) is not walked by its
//               lane: the wave takes these faces in turn (ballot, the face's indices and box broadcast from its lane, the
//               setup recomputed by every lane with the same arithmetic) and all 64 lanes stride over the rows.  A mesh of
//               few faces (an imported coarse one, whose faces are the large ones) is launched in several SLICES
//               (gridDim.y): slice 0 does all of the above, and every slice takes its share of the rows of the large
//               faces, so 12 triangles across a whole grid do not sit on one wave.  SLICES * F stays below SLICE_FACES, so
//               reading the faces once per slice costs nothing that matters.
//   3. scan     inclusive prefix sum of the deltas along x per row -> uint8 (winding != 0) or int32 (the windings).  A lane
//               owns 4 consecutive voxels where W % 4 == 0 (16-byte loads) and 1 otherwise; a wave takes 64 / SEG rows at a
//               time, SEG = the lanes of a row rounded up to a power of two and at most 64; longer rows go in steps of 64
//               lanes with a carry.  Reads and writes are coalesced along x.
// A face with an index outside [0, V) or a vertex that is not finite is counted in the head and never read through.
// Contraction is off: every float64 product, difference and sum rounds on its own, as numpy's do; two faces that share an
// edge evaluate bit-identical edge functions.  Measured: profiles/voxelize.md.
//
// No reference counterpart: the reference writes NIfTI volumes only.
#include "common.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)

namespace {

using ctu_vox::MAX_SIDE;

constexpr int FB = 256;                         // block of both kernels
constexpr int COOP_ROWS = 16;                   // a face with more rows than this in its box is walked by its whole wave
constexpr int SLICE_FACES = 1 << 16;            // slices = SLICE_FACES / F, in 1..MAX_SLICES
constexpr int MAX_SLICES = 256;
constexpr int SCAN_BLOCKS = 256 * 8;            // the scan's grid is capped here; a wave strides over the row groups
constexpr int64_t LIMIT = (int64_t)1 << 31;
constexpr size_t HEAD = 256;                    // bytes reserved for the head: int64 refused faces

struct Axes {
    double o[3], s[3];                          // origin and spacing in (z, y, x), the float32 arguments widened
    double inv[3];                              // 1 / s: first_index()'s estimate only, never a result
    int n[3];                                   // D, H, W
};

bool shape_ok(int D, int H, int W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= MAX_SIDE && H <= MAX_SIDE && W <= MAX_SIDE && (int64_t)D * H * W < LIMIT;
}

__device__ __forceinline__ double centre(const Axes& g, int a, int k) { return g.o[a] + (double)k * g.s[a]; }

// The smallest k in [0, n] whose centre on axis a is > x (STRICT) or >= x; n if there is none.  The centres do not decrease
// with k.  The estimate comes from a product with 1 / spacing (a float64 division costs about as much as the rest of a row)
// and is clamped in floating point before it becomes an integer (x may be +-inf or 1e30 widened); the comparisons then
// decide, so the result does not depend on how good the estimate is.  x is not NaN.
template <bool STRICT>
__device__ __forceinline__ int first_index(const Axes& g, int a, double x) {
    const int n = g.n[a];
    double t = floor((x - g.o[a]) * g.inv[a]);
    t = t >= 0.0 ? t : 0.0;                                          // also what a NaN estimate becomes
    t = t <= (double)n ? t : (double)n;
    int k = (int)t;
    while (k > 0 && (STRICT ? centre(g, a, k - 1) > x : centre(g, a, k - 1) >= x)) --k;
    while (k < n && !(STRICT ? centre(g, a, k) > x : centre(g, a, k) >= x)) ++k;
    return k;
}

__device__ __forceinline__ int sign_of(double v) { return (v > 0.0) - (v < 0.0); }

// What the rows of one face share.  Edge q runs from corner q to corner (q + 1) % 3; its function is evaluated from the
// endpoint of lower vertex index (a) to the other (b), and `flip` bit q says that the face traverses it from b to a.
struct Face {
    double az[3], ay[3], dz[3], dy[3];
    double p0z, p0y, p0x, nz, ny, area;
    int flip;
};

__device__ __forceinline__ void load_vertex(const float* __restrict__ vert, int i, double (&p)[3]) {
    const float* v = vert + (int64_t)i * 3;
    p[0] = (double)v[0];
    p[1] = (double)v[1];
    p[2] = (double)v[2];
}

__device__ __forceinline__ bool finite3(const double (&p)[3]) { return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0; }

// idx: three distinct indices in [0, V).  Returns false for a vertex that is not finite (f is then not filled).
__device__ __forceinline__ bool face_setup(const float* __restrict__ vert, const int (&idx)[3], Face& f, double (&lo)[2], double (&hi)[2]) {
    double p[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) load_vertex(vert, idx[q], p[q]);
    if (!(finite3(p[0]) && finite3(p[1]) && finite3(p[2]))) return false;
    f.flip = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int r = q == 2 ? 0 : q + 1;
        const bool forward = idx[q] < idx[r];
        const double* a = forward ? p[q] : p[r];
        const double* b = forward ? p[r] : p[q];
        f.az[q] = a[0];
        f.ay[q] = a[1];
        f.dz[q] = b[0] - a[0];
        f.dy[q] = b[1] - a[1];
        f.flip |= forward ? 0 : 1 << q;
    }
    const double e1z = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1x = p[1][2] - p[0][2];
    const double e2z = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2x = p[2][2] - p[0][2];
    f.area = e1z * e2y - e1y * e2z;                                  // the projection's doubled area; positive: entering
    f.nz = e1y * e2x - e1x * e2y;
    f.ny = e1x * e2z - e1z * e2x;
    f.p0z = p[0][0];
    f.p0y = p[0][1];
    f.p0x = p[0][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        lo[a] = fmin(p[0][a], fmin(p[1][a], p[2][a]));
        hi[a] = fmax(p[0][a], fmax(p[1][a], p[2][a]));
    }
    return true;
}

// the ray of row (i, j) against one face: the crossing's weight (0: none) and k, the first voxel of the row behind it
__device__ __forceinline__ int face_row(const Face& f, const Axes& g, int i, int j, int& k) {
    const double pz = centre(g, 0, i), py = centre(g, 1, j);
    int s[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double e = f.dz[q] * (py - f.ay[q]) - f.dy[q] * (pz - f.az[q]);
        int t = sign_of(e);
        if (t == 0) t = -sign_of(f.dy[q]);                           // the ray shifted by (+eps, +eps^2) in (z, y)
        if (t == 0) t = sign_of(f.dz[q]);
        s[q] = (f.flip >> q) & 1 ? -t : t;
    }
    if (s[0] == 0 || s[0] != s[1] || s[1] != s[2]) return 0;
    const double num = f.nz * (pz - f.p0z) + f.ny * (py - f.p0y);
    const double xc = f.p0x - num / f.area;
    if (xc != xc) return 0;
    k = first_index<true>(g, 2, xc);
    return k < g.n[2] ? s[0] : 0;                                    // a crossing behind the last centre is dropped
}

// (i, j) lies in the grid, so the add stays inside the delta volume
__device__ __forceinline__ void scatter_row(const Face& f, const Axes& g, int i, int j, int* __restrict__ delta) {
    int k;
    const int w = face_row(f, g, i, j, k);
    if (w) atomicAdd(delta + ((int64_t)i * g.n[1] + j) * g.n[2] + k, w);
}

struct Box { int i0, j0, nj, rows; };                                // rows i0.., columns j0 .. j0 + nj - 1; rows = their product

__device__ __forceinline__ Box row_box(const Axes& g, const double (&lo)[2], const double (&hi)[2]) {
    const int i0 = first_index<false>(g, 0, lo[0]), i1 = first_index<true>(g, 0, hi[0]);
    const int j0 = first_index<false>(g, 1, lo[1]), j1 = first_index<true>(g, 1, hi[1]);
    Box b = {i0, j0, j1 - j0, 0};
    if (i1 > i0 && j1 > j0) b.rows = (i1 - i0) * (j1 - j0);           // at most 1024 * 1024
    return b;
}

__global__ void __launch_bounds__(FB) voxelize_scatter_kernel(const float* __restrict__ vert, int V, const int* __restrict__ faces,
                                                              int64_t F, Axes g, int* __restrict__ delta,
                                                              unsigned long long* __restrict__ refused) {
    const int64_t t = (int64_t)blockIdx.x * FB + threadIdx.x;
    const bool first = blockIdx.y == 0;                              // the slice that counts refused faces and walks small boxes
    int idx[3] = {0, 0, 0};
    Box box = {0, 0, 0, 0};
    Face f;
    if (t < F) {
        idx[0] = faces[3 * t];
        idx[1] = faces[3 * t + 1];
        idx[2] = faces[3 * t + 2];
        if ((unsigned)idx[0] >= (unsigned)V || (unsigned)idx[1] >= (unsigned)V || (unsigned)idx[2] >= (unsigned)V) {
            if (first) atomicAdd(refused, 1ull);
        } else {
            double lo[2], hi[2];
            if (!face_setup(vert, idx, f, lo, hi)) {
                if (first) atomicAdd(refused, 1ull);
            } else if (idx[0] != idx[1] && idx[1] != idx[2] && idx[2] != idx[0] && f.area != 0.0) box = row_box(g, lo, hi);
        }
    }
    if (first && box.rows <= COOP_ROWS)
        for (int r = 0, i = box.i0, j = 0; r < box.rows; ++r) {
            scatter_row(f, g, i, box.j0 + j, delta);
            if (++j == box.nj) {
                j = 0;
                ++i;
            }
        }
    // every lane of the wave arrives here: the faces with large boxes, one after the other, all lanes on each
    unsigned long long big = __ballot(box.rows > COOP_ROWS);
    const int lane = threadIdx.x & 63, r0 = blockIdx.y * 64 + lane, step = gridDim.y * 64;
    while (big) {
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        const int bidx[3] = {__shfl(idx[0], src), __shfl(idx[1], src), __shfl(idx[2], src)};
        const Box b = {__shfl(box.i0, src), __shfl(box.j0, src), __shfl(box.nj, src), __shfl(box.rows, src)};
        Face fb;
        double lo[2], hi[2];
        face_setup(vert, bidx, fb, lo, hi);                          // the lane that owns it has checked the face
        for (int r = r0; r < b.rows; r += step) scatter_row(fb, g, b.i0 + r / b.nj, b.j0 + r % b.nj, delta);
    }
}

template <class T> __device__ __forceinline__ T scan_value(int s);
template <> __device__ __forceinline__ uint8_t scan_value<uint8_t>(int s) { return s != 0; }
template <> __device__ __forceinline__ int scan_value<int>(int s) { return s; }

template <class T> struct Out4;
template <> struct Out4<uint8_t> { typedef uchar4 type; };
template <> struct Out4<int> { typedef int4 type; };

// A lane owns VEC consecutive voxels of a row; seg lanes (a power of two in 1..64, seg * VEC >= W where that fits a wave)
// hold one row, and a wave holds 64 / seg rows side by side.  VEC = 4 (one 16-byte load, one 4- or 16-byte store) needs
// W % 4 == 0, so that a lane's four voxels lie in its row together and on a 16-byte boundary; VEC = 1 takes any W.
template <class T, int VEC>
__global__ void __launch_bounds__(FB) voxelize_scan_kernel(const int* __restrict__ delta, int64_t rows, int W, int seg, T* __restrict__ out) {
    const int lane = threadIdx.x & 63, l_in = lane & (seg - 1), per = 64 / seg;
    const int64_t groups = (rows + per - 1) / per, waves = (int64_t)gridDim.x * (FB / 64);
    for (int64_t grp = ((int64_t)blockIdx.x * FB + threadIdx.x) >> 6; grp < groups; grp += waves) {
        const int64_t row = grp * per + lane / seg;
        const int64_t base = row * W;
        int carry = 0;
        for (int x0 = 0; x0 < W; x0 += 64 * VEC) {                   // one step for W <= 64 * VEC
            const int x = x0 + l_in * VEC;
            const bool in = row < rows && x < W;
            int v[VEC];
            if (VEC == 4) {
                const int4 q = in ? *reinterpret_cast<const int4*>(delta + base + x) : make_int4(0, 0, 0, 0);
                v[0] = q.x;
                v[1 % VEC] = v[0] + q.y;                             // the prefix within the lane
                v[2 % VEC] = v[1 % VEC] + q.z;
                v[3 % VEC] = v[2 % VEC] + q.w;
            } else {
                v[0] = in ? delta[base + x] : 0;
            }
            int s = v[VEC - 1];
            for (int o = 1; o < seg; o <<= 1) {
                const int y = __shfl_up(s, o);
                if (l_in >= o) s += y;
            }
            const int before = carry + s - v[VEC - 1];               // everything left of this lane's voxels
            if (in) {
                if (VEC == 4) {
                    typename Out4<T>::type r;
                    r.x = scan_value<T>(before + v[0]);
                    r.y = scan_value<T>(before + v[1 % VEC]);
                    r.z = scan_value<T>(before + v[2 % VEC]);
                    r.w = scan_value<T>(before + v[3 % VEC]);
                    *reinterpret_cast<typename Out4<T>::type*>(out + base + x) = r;
                } else {
                    out[base + x] = scan_value<T>(before + v[0]);
                }
            }
            carry += __shfl(s, lane | (seg - 1));
        }
    }
}

template <class T>
int launch_scan(const int* delta, int D, int H, int W, void* out, hipStream_t st) {
    const bool vec = W % 4 == 0 && (uintptr_t)out % 16 == 0;        // delta is 16-byte aligned with the workspace
    const int lanes = vec ? W / 4 : W;
    int seg = 1;
    while (seg < lanes && seg < 64) seg <<= 1;
    const int64_t rows = (int64_t)D * H, groups = ceil_div64(rows, 64 / seg);
    const int64_t blocks = ceil_div64(groups, FB / 64);
    const unsigned grid = (unsigned)(blocks < SCAN_BLOCKS ? blocks : SCAN_BLOCKS);
    if (vec) voxelize_scan_kernel<T, 4><<<grid, FB, 0, st>>>(delta, rows, W, seg, (T*)out);
    else voxelize_scan_kernel<T, 1><<<grid, FB, 0, st>>>(delta, rows, W, seg, (T*)out);
    CTU_CHECK_LAUNCH("mesh voxelize scan");
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_mesh_voxelize_ws_bytes(int D, int H, int W) {
    return shape_ok(D, H, W) ? HEAD + align256((size_t)D * H * W * 4) : 0;
}

extern "C" int ctu_mesh_voxelize(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int D, int H, int W,
                                 const float* spacing, const float* origin, int want_winding, void* out, void* ws, void* stream) {
    CTU_REQUIRE(shape_ok(D, H, W), "mesh_voxelize: bad shape %dx%dx%d (every side in 1..%d, D*H*W < 2^31)", D, H, W, MAX_SIDE);
    CTU_REQUIRE(V >= 0 && F >= 0 && V < LIMIT && F < LIMIT, "mesh_voxelize: V and F must lie in [0, 2^31), got V = %lld, F = %lld",
                (long long)V, (long long)F);
    CTU_REQUIRE(F == 0 || V > 0, "mesh_voxelize: faces without vertices");
    Axes g;
    for (int a = 0; a < 3; ++a) {
        const float s = spacing ? spacing[a] : 1.f, o = origin ? origin[a] : 0.f;
        CTU_REQUIRE(s > 0.f && s < __builtin_inff() && o - o == 0.f, "mesh_voxelize: spacing must be positive and finite, origin finite");
        g.s[a] = (double)s;
        g.o[a] = (double)o;
        g.inv[a] = 1.0 / (double)s;
    }
    g.n[0] = D;
    g.n[1] = H;
    g.n[2] = W;
    CTU_REQUIRE(out && ws, "mesh_voxelize: null pointer");
    CTU_REQUIRE((uintptr_t)ws % 16 == 0, "mesh_voxelize: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t voxels = (size_t)D * H * W;
    if (F == 0) {                                                    // the empty mesh: zeros, and a zero head
        CTU_REQUIRE(hipMemsetAsync(ws, 0, HEAD, st) == hipSuccess && hipMemsetAsync(out, 0, voxels * (want_winding ? 4 : 1), st) == hipSuccess,
                    "mesh_voxelize: cannot clear the output");
        return CTU_OK;
    }
    CTU_REQUIRE(vertices && faces, "mesh_voxelize: null pointer");
    CTU_REQUIRE(hipMemsetAsync(ws, 0, HEAD + voxels * 4, st) == hipSuccess, "mesh_voxelize: cannot clear the workspace");
    int* delta = (int*)((unsigned char*)ws + HEAD);
    const int64_t slices = SLICE_FACES / F < 1 ? 1 : (SLICE_FACES / F > MAX_SLICES ? MAX_SLICES : SLICE_FACES / F);
    voxelize_scatter_kernel<<<dim3((unsigned)ceil_div64(F, FB), (unsigned)slices), FB, 0, st>>>(vertices, (int)V, faces, F, g, delta, (unsigned long long*)ws);
    CTU_CHECK_LAUNCH("mesh voxelize scatter");
    return want_winding ? launch_scan<int>(delta, D, H, W, out, st) : launch_scan<uint8_t>(delta, D, H, W, out, st);
}
