// Free-form deformation (FFD): a cubic B-spline displacement over a lattice of control points, fitted to the chamfer cost
// of registration.hip behind a frozen affine matrix, and applied to points and volumes, gfx950 (rule:
// ctunet_amd/registration.py, "B-spline deformable registration"; tests/ffd_ref.py restates it in numpy float64).
//
//   T(p) = q0 + u(q0), q0 = M p;  u = the 64-term sum of spatial.hip over the lattice laid on the fixed field's box.
//
// The fit.  q0 and so the lattice cell of a point never change, so the wrapper bins the points by cell once (ffd_cells_kernel,
// then a stable sort) and cuts every cell's run into segments of at most SEG = 256 points.  Per iteration, all float64 with
// contraction off, no float atomics, nothing allocated, no host synchronisation:
//   ffd_accumulate_kernel  one block per segment: stages the cell's 4^3 x 3 candidate controls in LDS; a thread per point
//                          forms q = T(p), samples the field (field_sample.h) and leaves (v g, |g|^2, Bz, By, Bx) in LDS;
//                          thread (k, component) then sums the segment IN POINT ORDER into its slab row of 64 x 4 doubles
//                          (gradient z, y, x and the majorising diagonal per control of the cell); the segment's sum of r^2
//                          and inlier count by a fixed tree.
//   ffd_reduce_kernel      one block: the segments' costs in a fixed order, the regulariser of the candidate lattice, the
//                          accept / reject decision, lambda and the history row; it also commits the previous step (below).
//   ffd_step_kernel        a wave per control point: on an accept its 64 lanes gather the <= 64 cells that touch the control
//                          (each lane its cell's segments in order, then a fixed xor tree), add the regulariser and store
//                          gradient, diagonal and the accepted control; then the next candidate
//                          c - grad / ((1 + lambda) d + 1e-12) goes into the OTHER candidate buffer.
// A candidate entry that is not finite is not written (the accepted value is) and raises an integer flag; the next reduce
// (or ffd_finish_kernel after the last iteration) then marks that step refused and keeps the old candidate buffer current.
// LDS of the accumulation: 32 KiB of point records + 1.5 KiB of controls + 3 KiB of reduction = 36.5 KiB, four blocks a CU.
//
// What cannot fault: the segment tables come from the wrapper, yet every index read from them is checked against its range
// before use (a bad one counts as an absent point); a knot is clamped into the lattice (NaN -> 0) before it indexes a control;
// every field and volume read sits behind the comparison that declares it inside (NaN fails).
//
// ffd_transform_kernel pushes points through T (and gives det(I + du/dq0) from the analytic derivative weights);
// ffd_resample_kernel is affine.hip's kernel with s = T(w) in place of s = M w: same tiling (chunk_tile.h), same sampler
// (trilinear.h), controls read from global memory (a 64^3 lattice does not fit LDS).
//
// No reference counterpart: the reference expects scans registered to its atlas by a host tool (ctunet/pytorch/datasets.py:22-45).
#include <type_traits>

#include "chunk_tile.h"
#include "common.h"
#include "field_sample.h"
#include "trilinear.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_field;
using namespace ctu_tile;
using namespace ctu_tri;

constexpr int SEG = CTU_FFD_SEGMENT;            // points of a segment = threads of its block
constexpr int ROW = 256;                        // doubles of a slab row: 64 controls x (gradient z, y, x, diagonal)
constexpr int RED_B = 1024;
constexpr int STEP_B = 256;                     // four waves = four control points
constexpr int PT_B = 256;
constexpr size_t HEAD = 1024;                   // bytes of the workspace head
constexpr int MAX_BATCH = 65535;                // grid.y
static_assert(SEG == 256 && ROW == 4 * 64, "ffd: a thread per (control of the cell, component)");

struct Lattice {
    int G[3], nc[3];                            // control points and cells per axis, G = nc + 3
    double h[3], org[3];                        // control spacing, the box origin
};

struct State {
    double cost, sum2, reg;                     // accepted: total cost, sum of r^2, regulariser energy
    double lambda, w;
    long long count;                            // inliers of the accepted controls
    int cur;                                    // the candidate buffer the last accumulation read
    int go;                                     // the last step kernel was allowed to move
    int bad;                                    // ... and met a candidate entry that was not finite
    int accepted;                               // the last decision
};
static_assert(sizeof(State) <= HEAD, "ffd: the state outgrew the workspace head");

// the workspace after the head, in doubles: accepted controls [n3], two candidate buffers [2][n3], gradient [n3], diagonal
// [g3], segment costs [S], segment counts [S] (int64 bits), slab [S][ROW]
struct Ws {
    State* s;
    double *acc, *buf, *grad, *diag, *segcost, *slab;
    long long* segcount;
};
__host__ __device__ inline Ws carve(void* ws, int64_t g3, int64_t S) {
    Ws w;
    w.s = (State*)ws;
    double* d = (double*)((char*)ws + HEAD);
    w.acc = d; d += 3 * g3;
    w.buf = d; d += 6 * g3;
    w.grad = d; d += 3 * g3;
    w.diag = d; d += g3;
    w.segcost = d; d += S;
    w.segcount = (long long*)d; d += S;
    w.slab = d;
    return w;
}

// uniform cubic B-spline weights of the fraction f (spatial.hip's) and their derivatives
__device__ __forceinline__ void bspline(double f, double B[4]) {
    const double omf = 1.0 - f, f2 = f * f, f3 = f2 * f;
    B[0] = ((omf * omf) * omf) / 6.0;
    B[1] = ((3.0 * f3 - 6.0 * f2) + 4.0) / 6.0;
    B[2] = ((((-3.0 * f3) + 3.0 * f2) + 3.0 * f) + 1.0) / 6.0;
    B[3] = f3 / 6.0;
}
__device__ __forceinline__ void dbspline(double f, double dB[4]) {
    const double omf = 1.0 - f, f2 = f * f;
    dB[0] = (-(omf * omf)) / 2.0;
    dB[1] = (3.0 * f2 - 4.0 * f) / 2.0;
    dB[2] = (((-3.0 * f2) + 2.0 * f) + 1.0) / 2.0;
    dB[3] = f2 / 2.0;
}

// t = clamp((q - org) / h, 0, nc), NaN -> 0; cell = min(floor(t), nc - 1) in 0 .. nc - 1; f = t - cell; free: t was not clamped
__device__ __forceinline__ void knot(double q, double org, double h, int nc, int& cell, double& f, bool& free_) {
    double t = (q - org) / h;
    free_ = t >= 0.0 && t <= (double)nc;
    t = t >= 0.0 ? t : 0.0;
    t = t <= (double)nc ? t : (double)nc;
    cell = min((int)floor(t), nc - 1);
    f = t - (double)cell;
}

// the 64 terms in spatial.hip's order (z outermost, x innermost) over controls in GLOBAL memory
__device__ __forceinline__ void displace(const Lattice& L, const double* __restrict__ ctl, const int c[3], const double B[3][4],
                                         double e[3]) {
    const int g3 = L.G[0] * L.G[1] * L.G[2];
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double wzy = B[0][l] * B[1][k];
            const double* p = ctl + ((c[0] + l) * L.G[1] + (c[1] + k)) * L.G[2] + c[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double wt = wzy * B[2][j];
                e0 = e0 + wt * p[j];
                e1 = e1 + wt * p[g3 + j];
                e2 = e2 + wt * p[2 * g3 + j];
            }
        }
    }
    e[0] = e0; e[1] = e1; e[2] = e2;
}

__global__ void __launch_bounds__(PT_B) ffd_cells_kernel(Lattice L, const float* __restrict__ pts, int64_t P,
                                                         const double* __restrict__ matrix, int* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * PT_B + threadIdx.x;
    if (i >= P) return;
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = matrix[k];
    const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
    double q0[3];
    apply(M, p, q0);
    int c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double f;
        bool fr;
        knot(q0[r], L.org[r], L.h[r], L.nc[r], c[r], f, fr);
    }
    cells[i] = (c[0] * L.nc[1] + c[1]) * L.nc[2] + c[2];
}

__global__ void __launch_bounds__(PT_B) ffd_init_kernel(int g3, const double* __restrict__ init, double w, Ws ws,
                                                        double* __restrict__ control) {
    const int i = blockIdx.x * PT_B + threadIdx.x;
    if (i < 3 * g3) {
        const double v = init ? init[i] : 0.0;
        ws.acc[i] = v;
        ws.buf[i] = v;
        ws.buf[3 * g3 + i] = v;
        ws.grad[i] = 0.0;
        if (i < g3) ws.diag[i] = 0.0;
        control[i] = v;
    }
    if (i == 0) {
        State* s = ws.s;
        s->cost = __builtin_inf();
        s->sum2 = __builtin_inf();
        s->reg = 0.0;
        s->lambda = 1e-3;
        s->w = w;
        s->count = 0;
        s->cur = 0;
        s->go = 0;
        s->bad = 0;
        s->accepted = 0;
    }
}

// the candidate buffer an accumulation reads: the one the last step wrote, unless that step was refused
__device__ __forceinline__ int current(const State* s) { return s->go && !s->bad ? 1 - s->cur : s->cur; }

struct AccArgs {
    Lattice L;
    FieldGrid f;
    double bound;
    int64_t P;
    int S;
    const float* pts;
    const double* matrix;
    const float* field;
    const int *perm, *seg_cell, *seg_begin, *seg_count;
};

__global__ void __launch_bounds__(SEG) ffd_accumulate_kernel(AccArgs a, Ws ws) {
    __shared__ double ctl[3][64];
    __shared__ double rec[SEG][16];
    __shared__ double red[SEG];
    __shared__ int cnt[SEG];
    const int t = threadIdx.x, sg = blockIdx.x;
    const Lattice& L = a.L;
    const int g3 = L.G[0] * L.G[1] * L.G[2], ncells = L.nc[0] * L.nc[1] * L.nc[2];
    int cell = a.seg_cell[sg], count = a.seg_count[sg];
    const int begin = a.seg_begin[sg];
    if ((unsigned)cell >= (unsigned)ncells || count < 0 || begin < 0) {        // a table the wrapper did not build
        cell = 0;
        count = 0;
    }
    count = min(count, SEG);
    const int c2 = cell % L.nc[2], c1 = cell / L.nc[2] % L.nc[1], c0 = cell / (L.nc[2] * L.nc[1]);
    const double* cand = ws.buf + (int64_t)current(ws.s) * 3 * g3;
    if (t < 192) {
        const int comp = t >> 6, k = t & 63;
        ctl[comp][k] = cand[comp * g3 + ((c0 + (k >> 4)) * L.G[1] + (c1 + ((k >> 2) & 3))) * L.G[2] + (c2 + (k & 3))];
    }
    __syncthreads();
    double r2 = 0.0;
    int inl = 0;
    if (t < count) {
        double vg[4] = {0.0, 0.0, 0.0, 0.0}, B[3][4];
        const int64_t at = (int64_t)begin + t;
        const int idx = at < a.P ? a.perm[at] : -1;
        bool have = idx >= 0 && idx < a.P;
        if (have) {
            double M[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) M[k] = a.matrix[k];
            const double p[3] = {(double)a.pts[3 * (int64_t)idx], (double)a.pts[3 * (int64_t)idx + 1],
                                 (double)a.pts[3 * (int64_t)idx + 2]};
            double q[3];
            apply(M, p, q);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                int c;
                double f;
                bool fr;
                knot(q[r], L.org[r], L.h[r], L.nc[r], c, f, fr);
                bspline(f, B[r]);
            }
            double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll 1
            for (int l = 0; l < 4; ++l) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double wzy = B[0][l] * B[1][k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double wt = wzy * B[2][j];
                        const int kk = l * 16 + k * 4 + j;
                        e0 = e0 + wt * ctl[0][kk];
                        e1 = e1 + wt * ctl[1][kk];
                        e2 = e2 + wt * ctl[2][kk];
                    }
                }
            }
            q[0] = q[0] + e0; q[1] = q[1] + e1; q[2] = q[2] + e2;
            double v, g[3];
            double rr = a.bound < __builtin_inf() ? a.bound : 0.0;
            if (sample_inlier(a.f, a.field, q, a.bound, v, g)) {
                vg[0] = v * g[0]; vg[1] = v * g[1]; vg[2] = v * g[2];
                vg[3] = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                rr = v;
                inl = 1;
            }
            r2 = rr * rr;
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) B[r][j] = 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            rec[t][j] = vg[j];
            rec[t][4 + j] = B[0][j];
            rec[t][8 + j] = B[1][j];
            rec[t][12 + j] = B[2][j];
        }
    }
    red[t] = r2;
    cnt[t] = inl;
    __syncthreads();
    {
        const int k = t >> 2, comp = t & 3;
        const int l = 4 + (k >> 4), m = 8 + ((k >> 2) & 3), n = 12 + (k & 3);
        double acc = 0.0;
        for (int i = 0; i < count; ++i) {                                       // point order
            const double B = (rec[i][l] * rec[i][m]) * rec[i][n];
            acc = acc + rec[i][comp] * B;
        }
        ws.slab[(int64_t)sg * ROW + t] = acc;
    }
    for (int o = SEG / 2; o > 0; o >>= 1) {
        if (t < o) {
            red[t] = red[t] + red[t + o];
            cnt[t] += cnt[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        ws.segcost[sg] = red[0];
        ws.segcount[sg] = cnt[0];
    }
}

__global__ void __launch_bounds__(RED_B) ffd_reduce_kernel(Lattice L, int64_t P, int S, int it, Ws ws, double* __restrict__ history) {
    __shared__ double ra[RED_B], rb[RED_B];
    __shared__ long long rc[RED_B];
    const int t = threadIdx.x;
    State* s = ws.s;
    const int g3 = L.G[0] * L.G[1] * L.G[2];
    const int cur = current(s);
    const bool refused_before = s->go && s->bad;
    const double* c = ws.buf + (int64_t)cur * 3 * g3;
    double a = 0.0;
    long long n = 0;
    for (int i = t; i < S; i += RED_B) {
        a = a + ws.segcost[i];
        n += ws.segcount[i];
    }
    // the regulariser: every control's edges towards +z, +y and +x
    double b = 0.0;
    const int sy = L.G[2], sz = L.G[1] * L.G[2];
    for (int j = t; j < g3; j += RED_B) {
        const int x = j % L.G[2], y = j / L.G[2] % L.G[1], z = j / sz;
        const double v0 = c[j], v1 = c[g3 + j], v2 = c[2 * g3 + j];
        if (z + 1 < L.G[0]) {
            const double d0 = v0 - c[j + sz], d1 = v1 - c[g3 + j + sz], d2 = v2 - c[2 * g3 + j + sz];
            b = b + ((d0 * d0 + d1 * d1) + d2 * d2);
        }
        if (y + 1 < L.G[1]) {
            const double d0 = v0 - c[j + sy], d1 = v1 - c[g3 + j + sy], d2 = v2 - c[2 * g3 + j + sy];
            b = b + ((d0 * d0 + d1 * d1) + d2 * d2);
        }
        if (x + 1 < L.G[2]) {
            const double d0 = v0 - c[j + 1], d1 = v1 - c[g3 + j + 1], d2 = v2 - c[2 * g3 + j + 1];
            b = b + ((d0 * d0 + d1 * d1) + d2 * d2);
        }
    }
    ra[t] = a; rb[t] = b; rc[t] = n;
    __syncthreads();
    for (int o = RED_B / 2; o > 0; o >>= 1) {
        if (t < o) {
            ra[t] = ra[t] + ra[t + o];
            rb[t] = rb[t] + rb[t + o];
            rc[t] += rc[t + o];
        }
        __syncthreads();
    }
    if (t != 0) return;
    if (refused_before && it > 0) history[6 * (int64_t)(it - 1) + 5] = -1.0;
    const double sum2_c = ra[0], reg_c = (0.5 * s->w) * rb[0];
    const double cost_c = 0.5 * sum2_c + reg_c;
    const bool accepted = cost_c < s->cost;                        // NaN and +inf: rejected
    double lambda = s->lambda;
    if (accepted) {
        s->cost = cost_c;
        s->sum2 = sum2_c;
        s->reg = reg_c;
        s->count = rc[0];
        lambda = fmax(lambda / 3.0, 1e-9);
    } else {
        lambda = fmin(lambda * 10.0, 1e9);
    }
    s->lambda = lambda;
    s->cur = cur;
    s->accepted = accepted ? 1 : 0;
    s->go = s->count > 0 ? 1 : 0;
    s->bad = 0;
    double* h = history + 6 * (int64_t)it;
    h[0] = s->cost / (double)P;
    h[1] = sqrt(s->sum2 / (double)P);
    h[2] = s->reg;
    h[3] = (double)s->count;
    h[4] = lambda;
    h[5] = s->go ? (accepted ? 1.0 : 0.0) : -1.0;
}

__global__ void __launch_bounds__(STEP_B) ffd_step_kernel(Lattice L, int S, Ws ws, const int* __restrict__ cell_seg,
                                                          double* __restrict__ control) {
    State* s = ws.s;
    const int g3 = L.G[0] * L.G[1] * L.G[2];
    const int j = blockIdx.x * (STEP_B / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= g3) return;                                                        // a whole wave
    const int sy = L.G[2], sz = L.G[1] * L.G[2];
    const int gx = j % L.G[2], gy = j / L.G[2] % L.G[1], gz = j / sz;
    const double* cand = ws.buf + (int64_t)s->cur * 3 * g3;
    double* next = ws.buf + (int64_t)(1 - s->cur) * 3 * g3;
    const double w = s->w;
    const int comp = min(lane, 2);                                              // lanes 0..2 own a component each
    double cv, gr, d;
    if (s->accepted) {
        // lane (l, m, n): the cell in which this control is number (l, m, n) of the 4^3
        const int l = lane >> 4, m = (lane >> 2) & 3, n = lane & 3;
        const int cz = gz - l, cy = gy - m, cx = gx - n;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (cz >= 0 && cz < L.nc[0] && cy >= 0 && cy < L.nc[1] && cx >= 0 && cx < L.nc[2]) {
            const int cell = (cz * L.nc[1] + cy) * L.nc[2] + cx;
            const int s0 = max(cell_seg[cell], 0), s1 = min(cell_seg[cell + 1], S);
            for (int sg = s0; sg < s1; ++sg) {                                  // the cell's segments in order
                const double* row = ws.slab + (int64_t)sg * ROW + lane * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = acc[k] + row[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o);
        const double* ca = cand + comp * g3;
        cv = ca[j];
        int deg = 0;
        double ns = 0.0;
        if (gz > 0) { ns = ns + ca[j - sz]; ++deg; }
        if (gz + 1 < L.G[0]) { ns = ns + ca[j + sz]; ++deg; }
        if (gy > 0) { ns = ns + ca[j - sy]; ++deg; }
        if (gy + 1 < L.G[1]) { ns = ns + ca[j + sy]; ++deg; }
        if (gx > 0) { ns = ns + ca[j - 1]; ++deg; }
        if (gx + 1 < L.G[2]) { ns = ns + ca[j + 1]; ++deg; }
        gr = (comp == 0 ? acc[0] : comp == 1 ? acc[1] : acc[2]) + w * ((double)deg * cv - ns);
        d = acc[3] + (2.0 * w) * (double)deg;
        if (lane < 3) {
            ws.grad[comp * g3 + j] = gr;
            ws.acc[comp * g3 + j] = cv;
            control[comp * g3 + j] = cv;
            if (lane == 0) ws.diag[j] = d;
        }
    } else {
        cv = ws.acc[comp * g3 + j];
        gr = ws.grad[comp * g3 + j];
        d = ws.diag[j];
    }
    if (!s->go || lane >= 3) return;
    const double nv = cv - gr / ((1.0 + s->lambda) * d + 1e-12);
    if (finite(nv)) {
        next[comp * g3 + j] = nv;
    } else {
        next[comp * g3 + j] = cv;
        atomicOr(&s->bad, 1);
    }
}

__global__ void ffd_finish_kernel(int rows, Ws ws, double* __restrict__ history) {
    const State* s = ws.s;
    if (s->go && s->bad) history[6 * (int64_t)(rows - 1) + 5] = -1.0;
}

// ---- applying a fitted field -------------------------------------------------------------------------------------------
template <bool JAC>
__global__ void __launch_bounds__(PT_B) ffd_transform_kernel(Lattice L, const float* __restrict__ pts, int64_t P,
                                                             const double* __restrict__ matrix, const double* __restrict__ ctl,
                                                             float* __restrict__ out, double* __restrict__ jac) {
    const int64_t i = (int64_t)blockIdx.x * PT_B + threadIdx.x;
    if (i >= P) return;
    double M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = matrix[k];
    const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
    double q[3], B[3][4], f[3], e[3];
    int c[3];
    bool fr[3];
    apply(M, p, q);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        knot(q[r], L.org[r], L.h[r], L.nc[r], c[r], f[r], fr[r]);
        bspline(f[r], B[r]);
    }
    displace(L, ctl, c, B, e);
    if (out) {
#pragma unroll
        for (int r = 0; r < 3; ++r) out[3 * i + r] = (float)(q[r] + e[r]);
    }
    if (!JAC) return;
    // D[a][b] = sum c_a W_b, W_b the weight product with axis b's weights replaced by their derivatives (zero where the knot
    // was clamped); J = I + D / h_b; det by the first row's cofactors
    double dB[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        dbspline(f[r], dB[r]);
        if (!fr[r]) dB[r][0] = dB[r][1] = dB[r][2] = dB[r][3] = 0.0;
    }
    const int g3 = L.G[0] * L.G[1] * L.G[2];
    double D[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const double* pc = ctl + ((c[0] + l) * L.G[1] + (c[1] + k)) * L.G[2] + c[2];
            const double w0zy = dB[0][l] * B[1][k], w1zy = B[0][l] * dB[1][k], w2zy = B[0][l] * B[1][k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double W[3] = {w0zy * B[2][j], w1zy * B[2][j], w2zy * dB[2][j]};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double cv = pc[a * g3 + j];
#pragma unroll
                    for (int b = 0; b < 3; ++b) D[a][b] = D[a][b] + W[b] * cv;
                }
            }
        }
    }
    double J[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) J[a][b] = (a == b ? 1.0 : 0.0) + D[a][b] / L.h[b];
    const double m0 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double m1 = J[1][0] * J[2][2] - J[1][2] * J[2][0];
    const double m2 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    jac[i] = (J[0][0] * m0 - J[0][1] * m1) + J[0][2] * m2;
}

struct RsArgs {
    int D, H, W;                                // input grid
    int d, h, w;                                // output grid
    int ntx, nty;
    int K;
    double sp[3], org[3], osp[3], oorg[3];      // (z, y, x)
    double fill;
    const double* m;                            // DEVICE: row-major, the first 12 entries are read
    const double* ctl;                          // DEVICE [3][Gz][Gy][Gx]
    Lattice L;
};

// NaN fails both comparisons
__device__ __forceinline__ bool within(double v, double lo, int n) { return v >= lo && v < (double)n; }

template <class T, int MODE>
__global__ void __launch_bounds__(SB) ffd_resample_kernel(RsArgs a, const T* __restrict__ in,
                                                          typename OutOf<T, MODE>::type* __restrict__ out) {
    typedef typename OutOf<T, MODE>::type O;
    constexpr int VX = 16 / (int)sizeof(O);
    const Origin t = origin<O>(a.ntx, a.nty);
    int yy, zz;
    row_of(t, yy, zz);
    if (yy >= a.h || zz >= a.d) return;
    const T* item = in + (int64_t)blockIdx.y * a.D * a.H * a.W;
    O* orow = out + (int64_t)blockIdx.y * a.d * a.h * a.w + ((int64_t)zz * a.h + yy) * a.w;
    const Span s = chunk_of(orow, t.X0, a.w);
    if (s.xa >= s.xb) return;

    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = a.m[i];
    const double w0 = a.oorg[0] + (double)zz * a.osp[0], w1 = a.oorg[1] + (double)yy * a.osp[1];
    double base[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) base[r] = m[4 * r] * w0 + m[4 * r + 1] * w1;
    const int n[3] = {a.D, a.H, a.W};
    O fillv;                                                   // the entry point has checked that O holds the value
    if constexpr (std::is_floating_point<O>::value) fillv = (O)a.fill;
    else fillv = (O)(long long)a.fill;

    Chunk<O> res;
#pragma unroll 1
    for (int v = 0; v < VX; ++v) {
        const int x = min(max(s.cx + v, 0), a.w - 1);          // a clipped voxel repeats its neighbour and is not stored
        const double w2 = a.oorg[2] + (double)x * a.osp[2];
        double q[3], B[3][4], e[3], u[3];
        int c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            q[r] = (base[r] + m[4 * r + 2] * w2) + m[4 * r + 3];
            double f;
            bool fr;
            knot(q[r], a.L.org[r], a.L.h[r], a.L.nc[r], c[r], f, fr);
            bspline(f, B[r]);
        }
        displace(a.L, a.ctl, c, B, e);
#pragma unroll
        for (int r = 0; r < 3; ++r) u[r] = ((q[r] + e[r]) - a.org[r]) / a.sp[r];
        // from here on affine.hip's rule per mode
        O val = fillv;
        if constexpr (MODE == NEAREST) {
            const double f0 = floor(u[0] + 0.5), f1 = floor(u[1] + 0.5), f2 = floor(u[2] + 0.5);
            if (within(f0, 0.0, n[0]) && within(f1, 0.0, n[1]) && within(f2, 0.0, n[2]))
                val = item[((int)f0 * a.H + (int)f1) * a.W + (int)f2];
        } else if (within(u[0], -1.0, n[0]) && within(u[1], -1.0, n[1]) && within(u[2], -1.0, n[2])) {
            int i0[3];
            float wt[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double f = floor(u[r]);
                i0[r] = (int)f;                                // -1 .. n - 1
                wt[r] = (float)(u[r] - f);
            }
            O cn[8];                                           // a neighbour outside the volume reads as the fill
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int z = i0[0] + (j >> 2), y = i0[1] + ((j >> 1) & 1), xx = i0[2] + (j & 1);
                const bool ok = z >= 0 && z < a.D && y >= 0 && y < a.H && xx >= 0 && xx < a.W;
                cn[j] = ok ? (O)item[(z * a.H + y) * a.W + xx] : fillv;
            }
            if constexpr (MODE == LINEAR) {
                val = tri(cn, wt[2], wt[1], wt[0]);
            } else {
                val = (O)label_vote(cn, a.K, wt[2], wt[1], wt[0]);
            }
        } else if constexpr (MODE == LABEL) {
            val = (unsigned)fillv < (unsigned)a.K ? fillv : (O)0;
        }
        res.v[v] = val;
    }
    store(orow, s, res, true);
}

template <class T, int MODE>
int launch(RsArgs a, const void* in, int64_t N, void* out, hipStream_t st) {
    typedef typename OutOf<T, MODE>::type O;
    const Tiles tl = tiles(a.d, a.h, a.w, out, sizeof(O));
    a.ntx = tl.ntx;
    a.nty = tl.nty;
    const int64_t vin = (int64_t)a.D * a.H * a.W, vout = (int64_t)a.d * a.h * a.w;
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const int64_t nb = N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH;
        const dim3 grid((unsigned)tl.blocks, (unsigned)nb);
        ffd_resample_kernel<T, MODE><<<grid, SB, 0, st>>>(a, (const T*)in + n0 * vin, (O*)out + n0 * vout);
        CTU_CHECK_LAUNCH("ffd_resample");
    }
    return CTU_OK;
}

// the lattice of an entry point's arguments; false with the reason in `why`
bool lattice(Lattice& L, const int* G, const double* h, const double* box_origin, const char** why) {
    *why = "null pointer";
    if (!G || !h || !box_origin) return false;
    *why = "every G must lie in 4..64";
    for (int i = 0; i < 3; ++i) {
        if (G[i] < 4 || G[i] > CTU_FFD_MAX_G) return false;
        L.G[i] = G[i];
        L.nc[i] = G[i] - 3;
        L.h[i] = h[i];
        L.org[i] = box_origin[i];
    }
    *why = "control_spacing must be positive and finite, box_origin finite";
    return steps_ok(L.h) && finite_n(L.org, 3);
}

#define FFD_LATTICE(L, name)                                                         \
    Lattice L;                                                                       \
    {                                                                                \
        const char* why;                                                             \
        CTU_REQUIRE(lattice(L, G, control_spacing, box_origin, &why), name ": %s", why); \
    }

}  // namespace

extern "C" size_t ctu_ffd_ws_bytes(const int* G, int64_t S) {
    if (!G || S < 1) return 0;
    for (int i = 0; i < 3; ++i)
        if (G[i] < 4 || G[i] > CTU_FFD_MAX_G) return 0;
    const int64_t g3 = (int64_t)G[0] * G[1] * G[2];
    return HEAD + (size_t)(13 * g3 + 2 * S + S * ROW) * sizeof(double);
}

extern "C" int ctu_ffd_cells(const float* points, int64_t P, const double* matrix, const int* G, const double* control_spacing,
                             const double* box_origin, int* cells, void* stream) {
    CTU_REQUIRE(points && matrix && cells, "ffd_cells: null pointer");
    CTU_REQUIRE(P >= 1 && P < ((int64_t)1 << 31), "ffd_cells: P must lie in 1 .. 2^31 - 1, got %lld", (long long)P);
    FFD_LATTICE(L, "ffd_cells");
    ffd_cells_kernel<<<(unsigned)ceil_div64(P, PT_B), PT_B, 0, (hipStream_t)stream>>>(L, points, P, matrix, cells);
    CTU_CHECK_LAUNCH("ffd_cells");
    return CTU_OK;
}

extern "C" int ctu_ffd_init(const int* G, int64_t S, const double* init_control, double weight, void* ws, double* control,
                            void* stream) {
    CTU_REQUIRE(ws && control && G, "ffd_init: null pointer");
    CTU_REQUIRE(ctu_ffd_ws_bytes(G, S) > 0, "ffd_init: every G must lie in 4..64 and S be at least 1");
    CTU_REQUIRE(weight >= 0.0 && weight - weight == 0.0, "ffd_init: the regulariser weight must be finite and >= 0");
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "ffd_init: the workspace must be 8-byte aligned");
    const int g3 = G[0] * G[1] * G[2];
    ffd_init_kernel<<<ceil_div(3 * g3, PT_B), PT_B, 0, (hipStream_t)stream>>>(g3, init_control, weight, carve(ws, g3, S), control);
    CTU_CHECK_LAUNCH("ffd_init");
    return CTU_OK;
}

extern "C" int ctu_ffd_accumulate(const float* points, int64_t P, const double* matrix, const float* field, int D, int H, int W,
                                  const double* spacing, const double* origin, const int* G, const double* control_spacing,
                                  const double* box_origin, double max_distance, const int* perm, const int* seg_cell,
                                  const int* seg_begin, const int* seg_count, int64_t S, void* ws, void* stream) {
    CTU_REQUIRE(points && matrix && field && perm && seg_cell && seg_begin && seg_count && ws, "ffd_accumulate: null pointer");
    CTU_REQUIRE(P >= 1 && P < ((int64_t)1 << 31), "ffd_accumulate: P must lie in 1 .. 2^31 - 1, got %lld", (long long)P);
    CTU_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "ffd_accumulate: S must lie in 1 .. 2^31 - 1, got %lld", (long long)S);
    CTU_REQUIRE(D >= 2 && H >= 2 && W >= 2 && grid_ok(D, H, W),
                "ffd_accumulate: bad field shape %dx%dx%d (every side >= 2, D*H*W < 2^31)", D, H, W);
    CTU_REQUIRE(max_distance >= 0.0, "ffd_accumulate: max_distance must be >= 0 (+inf: no bound)");
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "ffd_accumulate: the workspace must be 8-byte aligned");
    FFD_LATTICE(L, "ffd_accumulate");
    AccArgs a;
    a.L = L;
    a.f.n[0] = D; a.f.n[1] = H; a.f.n[2] = W;
    for (int i = 0; i < 3; ++i) {
        a.f.sp[i] = spacing ? spacing[i] : 1.0;
        a.f.org[i] = origin ? origin[i] : 0.0;
    }
    CTU_REQUIRE(steps_ok(a.f.sp) && finite_n(a.f.org, 3), "ffd_accumulate: spacing must be positive and finite, origin finite");
    a.bound = max_distance; a.P = P; a.S = (int)S;
    a.pts = points; a.matrix = matrix; a.field = field;
    a.perm = perm; a.seg_cell = seg_cell; a.seg_begin = seg_begin; a.seg_count = seg_count;
    ffd_accumulate_kernel<<<(unsigned)S, SEG, 0, (hipStream_t)stream>>>(a, carve(ws, (int64_t)L.G[0] * L.G[1] * L.G[2], S));
    CTU_CHECK_LAUNCH("ffd_accumulate");
    return CTU_OK;
}

extern "C" int ctu_ffd_update(int64_t P, const int* G, const double* control_spacing, const double* box_origin,
                              const int* cell_seg, int64_t S, int it, double* control, double* history, int history_rows, void* ws,
                              void* stream) {
    CTU_REQUIRE(cell_seg && control && history && ws, "ffd_update: null pointer");
    CTU_REQUIRE(P >= 1 && S >= 1 && S < ((int64_t)1 << 31), "ffd_update: P and S must be at least 1");
    CTU_REQUIRE(it >= 0 && it < history_rows, "ffd_update: iteration %d outside the %d history rows", it, history_rows);
    FFD_LATTICE(L, "ffd_update");
    const int g3 = L.G[0] * L.G[1] * L.G[2];
    const Ws w = carve(ws, g3, S);
    hipStream_t st = (hipStream_t)stream;
    ffd_reduce_kernel<<<1, RED_B, 0, st>>>(L, P, (int)S, it, w, history);
    CTU_CHECK_LAUNCH("ffd_update (reduce)");
    ffd_step_kernel<<<ceil_div(g3, STEP_B / 64), STEP_B, 0, st>>>(L, (int)S, w, cell_seg, control);
    CTU_CHECK_LAUNCH("ffd_update (step)");
    if (it == history_rows - 1) {
        ffd_finish_kernel<<<1, 1, 0, st>>>(history_rows, w, history);
        CTU_CHECK_LAUNCH("ffd_update (finish)");
    }
    return CTU_OK;
}

extern "C" int ctu_ffd_transform_points(const float* points, int64_t P, const double* matrix, const double* control, const int* G,
                                        const double* control_spacing, const double* box_origin, float* out, double* jacobian,
                                        void* stream) {
    CTU_REQUIRE(points && matrix && control && (out || jacobian), "ffd_transform_points: null pointer");
    CTU_REQUIRE(P >= 1 && P < ((int64_t)1 << 31), "ffd_transform_points: P must lie in 1 .. 2^31 - 1, got %lld", (long long)P);
    FFD_LATTICE(L, "ffd_transform_points");
    const unsigned nb = (unsigned)ceil_div64(P, PT_B);
    if (jacobian)
        ffd_transform_kernel<true><<<nb, PT_B, 0, (hipStream_t)stream>>>(L, points, P, matrix, control, out, jacobian);
    else
        ffd_transform_kernel<false><<<nb, PT_B, 0, (hipStream_t)stream>>>(L, points, P, matrix, control, out, nullptr);
    CTU_CHECK_LAUNCH("ffd_transform_points");
    return CTU_OK;
}

extern "C" int ctu_ffd_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W, int d, int h,
                                int w, const double* matrix, const double* control, const int* G, const double* control_spacing,
                                const double* box_origin, const double* spacing, const double* origin, const double* out_spacing,
                                const double* out_origin, double fill, void* out, void* stream) {
    CTU_REQUIRE(in && out && matrix && control, "ffd_resample: null pointer");
    CTU_REQUIRE(mode >= NEAREST && mode <= LABEL, "ffd_resample: unknown mode %d", mode);
    CTU_REQUIRE(N > 0 && grid_ok(D, H, W) && grid_ok(d, h, w),
                "ffd_resample: bad shape N=%lld in=%dx%dx%d out=%dx%dx%d (every side >= 1, D*H*W < 2^31 on either grid)",
                (long long)N, D, H, W, d, h, w);
    CTU_REQUIRE((!spacing || steps_ok(spacing)) && (!out_spacing || steps_ok(out_spacing)),
                "ffd_resample: spacing must be positive and finite");
    CTU_REQUIRE((!origin || finite_n(origin, 3)) && (!out_origin || finite_n(out_origin, 3)), "ffd_resample: origin must be finite");
    if (mode == LABEL)
        CTU_REQUIRE(num_classes >= 2 && num_classes <= 16, "ffd_resample: num_classes must lie in 2..16, got %d", num_classes);
    FFD_LATTICE(L, "ffd_resample");
    RsArgs a;
    a.D = D; a.H = H; a.W = W; a.d = d; a.h = h; a.w = w;
    a.K = num_classes; a.m = matrix; a.ctl = control; a.fill = fill; a.L = L;
    for (int i = 0; i < 3; ++i) {
        a.sp[i] = spacing ? spacing[i] : 1.0;
        a.org[i] = origin ? origin[i] : 0.0;
        a.osp[i] = out_spacing ? out_spacing[i] : 1.0;
        a.oorg[i] = out_origin ? out_origin[i] : 0.0;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool whole = fill == (double)(long long)fill, f32 = (double)(float)fill - (double)(float)fill == 0.0;
#define RS(T, MODE) return launch<T, MODE>(a, in, N, out, st)
    if (mode == NEAREST) {
        if (dtype == CTU_U8) {
            CTU_REQUIRE(whole && fill >= 0 && fill <= 255, "ffd_resample: fill %g is no uint8", fill);
            RS(uint8_t, NEAREST);
        }
        if (dtype == CTU_I16) {
            CTU_REQUIRE(whole && fill >= -32768 && fill <= 32767, "ffd_resample: fill %g is no int16", fill);
            RS(int16_t, NEAREST);
        }
        if (dtype == CTU_F32) {
            CTU_REQUIRE(f32, "ffd_resample: fill %g is not finite in float32", fill);
            RS(float, NEAREST);
        }
        CTU_REQUIRE(false, "ffd_resample: unsupported dtype %d for nearest (uint8, int16 or float32)", dtype);
    }
    if (mode == LINEAR) {
        CTU_REQUIRE(f32, "ffd_resample: fill %g is not finite in float32", fill);
        if (dtype == CTU_F32) RS(float, LINEAR);
        if (dtype == CTU_I16) RS(int16_t, LINEAR);
        if (dtype == CTU_U8) RS(uint8_t, LINEAR);
        CTU_REQUIRE(false, "ffd_resample: unsupported dtype %d for linear (float32, int16 or uint8)", dtype);
    }
    CTU_REQUIRE(whole && fill >= 0 && fill <= 255, "ffd_resample: fill %g is no uint8 label", fill);
    if (dtype == CTU_U8) RS(uint8_t, LABEL);
#undef RS
    CTU_REQUIRE(false, "ffd_resample: unsupported dtype %d for label_linear (uint8)", dtype);
}
