// Rigid registration of a point set to a distance field by Levenberg-Marquardt chamfer matching, gfx950 (rule:
// ctunet_amd/registration.py; tests/registration_ref.py restates it in numpy float64).
//
// Three kernels, all float64, contraction off for the file so that a point's terms are the restatement's bit for bit:
//   reg_init_kernel        one block: the mean of the finite points (fixed order) and the start state (M = M_c = init,
//                          cost = +inf, lambda = 1e-3) into the workspace; once per registration.
//   reg_accumulate_kernel  a thread per point with a grid stride, at most CTU_REG_MAX_BLOCKS blocks of 256: samples the field
//                          at M_c p, forms the residual and the Jacobian row about the candidate's pivot and adds the 21
//                          entries of upper H, the 6 of b and the cost into 28 registers, plus the inlier count; a fixed-order
//                          wave reduction (xor shuffles), then LDS across the 4 waves, then ONE slab row per block.  No float
//                          atomics: two calls are bit-equal.
//   reg_update_kernel      one block: sums the slab in block order, then one thread compares the costs, accepts or rejects
//                          the candidate, adapts lambda, solves the damped 6x6 system by Cholesky and forms the next
//                          candidate; writes the state, matrix, inverse and the iteration's history row.
// Everything that changes between iterations lives in the workspace, so a registration is 1 + 2 (iterations + 1) launches
// on one stream without a host synchronisation, and it can be captured into a graph.
// Every field read is guarded by the comparison that declares the point inside the field (NaN fails it).
// The similarity registration with the symmetric cost (sim_* kernels, ctu_similarity_*) follows the rigid entry points below.
//
// No reference counterpart: the reference expects scans registered to its atlas by a host tool (ctunet/pytorch/datasets.py:22-45).
#include "common.h"
#include "field_sample.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_field;                      // finite, lerp, apply, sample_inlier
typedef FieldGrid Grid;

constexpr int RB = 256;
constexpr int NW = RB / 64;
constexpr int NACC = 28;                        // 21 upper H, 6 b, cost
constexpr int ROW = 32;                         // doubles of a slab row: NACC sums, the count (int64 bits), padding
constexpr int MAX_BLOCKS = CTU_REG_MAX_BLOCKS;
constexpr int INIT_B = 1024;
constexpr int SUM_AHEAD = 16;                   // slab rows the update kernel loads ahead of their additions

// the workspace head, in doubles
struct State {
    double M[16], Mc[16];                       // accepted matrix, candidate
    double H[21], b[6];                         // of the accepted matrix
    double pivot[3], pivot_c[3], mean[3];
    double cost, lambda;
    long long count;                            // inliers of the accepted matrix
};
constexpr size_t HEAD = 1024;                   // bytes; the slab follows
static_assert(sizeof(State) <= HEAD, "registration: the state outgrew the workspace head");

struct AccArgs {
    int D, H, W;
    double sp[3], org[3];
    double bound;                               // +inf: none
};

__host__ __device__ inline int num_blocks(int64_t P) {
    const int64_t nb = (P + RB - 1) / RB;
    return (int)(nb < 1 ? 1 : (nb > MAX_BLOCKS ? MAX_BLOCKS : nb));
}

__global__ void __launch_bounds__(INIT_B) reg_init_kernel(const float* __restrict__ pts, int64_t P, const double* __restrict__ init,
                                                          State* __restrict__ s) {
    __shared__ double red[INIT_B][4];
    double sum[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    for (int64_t i = threadIdx.x; i < P; i += INIT_B) {
        const double p0 = pts[3 * i], p1 = pts[3 * i + 1], p2 = pts[3 * i + 2];
        if (finite(p0) && finite(p1) && finite(p2)) {
            sum[0] += p0; sum[1] += p1; sum[2] += p2;
            cnt += 1.0;
        }
    }
    red[threadIdx.x][0] = sum[0]; red[threadIdx.x][1] = sum[1]; red[threadIdx.x][2] = sum[2]; red[threadIdx.x][3] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < INIT_B; ++i)
        for (int a = 0; a < 4; ++a) t[a] += red[i][a];
    for (int a = 0; a < 3; ++a) s->mean[a] = t[3] > 0.0 ? t[a] / t[3] : 0.0;
    for (int i = 0; i < 16; ++i) {
        const double v = init ? init[i] : (i % 5 == 0 ? 1.0 : 0.0);
        s->M[i] = v;
        s->Mc[i] = v;
    }
    s->M[12] = s->M[13] = s->M[14] = 0.0; s->M[15] = 1.0;
    s->Mc[12] = s->Mc[13] = s->Mc[14] = 0.0; s->Mc[15] = 1.0;
    for (int i = 0; i < 21; ++i) s->H[i] = 0.0;
    for (int i = 0; i < 6; ++i) s->b[i] = 0.0;
    double pv[3];
    apply(s->Mc, s->mean, pv);
    for (int a = 0; a < 3; ++a) s->pivot[a] = s->pivot_c[a] = pv[a];
    s->cost = __builtin_inf();
    s->lambda = 1e-3;
    s->count = 0;
}

__global__ void __launch_bounds__(RB) reg_accumulate_kernel(AccArgs a, const float* __restrict__ pts, int64_t P,
                                                            const float* __restrict__ field, const State* __restrict__ s,
                                                            double* __restrict__ slab) {
    __shared__ double red[NW][NACC + 1];
    double M[12], pivot[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = s->Mc[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pivot[i] = s->pivot_c[i];
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    long long count = 0;
    const int n[3] = {a.D, a.H, a.W};
    const double rout = a.bound < __builtin_inf() ? a.bound : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < P; i += (int64_t)gridDim.x * RB) {
        const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double q[3], u[3];
        apply(M, p, q);
        bool inside = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            u[r] = (q[r] - a.org[r]) / a.sp[r];
            inside = inside && u[r] >= 0.0 && u[r] <= (double)(n[r] - 1);      // NaN fails
        }
        double rr = rout;
        if (inside) {
            int i0[3];
            double f[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double fl = fmin(floor(u[r]), (double)(n[r] - 2));
                i0[r] = (int)fl;                                               // 0 .. n - 2
                f[r] = u[r] - fl;
            }
            const float* c0 = field + ((int64_t)i0[0] * a.H + i0[1]) * a.W + i0[2];
            const float* c1 = c0 + (int64_t)a.H * a.W;
            const double c000 = c0[0], c001 = c0[1], c010 = c0[a.W], c011 = c0[a.W + 1];
            const double c100 = c1[0], c101 = c1[1], c110 = c1[a.W], c111 = c1[a.W + 1];
            const double c00 = lerp(c000, c001, f[2]), c01 = lerp(c010, c011, f[2]);
            const double c10 = lerp(c100, c101, f[2]), c11 = lerp(c110, c111, f[2]);
            const double cz0 = lerp(c00, c01, f[1]), cz1 = lerp(c10, c11, f[1]);
            const double v = lerp(cz0, cz1, f[0]);
            if (v <= a.bound) {
                double g[3];
                g[0] = (cz1 - cz0) / a.sp[0];
                g[1] = lerp(c01 - c00, c11 - c10, f[0]) / a.sp[1];
                g[2] = lerp(lerp(c001 - c000, c011 - c010, f[1]), lerp(c101 - c100, c111 - c110, f[1]), f[0]) / a.sp[2];
                const double d[3] = {q[0] - pivot[0], q[1] - pivot[1], q[2] - pivot[2]};
                const double J[6] = {d[1] * g[2] - d[2] * g[1], d[2] * g[0] - d[0] * g[2], d[0] * g[1] - d[1] * g[0],
                                     g[0], g[1], g[2]};
                int k = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) acc[k++] += J[r] * J[c];
#pragma unroll
                for (int r = 0; r < 6; ++r) acc[21 + r] += J[r] * v;
                rr = v;
                ++count;
            }
        }
        acc[27] += rr * rr;
    }
    // lanes of a wave in xor order, then the waves in order
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) red[wave][i] = acc[i];
        red[wave][NACC] = __longlong_as_double(count);
    }
    __syncthreads();
    if (threadIdx.x < ROW) {
        double* row = slab + (int64_t)blockIdx.x * ROW;
        const int e = threadIdx.x;
        if (e < NACC) {
            double t = red[0][e];
            for (int w = 1; w < NW; ++w) t += red[w][e];
            row[e] = t;
        } else if (e == NACC) {
            long long t = 0;
            for (int w = 0; w < NW; ++w) t += __double_as_longlong(red[w][NACC]);
            row[e] = __longlong_as_double(t);
        } else {
            row[e] = 0.0;
        }
    }
}

// exp of the skew matrix of w in the index order of the vectors
__device__ void rodrigues(const double w[3], double R[9]) {
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double t = sqrt(t2);
    double sa, sb;
    if (t < 1e-4) {
        sa = 1.0 - t2 / 6.0;
        sb = 0.5 - t2 / 24.0;
    } else {
        sa = sin(t) / t;
        sb = (1.0 - cos(t)) / t2;
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int k = 0; k < 3; ++k) kk += K[3 * i + k] * K[3 * k + j];
            R[3 * i + j] = (i == j ? 1.0 : 0.0) + sa * K[3 * i + j] + sb * kk;
        }
}

// delta of (H + lambda diag(H) + 1e-12 I) delta = -b; false: a pivot that is not positive, or a result that is not finite
__device__ bool solve(const double H21[21], const double b[6], double lambda, double x[6]) {
    double A[6][6], L[6][6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = H21[k++];
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + lambda * A[i][i] + 1e-12;
    for (int j = 0; j < 6; ++j) {
        double sdiag = A[j][j];
        for (int c = 0; c < j; ++c) sdiag -= L[j][c] * L[j][c];
        if (!(sdiag > 0.0) || !finite(sdiag)) return false;
        L[j][j] = sqrt(sdiag);
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
            for (int c = 0; c < j; ++c) t -= L[i][c] * L[j][c];
            L[i][j] = t / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double t = -b[i];
        for (int c = 0; c < i; ++c) t -= L[i][c] * y[c];
        y[i] = t / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double t = y[i];
        for (int c = i + 1; c < 6; ++c) t -= L[c][i] * x[c];
        x[i] = t / L[i][i];
    }
    for (int i = 0; i < 6; ++i)
        if (!finite(x[i])) return false;
    return true;
}

__global__ void __launch_bounds__(64) reg_update_kernel(int64_t P, int nb, int it, State* __restrict__ s,
                                                        const double* __restrict__ slab, double* __restrict__ matrix,
                                                        double* __restrict__ inverse, double* __restrict__ history) {
    __shared__ double tot[ROW];
    const int e = threadIdx.x;
    if (e <= NACC) {
        // rows in block order; SUM_AHEAD loads are issued before their additions, so the order of the sum is unchanged and
        // a row costs an addition, not a round trip to memory
        double t = 0.0;
        long long n = 0;
        int r = 0;
        for (; r + SUM_AHEAD <= nb; r += SUM_AHEAD) {
            double v[SUM_AHEAD];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) v[k] = slab[(int64_t)(r + k) * ROW + e];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) {
                t += v[k];
                n += __double_as_longlong(v[k]);
            }
        }
        for (; r < nb; ++r) {
            const double v = slab[(int64_t)r * ROW + e];
            t += v;
            n += __double_as_longlong(v);
        }
        tot[e] = e < NACC ? t : __longlong_as_double(n);
    }
    __syncthreads();
    if (e != 0) return;
    const double cost_c = tot[27];
    const bool accepted = cost_c < s->cost;                        // NaN: rejected
    double lambda = s->lambda;
    if (accepted) {
        for (int i = 0; i < 16; ++i) s->M[i] = s->Mc[i];
        for (int i = 0; i < 21; ++i) s->H[i] = tot[i];
        for (int i = 0; i < 6; ++i) s->b[i] = tot[21 + i];
        for (int i = 0; i < 3; ++i) s->pivot[i] = s->pivot_c[i];
        s->cost = cost_c;
        s->count = __double_as_longlong(tot[NACC]);
        lambda = fmax(lambda / 3.0, 1e-9);
    } else {
        lambda = fmin(lambda * 10.0, 1e9);
    }
    s->lambda = lambda;
    double flag = accepted ? 1.0 : 0.0;
    double delta[6], H[21], b[6];
    for (int i = 0; i < 21; ++i) H[i] = s->H[i];
    for (int i = 0; i < 6; ++i) b[i] = s->b[i];
    bool ok = s->count >= CTU_REG_MIN_INLIERS && solve(H, b, lambda, delta);
    double cand[12];
    if (ok) {
        double R[9], pv[3], M[12];
        rodrigues(delta, R);
        for (int i = 0; i < 3; ++i) pv[i] = s->pivot[i];
        for (int i = 0; i < 12; ++i) M[i] = s->M[i];
        for (int i = 0; i < 3; ++i) {
            const double rp = (R[3 * i] * pv[0] + R[3 * i + 1] * pv[1]) + R[3 * i + 2] * pv[2];
            const double et = (pv[i] - rp) + delta[3 + i];
            for (int j = 0; j < 4; ++j) {
                double v = (R[3 * i] * M[j] + R[3 * i + 1] * M[4 + j]) + R[3 * i + 2] * M[8 + j];
                if (j == 3) v += et;
                cand[4 * i + j] = v;
                ok = ok && finite(v);
            }
        }
    }
    if (ok) {
        for (int i = 0; i < 12; ++i) s->Mc[i] = cand[i];
        double pc[3];
        apply(s->Mc, s->mean, pc);
        for (int i = 0; i < 3; ++i) s->pivot_c[i] = pc[i];
    } else {
        flag = -1.0;
    }
    // the accepted matrix and its closed-form inverse (R^T, -R^T t)
    for (int i = 0; i < 16; ++i) matrix[i] = s->M[i];
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            inverse[4 * i + j] = s->M[4 * j + i];
            t += s->M[4 * j + i] * s->M[4 * j + 3];
        }
        inverse[4 * i + 3] = -t;
    }
    inverse[12] = inverse[13] = inverse[14] = 0.0;
    inverse[15] = 1.0;
    double* h = history + 4 * (int64_t)it;
    h[0] = s->cost / (double)P;
    h[1] = (double)s->count;
    h[2] = lambda;
    h[3] = flag;
}

}  // namespace

extern "C" size_t ctu_registration_ws_bytes(int64_t P) {
    if (P < 1) return 0;
    return HEAD + (size_t)num_blocks(P) * ROW * sizeof(double);
}

extern "C" int ctu_registration_init(const float* points, int64_t P, const double* init, void* ws, void* stream) {
    CTU_REQUIRE(points && ws, "registration_init: null pointer");
    CTU_REQUIRE(P >= 1, "registration_init: P must be at least 1, got %lld", (long long)P);
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "registration_init: the workspace must be 8-byte aligned");
    reg_init_kernel<<<1, INIT_B, 0, (hipStream_t)stream>>>(points, P, init, (State*)ws);
    CTU_CHECK_LAUNCH("registration_init");
    return CTU_OK;
}

extern "C" int ctu_registration_accumulate(const float* points, int64_t P, const float* field, int D, int H, int W,
                                           const double* spacing, const double* origin, double max_distance, void* ws,
                                           void* stream) {
    CTU_REQUIRE(points && field && ws, "registration_accumulate: null pointer");
    CTU_REQUIRE(P >= 1, "registration_accumulate: P must be at least 1, got %lld", (long long)P);
    CTU_REQUIRE(D >= 2 && H >= 2 && W >= 2 && grid_ok(D, H, W),
                "registration_accumulate: bad field shape %dx%dx%d (every side >= 2, D*H*W < 2^31)", D, H, W);
    CTU_REQUIRE(max_distance >= 0.0, "registration_accumulate: max_distance must be >= 0 (+inf: no bound)");
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "registration_accumulate: the workspace must be 8-byte aligned");
    AccArgs a;
    a.D = D; a.H = H; a.W = W; a.bound = max_distance;
    for (int i = 0; i < 3; ++i) {
        a.sp[i] = spacing ? spacing[i] : 1.0;
        a.org[i] = origin ? origin[i] : 0.0;
    }
    CTU_REQUIRE(steps_ok(a.sp), "registration_accumulate: spacing must be positive and finite");
    CTU_REQUIRE(finite_n(a.org, 3), "registration_accumulate: origin must be finite");
    reg_accumulate_kernel<<<num_blocks(P), RB, 0, (hipStream_t)stream>>>(a, points, P, field, (const State*)ws,
                                                                        (double*)((char*)ws + HEAD));
    CTU_CHECK_LAUNCH("registration_accumulate");
    return CTU_OK;
}

extern "C" int ctu_registration_update(int64_t P, int it, double* matrix, double* inverse, double* history,
                                       int history_rows, void* ws, void* stream) {
    CTU_REQUIRE(matrix && inverse && history && ws, "registration_update: null pointer");
    CTU_REQUIRE(P >= 1, "registration_update: P must be at least 1, got %lld", (long long)P);
    CTU_REQUIRE(it >= 0 && it < history_rows, "registration_update: iteration %d outside the %d history rows", it, history_rows);
    reg_update_kernel<<<1, 64, 0, (hipStream_t)stream>>>(P, num_blocks(P), it, (State*)ws,
                                                         (const double*)((char*)ws + HEAD), matrix, inverse, history);
    CTU_CHECK_LAUNCH("registration_update");
    return CTU_OK;
}

// ---- Similarity (or rigid) registration with the symmetric chamfer cost ---------------------------------------------------
// The same three steps with DOF = 6 or 7 unknowns and a second term: the fixed object's surface points, pulled back through
// the candidate's inverse, against the distance field of the moving object (rule: ctunet_amd/registration.py;
// tests/similarity_ref.py restates it).  New kernels beside the rigid ones, which stay as they are:
//   sim_init_kernel             one block: the mean of the finite moving points, the start state and the adjugate inverse of
//                               init; an init whose determinant is not finite and positive leaves alive = 0.
//   sim_accumulate_kernel<DOF>  one launch over P + Q items (items < P forward, the rest backward), blocks and grid stride as
//                               above; DOF (DOF + 1) / 2 + DOF + 1 sums and two inlier counts per thread, the same fixed-order
//                               reduction, one slab row of SIM_ROW doubles per block.
//   sim_update_kernel<DOF>      one block: the slab in block order (loads ahead as above), the LM step of size DOF, the
//                               candidate E M with E = [L, pivot - L pivot + delta_t], L = exp(delta_s) Rod(delta_w), its
//                               adjugate inverse and determinant; matrix, inverse and the six-column history row.
namespace {

constexpr int SIM_ROW = 40;                     // doubles of a slab row: at most 36 sums, two counts (int64 bits), padding

struct SimState {
    double M[16], Mc[16];                       // accepted matrix, candidate
    double Minv[16], Minv_c[16];                // their inverses (identity while alive == 0)
    double H[28], b[7];                         // of the accepted matrix
    double pivot[3], pivot_c[3], mean[3];
    double cost, lambda, det, det_c;            // det: of the accepted matrix's 3x3 (0 while alive == 0)
    long long count, count_b;                   // inliers of the accepted matrix: both terms, the backward term
    long long alive;                            // 0: init has no usable inverse, every step is refused
};
static_assert(sizeof(SimState) <= HEAD, "registration: the similarity state outgrew the workspace head");

struct SimArgs {
    Grid f, g;                                  // the fixed field's grid, the moving field's
    double bound;                               // +inf: none
};

// inverse (3 rows of 4) and determinant of the affine M by the adjugate: cofactors as differences of products,
// det = (a00 c00 + a01 c01) + a02 c02, entries adj / det, translation -((inv_a0 t_0 + inv_a1 t_1) + inv_a2 t_2);
// true iff the determinant is finite and positive and every entry of the inverse is finite
__device__ bool invert(const double* M, double inv[12], double& det) {
    double c[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[i][j] = M[4 * i1 + j1] * M[4 * i2 + j2] - M[4 * i1 + j2] * M[4 * i2 + j1];
        }
    det = (M[0] * c[0][0] + M[1] * c[0][1]) + M[2] * c[0][2];
    bool ok = finite(det) && det > 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) inv[4 * i + j] = c[j][i] / det;
        inv[4 * i + 3] = -((inv[4 * i] * M[3] + inv[4 * i + 1] * M[7]) + inv[4 * i + 2] * M[11]);
        for (int j = 0; j < 4; ++j) ok = ok && finite(inv[4 * i + j]);
    }
    return ok;
}

__device__ __forceinline__ void set_affine(double* dst, const double* rows, bool identity) {
    for (int i = 0; i < 12; ++i) dst[i] = identity ? (i % 5 == 0 ? 1.0 : 0.0) : rows[i];
    dst[12] = dst[13] = dst[14] = 0.0;
    dst[15] = 1.0;
}

__global__ void __launch_bounds__(INIT_B) sim_init_kernel(const float* __restrict__ pts, int64_t P, const double* __restrict__ init,
                                                          SimState* __restrict__ s) {
    __shared__ double red[INIT_B][4];
    double sum[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    for (int64_t i = threadIdx.x; i < P; i += INIT_B) {
        const double p0 = pts[3 * i], p1 = pts[3 * i + 1], p2 = pts[3 * i + 2];
        if (finite(p0) && finite(p1) && finite(p2)) {
            sum[0] += p0; sum[1] += p1; sum[2] += p2;
            cnt += 1.0;
        }
    }
    red[threadIdx.x][0] = sum[0]; red[threadIdx.x][1] = sum[1]; red[threadIdx.x][2] = sum[2]; red[threadIdx.x][3] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < INIT_B; ++i)
        for (int a = 0; a < 4; ++a) t[a] += red[i][a];
    for (int a = 0; a < 3; ++a) s->mean[a] = t[3] > 0.0 ? t[a] / t[3] : 0.0;
    double m[12];
    for (int i = 0; i < 12; ++i) m[i] = init ? init[i] : (i % 5 == 0 ? 1.0 : 0.0);
    set_affine(s->M, m, false);
    set_affine(s->Mc, m, false);
    double inv[12], det;
    const bool alive = invert(m, inv, det);
    set_affine(s->Minv, inv, !alive);
    set_affine(s->Minv_c, inv, !alive);
    s->det = s->det_c = alive ? det : 0.0;
    s->alive = alive ? 1 : 0;
    for (int i = 0; i < 28; ++i) s->H[i] = 0.0;
    for (int i = 0; i < 7; ++i) s->b[i] = 0.0;
    double pv[3];
    apply(s->Mc, s->mean, pv);
    for (int a = 0; a < 3; ++a) s->pivot[a] = s->pivot_c[a] = pv[a];
    s->cost = __builtin_inf();
    s->lambda = 1e-3;
    s->count = s->count_b = 0;
}

template <int DOF>
__global__ void __launch_bounds__(RB) sim_accumulate_kernel(SimArgs a, const float* __restrict__ pts, int64_t P,
                                                            const float* __restrict__ field, const float* __restrict__ fpts,
                                                            int64_t Q, const float* __restrict__ mfield,
                                                            const SimState* __restrict__ s, double* __restrict__ slab) {
    constexpr int NH = DOF * (DOF + 1) / 2, NA = NH + DOF + 1;                  // upper H, b, cost
    __shared__ double red[NW][NA + 2];
    double M[12], Mi[12], pivot[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = s->Mc[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) Mi[i] = s->Minv_c[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pivot[i] = s->pivot_c[i];
    const bool alive = s->alive != 0;
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    long long count = 0, count_b = 0;
    const double rout = a.bound < __builtin_inf() ? a.bound : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < P + Q; i += (int64_t)gridDim.x * RB) {
        const bool fwd = i < P;
        const float* src = fwd ? pts + 3 * i : fpts + 3 * (i - P);
        const double y[3] = {(double)src[0], (double)src[1], (double)src[2]};
        double x[3], d[3], g[3], v;
        bool inl;
        if (fwd) {
            // q = M_c p against the fixed field; d = q - pivot
            apply(M, y, x);
            inl = sample_inlier(a.f, field, x, a.bound, v, g);
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] = x[r] - pivot[r];
        } else {
            // x = M_c^-1 y against the moving field; the gradient in the fixed frame is -A^-T g; d = y - pivot
            apply(Mi, y, x);
            double gm[3];
            inl = alive && sample_inlier(a.g, mfield, x, a.bound, v, gm);
            if (inl) {
#pragma unroll
                for (int r = 0; r < 3; ++r) g[r] = -((gm[0] * Mi[r] + gm[1] * Mi[4 + r]) + gm[2] * Mi[8 + r]);
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] = y[r] - pivot[r];
        }
        double rr = rout;
        if (inl) {
            double J[DOF];
            J[0] = d[1] * g[2] - d[2] * g[1];
            J[1] = d[2] * g[0] - d[0] * g[2];
            J[2] = d[0] * g[1] - d[1] * g[0];
            J[3] = g[0]; J[4] = g[1]; J[5] = g[2];
            if (DOF == 7) J[DOF - 1] = (d[0] * g[0] + d[1] * g[1]) + d[2] * g[2];
            int k = 0;
#pragma unroll
            for (int r = 0; r < DOF; ++r)
#pragma unroll
                for (int c = r; c < DOF; ++c) acc[k++] += J[r] * J[c];
#pragma unroll
            for (int r = 0; r < DOF; ++r) acc[NH + r] += J[r] * v;
            rr = v;
            ++count;
            if (!fwd) ++count_b;
        }
        acc[NA - 1] += rr * rr;
    }
    // lanes of a wave in xor order, then the waves in order
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        count += __shfl_xor(count, o);
        count_b += __shfl_xor(count_b, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) red[wave][i] = acc[i];
        red[wave][NA] = __longlong_as_double(count);
        red[wave][NA + 1] = __longlong_as_double(count_b);
    }
    __syncthreads();
    if (threadIdx.x < SIM_ROW) {
        double* row = slab + (int64_t)blockIdx.x * SIM_ROW;
        const int e = threadIdx.x;
        if (e < NA) {
            double t = red[0][e];
            for (int w = 1; w < NW; ++w) t += red[w][e];
            row[e] = t;
        } else if (e < NA + 2) {
            long long t = 0;
            for (int w = 0; w < NW; ++w) t += __double_as_longlong(red[w][e]);
            row[e] = __longlong_as_double(t);
        } else {
            row[e] = 0.0;
        }
    }
}

// delta of (H + lambda diag(H) + 1e-12 I) delta = -b for N unknowns; false: a pivot that is not positive, or a result that
// is not finite
template <int N>
__device__ bool solve_n(const double* Hu, const double* b, double lambda, double* x) {
    double A[N][N], L[N][N];
    int k = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i; j < N; ++j) A[i][j] = A[j][i] = Hu[k++];
    for (int i = 0; i < N; ++i) A[i][i] = A[i][i] + lambda * A[i][i] + 1e-12;
    for (int j = 0; j < N; ++j) {
        double sdiag = A[j][j];
        for (int c = 0; c < j; ++c) sdiag -= L[j][c] * L[j][c];
        if (!(sdiag > 0.0) || !finite(sdiag)) return false;
        L[j][j] = sqrt(sdiag);
        for (int i = j + 1; i < N; ++i) {
            double t = A[i][j];
            for (int c = 0; c < j; ++c) t -= L[i][c] * L[j][c];
            L[i][j] = t / L[j][j];
        }
    }
    double y[N];
    for (int i = 0; i < N; ++i) {
        double t = -b[i];
        for (int c = 0; c < i; ++c) t -= L[i][c] * y[c];
        y[i] = t / L[i][i];
    }
    for (int i = N - 1; i >= 0; --i) {
        double t = y[i];
        for (int c = i + 1; c < N; ++c) t -= L[c][i] * x[c];
        x[i] = t / L[i][i];
    }
    for (int i = 0; i < N; ++i)
        if (!finite(x[i])) return false;
    return true;
}

template <int DOF>
__global__ void __launch_bounds__(64) sim_update_kernel(int64_t n_items, int nb, int it, SimState* __restrict__ s,
                                                        const double* __restrict__ slab, double* __restrict__ matrix,
                                                        double* __restrict__ inverse, double* __restrict__ history) {
    constexpr int NH = DOF * (DOF + 1) / 2, NA = NH + DOF + 1;
    __shared__ double tot[SIM_ROW];
    const int e = threadIdx.x;
    if (e < NA + 2) {
        // rows in block order, SUM_AHEAD loads issued before their additions (the order of the sum is unchanged)
        double t = 0.0;
        long long n = 0;
        int r = 0;
        for (; r + SUM_AHEAD <= nb; r += SUM_AHEAD) {
            double v[SUM_AHEAD];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) v[k] = slab[(int64_t)(r + k) * SIM_ROW + e];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) {
                t += v[k];
                n += __double_as_longlong(v[k]);
            }
        }
        for (; r < nb; ++r) {
            const double v = slab[(int64_t)r * SIM_ROW + e];
            t += v;
            n += __double_as_longlong(v);
        }
        tot[e] = e < NA ? t : __longlong_as_double(n);
    }
    __syncthreads();
    if (e != 0) return;
    const double cost_c = tot[NA - 1];
    const bool accepted = cost_c < s->cost;                        // NaN: rejected
    double lambda = s->lambda;
    if (accepted) {
        for (int i = 0; i < 16; ++i) s->M[i] = s->Mc[i];
        for (int i = 0; i < 16; ++i) s->Minv[i] = s->Minv_c[i];
        for (int i = 0; i < NH; ++i) s->H[i] = tot[i];
        for (int i = 0; i < DOF; ++i) s->b[i] = tot[NH + i];
        for (int i = 0; i < 3; ++i) s->pivot[i] = s->pivot_c[i];
        s->det = s->det_c;
        s->cost = cost_c;
        s->count = __double_as_longlong(tot[NA]);
        s->count_b = __double_as_longlong(tot[NA + 1]);
        lambda = fmax(lambda / 3.0, 1e-9);
    } else {
        lambda = fmin(lambda * 10.0, 1e9);
    }
    s->lambda = lambda;
    double flag = accepted ? 1.0 : 0.0;
    double delta[DOF], H[NH], b[DOF];
    for (int i = 0; i < NH; ++i) H[i] = s->H[i];
    for (int i = 0; i < DOF; ++i) b[i] = s->b[i];
    bool ok = s->alive != 0 && s->count >= DOF && solve_n<DOF>(H, b, lambda, delta);
    double cand[12], cinv[12], cdet = 0.0;
    if (ok) {
        double L[9], pv[3], M[12];
        rodrigues(delta, L);
        if (DOF == 7) {
            const double es = exp(delta[DOF - 1]);
            for (int i = 0; i < 9; ++i) L[i] = es * L[i];
        }
        for (int i = 0; i < 3; ++i) pv[i] = s->pivot[i];
        for (int i = 0; i < 12; ++i) M[i] = s->M[i];
        for (int i = 0; i < 3; ++i) {
            const double lp = (L[3 * i] * pv[0] + L[3 * i + 1] * pv[1]) + L[3 * i + 2] * pv[2];
            const double et = (pv[i] - lp) + delta[3 + i];
            for (int j = 0; j < 4; ++j) {
                double v = (L[3 * i] * M[j] + L[3 * i + 1] * M[4 + j]) + L[3 * i + 2] * M[8 + j];
                if (j == 3) v += et;
                cand[4 * i + j] = v;
                ok = ok && finite(v);
            }
        }
        ok = ok && invert(cand, cinv, cdet);
    }
    if (ok) {
        for (int i = 0; i < 12; ++i) s->Mc[i] = cand[i];
        for (int i = 0; i < 12; ++i) s->Minv_c[i] = cinv[i];
        s->det_c = cdet;
        double pc[3];
        apply(s->Mc, s->mean, pc);
        for (int i = 0; i < 3; ++i) s->pivot_c[i] = pc[i];
    } else {
        flag = -1.0;
    }
    for (int i = 0; i < 16; ++i) matrix[i] = s->M[i];
    for (int i = 0; i < 16; ++i) inverse[i] = s->Minv[i];
    double* h = history + 6 * (int64_t)it;
    h[0] = s->cost / (double)n_items;
    h[1] = (double)s->count;
    h[2] = lambda;
    h[3] = flag;
    h[4] = (double)s->count_b;
    h[5] = cbrt(s->det);
}

bool sim_grid(Grid& g, int D, int H, int W, const double* spacing, const double* origin) {
    g.n[0] = D; g.n[1] = H; g.n[2] = W;
    for (int i = 0; i < 3; ++i) {
        g.sp[i] = spacing ? spacing[i] : 1.0;
        g.org[i] = origin ? origin[i] : 0.0;
    }
    return steps_ok(g.sp) && finite_n(g.org, 3);
}

}  // namespace

extern "C" size_t ctu_similarity_ws_bytes(int64_t P, int64_t Q) {
    if (P < 1 || Q < 0) return 0;
    return HEAD + (size_t)num_blocks(P + Q) * SIM_ROW * sizeof(double);
}

extern "C" int ctu_similarity_init(const float* points, int64_t P, const double* init, void* ws, void* stream) {
    CTU_REQUIRE(points && ws, "similarity_init: null pointer");
    CTU_REQUIRE(P >= 1, "similarity_init: P must be at least 1, got %lld", (long long)P);
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "similarity_init: the workspace must be 8-byte aligned");
    sim_init_kernel<<<1, INIT_B, 0, (hipStream_t)stream>>>(points, P, init, (SimState*)ws);
    CTU_CHECK_LAUNCH("similarity_init");
    return CTU_OK;
}

extern "C" int ctu_similarity_accumulate(int dof, const float* points, int64_t P, const float* field, int D, int H, int W,
                                         const double* spacing, const double* origin, const float* fixed_points, int64_t Q,
                                         const float* moving_field, int d, int h, int w, const double* moving_spacing,
                                         const double* moving_origin, double max_distance, void* ws, void* stream) {
    CTU_REQUIRE(dof == 6 || dof == 7, "similarity_accumulate: dof must be 6 or 7, got %d", dof);
    CTU_REQUIRE(points && field && ws, "similarity_accumulate: null pointer");
    CTU_REQUIRE(P >= 1 && Q >= 0, "similarity_accumulate: P must be at least 1 and Q at least 0, got %lld and %lld", (long long)P,
                (long long)Q);
    CTU_REQUIRE(D >= 2 && H >= 2 && W >= 2 && grid_ok(D, H, W),
                "similarity_accumulate: bad field shape %dx%dx%d (every side >= 2, D*H*W < 2^31)", D, H, W);
    CTU_REQUIRE(max_distance >= 0.0, "similarity_accumulate: max_distance must be >= 0 (+inf: no bound)");
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "similarity_accumulate: the workspace must be 8-byte aligned");
    SimArgs a;
    a.bound = max_distance;
    CTU_REQUIRE(sim_grid(a.f, D, H, W, spacing, origin), "similarity_accumulate: spacing must be positive and finite, origin finite");
    if (Q > 0) {
        CTU_REQUIRE(fixed_points && moving_field, "similarity_accumulate: Q > 0 needs fixed_points and moving_field");
        CTU_REQUIRE(d >= 2 && h >= 2 && w >= 2 && grid_ok(d, h, w),
                    "similarity_accumulate: bad moving field shape %dx%dx%d (every side >= 2, d*h*w < 2^31)", d, h, w);
        CTU_REQUIRE(sim_grid(a.g, d, h, w, moving_spacing, moving_origin),
                    "similarity_accumulate: moving_spacing must be positive and finite, moving_origin finite");
    } else {
        a.g = a.f;                                                              // never read: no item is a backward one
    }
    double* slab = (double*)((char*)ws + HEAD);
    const int nb = num_blocks(P + Q);
    if (dof == 7)
        sim_accumulate_kernel<7><<<nb, RB, 0, (hipStream_t)stream>>>(a, points, P, field, fixed_points, Q, moving_field,
                                                                     (const SimState*)ws, slab);
    else
        sim_accumulate_kernel<6><<<nb, RB, 0, (hipStream_t)stream>>>(a, points, P, field, fixed_points, Q, moving_field,
                                                                     (const SimState*)ws, slab);
    CTU_CHECK_LAUNCH("similarity_accumulate");
    return CTU_OK;
}

extern "C" int ctu_similarity_update(int dof, int64_t P, int64_t Q, int it, double* matrix, double* inverse, double* history,
                                     int history_rows, void* ws, void* stream) {
    CTU_REQUIRE(dof == 6 || dof == 7, "similarity_update: dof must be 6 or 7, got %d", dof);
    CTU_REQUIRE(matrix && inverse && history && ws, "similarity_update: null pointer");
    CTU_REQUIRE(P >= 1 && Q >= 0, "similarity_update: P must be at least 1 and Q at least 0, got %lld and %lld", (long long)P,
                (long long)Q);
    CTU_REQUIRE(it >= 0 && it < history_rows, "similarity_update: iteration %d outside the %d history rows", it, history_rows);
    const double* slab = (const double*)((char*)ws + HEAD);
    const int nb = num_blocks(P + Q);
    if (dof == 7)
        sim_update_kernel<7><<<1, 64, 0, (hipStream_t)stream>>>(P + Q, nb, it, (SimState*)ws, slab, matrix, inverse, history);
    else
        sim_update_kernel<6><<<1, 64, 0, (hipStream_t)stream>>>(P + Q, nb, it, (SimState*)ws, slab, matrix, inverse, history);
    CTU_CHECK_LAUNCH("similarity_update");
    return CTU_OK;
}
