// Registration of a point set to a distance field by Levenberg-Marquardt chamfer matching, gfx950 (rule:
// ctunet_amd/registration.py; tests/registration_ref.py and tests/similarity_ref.py restate it in numpy float64).
//
// One kernel family, all float64, contraction off for the file so that a point's terms are the restatements' bit for bit.
// A compile-time trait names the member: Rigid (ctu_registration_*: 6 unknowns, the directed cost, slab rows of 32 doubles,
// 4 history columns) and Sim<6> / Sim<7> (ctu_similarity_*: 6 or 7 unknowns, rows of 40 doubles, 6 columns, symmetric).  A
// symmetric member adds the backward term -- the fixed object's surface points, pulled back through the candidate's inverse,
// against the distance field of the moving object -- and with it the inverses, determinants, `alive` and the backward count
// of its state; `if constexpr (F::symmetric)` compiles all of that out of the rigid member.
//   init_kernel<F>        one block: the mean of the finite moving points (fixed order) and the start state (M = M_c = init,
//                         cost = +inf, lambda = 1e-3) into the workspace; once per registration.  Symmetric: also the adjugate
//                         inverse of init; an init whose determinant is not finite and positive leaves alive = 0.
//   accumulate_kernel<F>  a thread per item with a grid stride, at most CTU_REG_MAX_BLOCKS blocks of 256, over P + Q items
//                         (items < P forward, the rest backward; Q = 0 for Rigid): samples the field at M_c p (at M_c^-1 y),
//                         forms the residual and the Jacobian row about the candidate's pivot and adds the DOF (DOF + 1) / 2
//                         entries of upper H, the DOF of b and the cost into registers, plus the inlier counts; a fixed-order
//                         wave reduction (xor shuffles), then LDS across the 4 waves, then ONE slab row per block.  No float
//                         atomics: two calls are bit-equal.
//   update_kernel<F>      one block: sums the slab in block order, then one thread compares the costs, accepts or rejects the
//                         candidate, adapts lambda, solves the damped DOF x DOF system by Cholesky and forms the next candidate
//                         E M, E = [L, pivot - L pivot + delta_t], L = Rod(delta_w) (DOF 7: exp(delta_s) Rod(delta_w)); writes
//                         the state, matrix, inverse and the iteration's history row.  Rigid: the closed-form inverse
//                         (R^T, -R^T t).  Symmetric: the adjugate inverse, and a candidate without a usable one is refused.
// Everything that changes between iterations lives in the workspace, so a registration is 1 + 2 (iterations + 1) launches
// on one stream without a host synchronisation, and it can be captured into a graph.
// Every field read is guarded by the comparison that declares the point inside the field (NaN fails it).
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
constexpr int MAX_BLOCKS = CTU_REG_MAX_BLOCKS;
constexpr int INIT_B = 1024;
constexpr int SUM_AHEAD = 16;                   // slab rows the update kernel loads ahead of their additions
constexpr size_t HEAD = 1024;                   // bytes of the workspace head (the state); the slab follows

// the two workspace heads, in doubles (layouts: include/ctunet_hip.h)
struct RigidState {
    double M[16], Mc[16];                       // accepted matrix, candidate
    double H[21], b[6];                         // of the accepted matrix
    double pivot[3], pivot_c[3], mean[3];
    double cost, lambda;
    long long count;                            // inliers of the accepted matrix
};
struct SimState {
    double M[16], Mc[16];                       // accepted matrix, candidate
    double Minv[16], Minv_c[16];                // their inverses (identity while alive == 0)
    double H[28], b[7];                         // of the accepted matrix
    double pivot[3], pivot_c[3], mean[3];
    double cost, lambda, det, det_c;            // det: of the accepted matrix's 3x3 (0 while alive == 0)
    long long count, count_b;                   // inliers of the accepted matrix: both terms, the backward term
    long long alive;                            // 0: init has no usable inverse, every step is refused
};
static_assert(sizeof(RigidState) <= HEAD && sizeof(SimState) <= HEAD, "registration: a state outgrew the workspace head");

// the family members: unknowns, state, doubles of a slab row (NA sums, NC counts as int64 bits, padding), history columns
struct Rigid {
    typedef RigidState State;
    static constexpr int DOF = 6, ROW = 32, HIST = 4;
    static constexpr bool symmetric = false;
};
template <int N>
struct Sim {
    typedef SimState State;
    static constexpr int DOF = N, ROW = 40, HIST = 6;
    static constexpr bool symmetric = true;
};
static_assert(CTU_REG_MIN_INLIERS == Rigid::DOF, "registration: the rigid minimum of inliers is its number of unknowns");

struct AccArgs {
    Grid f, g;                                  // the fixed field's grid, the moving field's (backward items only)
    double bound;                               // +inf: none
};

__host__ __device__ inline int num_blocks(int64_t items) {
    const int64_t nb = (items + RB - 1) / RB;
    return (int)(nb < 1 ? 1 : (nb > MAX_BLOCKS ? MAX_BLOCKS : nb));
}

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

// the state is sized for the family's largest member, so the symmetric family starts as Sim<7> whatever dof follows
template <class F>
__global__ void __launch_bounds__(INIT_B) init_kernel(const float* __restrict__ pts, int64_t P, const double* __restrict__ init,
                                                      typename F::State* __restrict__ s) {
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
    if constexpr (F::symmetric) {
        double inv[12], det;
        const bool alive = invert(m, inv, det);
        set_affine(s->Minv, inv, !alive);
        set_affine(s->Minv_c, inv, !alive);
        s->det = s->det_c = alive ? det : 0.0;
        s->alive = alive ? 1 : 0;
        s->count_b = 0;
    }
    for (int i = 0; i < F::DOF * (F::DOF + 1) / 2; ++i) s->H[i] = 0.0;
    for (int i = 0; i < F::DOF; ++i) s->b[i] = 0.0;
    double pv[3];
    apply(s->Mc, s->mean, pv);
    for (int a = 0; a < 3; ++a) s->pivot[a] = s->pivot_c[a] = pv[a];
    s->cost = __builtin_inf();
    s->lambda = 1e-3;
    s->count = 0;
}

template <class F>
__global__ void __launch_bounds__(RB) accumulate_kernel(AccArgs a, const float* __restrict__ pts, int64_t P,
                                                        const float* __restrict__ field, const float* __restrict__ fpts,
                                                        int64_t Q, const float* __restrict__ mfield,
                                                        const typename F::State* __restrict__ s, double* __restrict__ slab) {
    constexpr int DOF = F::DOF, NH = DOF * (DOF + 1) / 2, NA = NH + DOF + 1;    // upper H, b, cost
    constexpr int NC = F::symmetric ? 2 : 1;                                    // inliers of both terms, of the backward term
    __shared__ double red[NW][NA + NC];
    double M[12], pivot[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = s->Mc[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pivot[i] = s->pivot_c[i];
    [[maybe_unused]] double Mi[12];                                             // the symmetric family's alone
    [[maybe_unused]] bool alive = false;
    if constexpr (F::symmetric) {
#pragma unroll
        for (int i = 0; i < 12; ++i) Mi[i] = s->Minv_c[i];
        alive = s->alive != 0;
    }
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    long long count[NC] = {};
    const double rout = a.bound < __builtin_inf() ? a.bound : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < P + Q; i += (int64_t)gridDim.x * RB) {
        const bool fwd = !F::symmetric || i < P;
        const float* src = fwd ? pts + 3 * i : fpts + 3 * (i - P);
        const double y[3] = {(double)src[0], (double)src[1], (double)src[2]};
        double x[3], d[3], g[3], v;
        bool inl = false;
        if (fwd) {
            // q = M_c p against the fixed field; d = q - pivot
            apply(M, y, x);
            inl = sample_inlier(a.f, field, x, a.bound, v, g);
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] = x[r] - pivot[r];
        } else if constexpr (F::symmetric) {
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
            if constexpr (DOF == 7) J[6] = (d[0] * g[0] + d[1] * g[1]) + d[2] * g[2];
            int k = 0;
#pragma unroll
            for (int r = 0; r < DOF; ++r)
#pragma unroll
                for (int c = r; c < DOF; ++c) acc[k++] += J[r] * J[c];
#pragma unroll
            for (int r = 0; r < DOF; ++r) acc[NH + r] += J[r] * v;
            rr = v;
            ++count[0];
            if constexpr (F::symmetric)
                if (!fwd) ++count[1];
        }
        acc[NA - 1] += rr * rr;
    }
    // lanes of a wave in xor order, then the waves in order
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < NC; ++i) count[i] += __shfl_xor(count[i], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) red[wave][i] = acc[i];
#pragma unroll
        for (int i = 0; i < NC; ++i) red[wave][NA + i] = __longlong_as_double(count[i]);
    }
    __syncthreads();
    if (threadIdx.x < F::ROW) {
        double* row = slab + (int64_t)blockIdx.x * F::ROW;
        const int e = threadIdx.x;
        if (e < NA) {
            double t = red[0][e];
            for (int w = 1; w < NW; ++w) t += red[w][e];
            row[e] = t;
        } else if (e < NA + NC) {
            long long t = 0;
            for (int w = 0; w < NW; ++w) t += __double_as_longlong(red[w][e]);
            row[e] = __longlong_as_double(t);
        } else {
            row[e] = 0.0;
        }
    }
}

template <class F>
__global__ void __launch_bounds__(64) update_kernel(int64_t n_items, int nb, int it, typename F::State* __restrict__ s,
                                                    const double* __restrict__ slab, double* __restrict__ matrix,
                                                    double* __restrict__ inverse, double* __restrict__ history) {
    constexpr int DOF = F::DOF, NH = DOF * (DOF + 1) / 2, NA = NH + DOF + 1, NC = F::symmetric ? 2 : 1;
    __shared__ double tot[F::ROW];
    const int e = threadIdx.x;
    if (e < NA + NC) {
        // rows in block order; SUM_AHEAD loads are issued before their additions, so the order of the sum is unchanged and
        // a row costs an addition, not a round trip to memory
        double t = 0.0;
        long long n = 0;
        int r = 0;
        for (; r + SUM_AHEAD <= nb; r += SUM_AHEAD) {
            double v[SUM_AHEAD];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) v[k] = slab[(int64_t)(r + k) * F::ROW + e];
#pragma unroll
            for (int k = 0; k < SUM_AHEAD; ++k) {
                t += v[k];
                n += __double_as_longlong(v[k]);
            }
        }
        for (; r < nb; ++r) {
            const double v = slab[(int64_t)r * F::ROW + e];
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
        for (int i = 0; i < NH; ++i) s->H[i] = tot[i];
        for (int i = 0; i < DOF; ++i) s->b[i] = tot[NH + i];
        for (int i = 0; i < 3; ++i) s->pivot[i] = s->pivot_c[i];
        s->cost = cost_c;
        s->count = __double_as_longlong(tot[NA]);
        if constexpr (F::symmetric) {
            for (int i = 0; i < 16; ++i) s->Minv[i] = s->Minv_c[i];
            s->det = s->det_c;
            s->count_b = __double_as_longlong(tot[NA + 1]);
        }
        lambda = fmax(lambda / 3.0, 1e-9);
    } else {
        lambda = fmin(lambda * 10.0, 1e9);
    }
    s->lambda = lambda;
    double flag = accepted ? 1.0 : 0.0;
    double delta[DOF], H[NH], b[DOF];
    for (int i = 0; i < NH; ++i) H[i] = s->H[i];
    for (int i = 0; i < DOF; ++i) b[i] = s->b[i];
    bool ok = s->count >= DOF;                                     // fewer inliers than unknowns: only the damping would solve it
    if constexpr (F::symmetric) ok = ok && s->alive != 0;
    ok = ok && solve_n<DOF>(H, b, lambda, delta);
    double cand[12];
    [[maybe_unused]] double cinv[12], cdet = 0.0;                  // the symmetric family's alone
    if (ok) {
        double L[9], pv[3], M[12];
        rodrigues(delta, L);
        if constexpr (DOF == 7) {
            const double es = exp(delta[6]);
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
        if constexpr (F::symmetric) ok = ok && invert(cand, cinv, cdet);
    }
    if (ok) {
        for (int i = 0; i < 12; ++i) s->Mc[i] = cand[i];
        if constexpr (F::symmetric) {
            for (int i = 0; i < 12; ++i) s->Minv_c[i] = cinv[i];
            s->det_c = cdet;
        }
        double pc[3];
        apply(s->Mc, s->mean, pc);
        for (int i = 0; i < 3; ++i) s->pivot_c[i] = pc[i];
    } else {
        flag = -1.0;
    }
    for (int i = 0; i < 16; ++i) matrix[i] = s->M[i];
    if constexpr (F::symmetric) {
        for (int i = 0; i < 16; ++i) inverse[i] = s->Minv[i];
    } else {
        // the closed form (R^T, -R^T t); the translation's three products are added in order from 0
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
    }
    double* h = history + F::HIST * (int64_t)it;
    h[0] = s->cost / (double)n_items;
    h[1] = (double)s->count;
    h[2] = lambda;
    h[3] = flag;
    if constexpr (F::symmetric) {
        h[4] = (double)s->count_b;
        h[5] = cbrt(s->det);
    }
}

// ---- the entry points: one checker and launcher per step, `who` in front of every error text ----------------------------------
template <class F>
size_t ws_bytes(int64_t items) {
    return HEAD + (size_t)num_blocks(items) * F::ROW * sizeof(double);
}

// a field's grid from an entry point's arguments (NULL spacing: 1, NULL origin: 0)
Grid field_grid(int D, int H, int W, const double* spacing, const double* origin) {
    Grid g;
    g.n[0] = D; g.n[1] = H; g.n[2] = W;
    for (int i = 0; i < 3; ++i) {
        g.sp[i] = spacing ? spacing[i] : 1.0;
        g.org[i] = origin ? origin[i] : 0.0;
    }
    return g;
}

bool shape_ok(const Grid& g) { return g.n[0] >= 2 && g.n[1] >= 2 && g.n[2] >= 2 && grid_ok(g.n[0], g.n[1], g.n[2]); }

template <class F>
int check_counts(const char* who, int64_t P, int64_t Q) {
    if constexpr (F::symmetric)
        CTU_REQUIRE(P >= 1 && Q >= 0, "%s: P must be at least 1 and Q at least 0, got %lld and %lld", who, (long long)P,
                    (long long)Q);
    else
        CTU_REQUIRE(P >= 1, "%s: P must be at least 1, got %lld", who, (long long)P);
    return CTU_OK;
}

template <class F>
int run_init(const char* who, const float* points, int64_t P, const double* init, void* ws, void* stream) {
    CTU_REQUIRE(points && ws, "%s: null pointer", who);
    CTU_REQUIRE(P >= 1, "%s: P must be at least 1, got %lld", who, (long long)P);
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    init_kernel<F><<<1, INIT_B, 0, (hipStream_t)stream>>>(points, P, init, (typename F::State*)ws);
    CTU_CHECK_LAUNCH(who);
    return CTU_OK;
}

template <class F>
int run_accumulate(const char* who, const float* points, int64_t P, const float* field, int D, int H, int W,
                   const double* spacing, const double* origin, const float* fixed_points, int64_t Q, const float* moving_field,
                   int d, int h, int w, const double* moving_spacing, const double* moving_origin, double max_distance, void* ws,
                   void* stream) {
    CTU_REQUIRE(points && field && ws, "%s: null pointer", who);
    if (const int rc = check_counts<F>(who, P, Q)) return rc;
    AccArgs a;
    a.f = a.g = field_grid(D, H, W, spacing, origin);                           // g: never read unless Q > 0
    a.bound = max_distance;
    CTU_REQUIRE(shape_ok(a.f), "%s: bad field shape %dx%dx%d (every side >= 2, D*H*W < 2^31)", who, D, H, W);
    CTU_REQUIRE(max_distance >= 0.0, "%s: max_distance must be >= 0 (+inf: no bound)", who);
    CTU_REQUIRE((uintptr_t)ws % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    if constexpr (F::symmetric) {
        CTU_REQUIRE(steps_ok(a.f.sp) && finite_n(a.f.org, 3), "%s: spacing must be positive and finite, origin finite", who);
        if (Q > 0) {
            CTU_REQUIRE(fixed_points && moving_field, "%s: Q > 0 needs fixed_points and moving_field", who);
            a.g = field_grid(d, h, w, moving_spacing, moving_origin);
            CTU_REQUIRE(shape_ok(a.g), "%s: bad moving field shape %dx%dx%d (every side >= 2, d*h*w < 2^31)", who, d, h, w);
            CTU_REQUIRE(steps_ok(a.g.sp) && finite_n(a.g.org, 3),
                        "%s: moving_spacing must be positive and finite, moving_origin finite", who);
        }
    } else {
        CTU_REQUIRE(steps_ok(a.f.sp), "%s: spacing must be positive and finite", who);
        CTU_REQUIRE(finite_n(a.f.org, 3), "%s: origin must be finite", who);
    }
    accumulate_kernel<F><<<num_blocks(P + Q), RB, 0, (hipStream_t)stream>>>(
        a, points, P, field, fixed_points, Q, moving_field, (const typename F::State*)ws, (double*)((char*)ws + HEAD));
    CTU_CHECK_LAUNCH(who);
    return CTU_OK;
}

template <class F>
int run_update(const char* who, int64_t P, int64_t Q, int it, double* matrix, double* inverse, double* history,
               int history_rows, void* ws, void* stream) {
    CTU_REQUIRE(matrix && inverse && history && ws, "%s: null pointer", who);
    if (const int rc = check_counts<F>(who, P, Q)) return rc;
    CTU_REQUIRE(it >= 0 && it < history_rows, "%s: iteration %d outside the %d history rows", who, it, history_rows);
    update_kernel<F><<<1, 64, 0, (hipStream_t)stream>>>(P + Q, num_blocks(P + Q), it, (typename F::State*)ws,
                                                        (const double*)((char*)ws + HEAD), matrix, inverse, history);
    CTU_CHECK_LAUNCH(who);
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_registration_ws_bytes(int64_t P) { return P < 1 ? 0 : ws_bytes<Rigid>(P); }

extern "C" int ctu_registration_init(const float* points, int64_t P, const double* init, void* ws, void* stream) {
    return run_init<Rigid>("registration_init", points, P, init, ws, stream);
}

extern "C" int ctu_registration_accumulate(const float* points, int64_t P, const float* field, int D, int H, int W,
                                           const double* spacing, const double* origin, double max_distance, void* ws,
                                           void* stream) {
    return run_accumulate<Rigid>("registration_accumulate", points, P, field, D, H, W, spacing, origin, nullptr, 0, nullptr, 0, 0,
                                 0, nullptr, nullptr, max_distance, ws, stream);
}

extern "C" int ctu_registration_update(int64_t P, int it, double* matrix, double* inverse, double* history,
                                       int history_rows, void* ws, void* stream) {
    return run_update<Rigid>("registration_update", P, 0, it, matrix, inverse, history, history_rows, ws, stream);
}

extern "C" size_t ctu_similarity_ws_bytes(int64_t P, int64_t Q) { return P < 1 || Q < 0 ? 0 : ws_bytes<Sim<7>>(P + Q); }

extern "C" int ctu_similarity_init(const float* points, int64_t P, const double* init, void* ws, void* stream) {
    return run_init<Sim<7>>("similarity_init", points, P, init, ws, stream);
}

extern "C" int ctu_similarity_accumulate(int dof, const float* points, int64_t P, const float* field, int D, int H, int W,
                                         const double* spacing, const double* origin, const float* fixed_points, int64_t Q,
                                         const float* moving_field, int d, int h, int w, const double* moving_spacing,
                                         const double* moving_origin, double max_distance, void* ws, void* stream) {
    CTU_REQUIRE(dof == 6 || dof == 7, "similarity_accumulate: dof must be 6 or 7, got %d", dof);
    return (dof == 7 ? run_accumulate<Sim<7>> : run_accumulate<Sim<6>>)(
        "similarity_accumulate", points, P, field, D, H, W, spacing, origin, fixed_points, Q, moving_field, d, h, w,
        moving_spacing, moving_origin, max_distance, ws, stream);
}

extern "C" int ctu_similarity_update(int dof, int64_t P, int64_t Q, int it, double* matrix, double* inverse, double* history,
                                     int history_rows, void* ws, void* stream) {
    CTU_REQUIRE(dof == 6 || dof == 7, "similarity_update: dof must be 6 or 7, got %d", dof);
    return (dof == 7 ? run_update<Sim<7>> : run_update<Sim<6>>)("similarity_update", P, Q, it, matrix, inverse, history,
                                                                history_rows, ws, stream);
}
