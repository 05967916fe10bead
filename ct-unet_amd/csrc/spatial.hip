// On-device random spatial augmentation, gfx950: a random flip, a cubic B-spline elastic deformation and a random affine
// map applied to a batch of volumes in ONE nearest-neighbour gather pass (rule: ctunet_amd/transforms.py, "RandomSpatial";
// tests/spatial_ref.py restates it).  Two launches, no atomics, no host synchronisation, so a call replays inside a graph:
//   ctu_spatial_draw  one block per sample: the per-sample record (flags, scalars, the 3x4 matrix M) and the control
//                     displacements [3][Gz][Gy][Gx] from Philox4x32-10 (philox.h) and the instance's DEVICE sample counter
//   ctu_spatial_warp  out[n][c][o] = in[n][c][k(o)] for all C channels of a sample, k from the record and the control grid
// The warp kernel's output is tiled by chunk_tile.h: a block of 256 threads owns 4 planes x 4 rows x 16 chunks, a chunk
// being the 16 bytes one thread stores on the 16-byte grid of its output row; a later channel's rows may sit on another
// grid, so its store tests the address.  The sample's control grid (3 G^3 doubles, 8.2 KB at G = 7, 41.5 KB at G = 12) is
// staged in LDS once per block, and only when the sample's elastic flag is set -- a branch that is uniform over the block.
// The source index of a voxel is computed once and reused for every channel.  Every read of the volume sits behind the
// comparison that declares its index inside it, and every read of the LDS grid uses an index clamped to the grid, so no
// record or grid content (NaN and infinite entries included) can take a read outside either.
// Coordinates: float64, every operation rounded on its own (contraction is off for the file).
//
// Replaces: the flip / elastic / affine steps of ctunet/pytorch/transforms.py:173-228 (cranioplasty_transform), which the
//           reference takes from torchio on the host; the rule here is the port's own.
#include "chunk_tile.h"
#include "common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_tile;
using namespace ctu_rng;

constexpr int REC = CTU_SPATIAL_RECORD;
constexpr int GMIN = CTU_SPATIAL_MIN_POINTS, GMAX = CTU_SPATIAL_MAX_POINTS;
constexpr int MAXC = 64;                        // channels per sample

// (2 u - 1) a
__device__ __forceinline__ double sym(uint32_t r, double a) { return (2.0 * unif_f64(r) - 1.0) * a; }

// ---------------------------------------------------------------------------------------------------------------- draw
struct DrawArgs {
    int n[3], G[3];
    int flip_mask, locked;
    double sp[3];
    double p_flip, p_affine, p_elastic;
    double s_lo, s_hi;
    double deg[3], tr[3], md[3];
    const int64_t* seq;
    uint32_t k0, k1;
    double* record;
    double* control;
};

// C = A B, each entry ((a0 b0 + a1 b1) + a2 b2)
__device__ __forceinline__ void mat3(const double A[9], const double B[9], double C[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// one block per sample; the threads share the control points, thread 0 also writes the record (layout: ctunet_hip.h)
__global__ void __launch_bounds__(SB) spatial_draw_kernel(DrawArgs a) {
    const int n = blockIdx.x;
    const int64_t seq = a.seq[0] + n;
    const int gz = a.G[0], gy = a.G[1], gx = a.G[2];
    const int g3 = gz * gy * gx;
    double* ctl = a.control + (int64_t)n * 3 * g3;
    for (int i = threadIdx.x; i < g3; i += SB) {
        const int ix = i % gx, iy = (i / gx) % gy, iz = i / (gx * gy);
        const bool free_pt = iz >= a.locked && iz < gz - a.locked && iy >= a.locked && iy < gy - a.locked &&
                             ix >= a.locked && ix < gx - a.locked;
        const uint4 r = philox_seq((uint32_t)i, 1, seq, a.k0, a.k1);
        ctl[i] = free_pt ? sym(r.x, a.md[0]) : 0.0;
        ctl[g3 + i] = free_pt ? sym(r.y, a.md[1]) : 0.0;
        ctl[2 * g3 + i] = free_pt ? sym(r.z, a.md[2]) : 0.0;
    }
    if (threadIdx.x != 0) return;
    double* rec = a.record + (int64_t)n * REC;
    const uint4 r0 = philox_seq(0, 0, seq, a.k0, a.k1), r1 = philox_seq(1, 0, seq, a.k0, a.k1);
    const uint4 r2 = philox_seq(2, 0, seq, a.k0, a.k1), r3 = philox_seq(3, 0, seq, a.k0, a.k1);
    const uint32_t fl[3] = {r0.x, r0.y, r0.z}, sc[3] = {r1.y, r1.z, r1.w}, an[3] = {r2.x, r2.y, r2.z}, tr[3] = {r3.x, r3.y, r3.z};
    const bool affine = unif_f64(r0.w) < a.p_affine;
    double scale[3], t[3], cs[3], sn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        rec[i] = ((a.flip_mask >> i) & 1) && unif_f64(fl[i]) < a.p_flip ? 1.0 : 0.0;
        scale[i] = a.s_lo + unif_f64(sc[i]) * (a.s_hi - a.s_lo);
        const double deg = sym(an[i], a.deg[i]);
        t[i] = sym(tr[i], a.tr[i]);
        const double rad = deg * 0.017453292519943295;
        cs[i] = cos(rad);
        sn[i] = sin(rad);
        rec[5 + i] = scale[i];
        rec[8 + i] = deg;
        rec[11 + i] = t[i];
    }
    rec[3] = affine ? 1.0 : 0.0;
    rec[4] = unif_f64(r1.x) < a.p_elastic ? 1.0 : 0.0;
    double* M = rec + 14;
    if (affine) {
        // rotations about z, y, x of vectors (z, y, x): each leaves its own component alone
        const double Rz[9] = {1.0, 0.0, 0.0, 0.0, cs[0], -sn[0], 0.0, sn[0], cs[0]};
        const double Ry[9] = {cs[1], 0.0, sn[1], 0.0, 1.0, 0.0, -sn[1], 0.0, cs[1]};
        const double Rx[9] = {cs[2], -sn[2], 0.0, sn[2], cs[2], 0.0, 0.0, 0.0, 1.0};
        double P[9], Q[9], c[3];
        mat3(Rz, Ry, P);
        mat3(P, Rx, Q);
#pragma unroll
        for (int i = 0; i < 3; ++i) c[i] = ((double)(a.n[i] - 1) * 0.5) * a.sp[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double L[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) M[4 * i + j] = L[j] = Q[3 * i + j] * scale[j];
            M[4 * i + 3] = (c[i] - ((L[0] * c[0] + L[1] * c[1]) + L[2] * c[2])) + t[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = i % 5 == 0 ? 1.0 : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- warp
struct WarpArgs {
    int D, H, W, C;
    int G[3];
    int ntx, nty;
    double sp[3];
    const double* record;
    const double* control;
    int64_t* seq;
    int N;
};

// NaN fails both comparisons
__device__ __forceinline__ bool within(double v, int n) { return v >= 0.0 && v < (double)n; }

// uniform cubic B-spline weights of the fraction f
__device__ __forceinline__ void bspline(double f, double B[4]) {
    const double omf = 1.0 - f, f2 = f * f, f3 = f2 * f;
    B[0] = ((omf * omf) * omf) / 6.0;
    B[1] = ((3.0 * f3 - 6.0 * f2) + 4.0) / 6.0;
    B[2] = ((((-3.0 * f3) + 3.0 * f2) + 3.0 * f) + 1.0) / 6.0;
    B[3] = f3 / 6.0;
}

template <class T>
__global__ void __launch_bounds__(SB) spatial_warp_kernel(WarpArgs a, const T* __restrict__ in, T* __restrict__ out) {
    constexpr int VX = 16 / (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) double phi[];                // [3][Gz][Gy][Gx] of this sample
    const int n = blockIdx.y;
    if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0) a.seq[0] += a.N;       // the draw kernel has read it
    const double* rec = a.record + (int64_t)n * REC;
    const bool elastic = rec[4] != 0.0;
    const int g3 = a.G[0] * a.G[1] * a.G[2];
    if (elastic) {                                                              // uniform: one record per block
        const double* ctl = a.control + (int64_t)n * 3 * g3;
        for (int i = threadIdx.x; i < 3 * g3; i += SB) phi[i] = ctl[i];
        __syncthreads();
    }
    const Origin t = origin<T>(a.ntx, a.nty);
    int yy, zz;
    row_of(t, yy, zz);
    if (yy >= a.H || zz >= a.D) return;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    const T* item = in + (int64_t)n * a.C * V;
    T* orow = out + (int64_t)n * a.C * V + ((int64_t)zz * a.H + yy) * a.W;
    const Span s = chunk_of(orow, t.X0, a.W);
    if (s.xa >= s.xb) return;
    const int cx = s.cx;

    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = rec[14 + i];
    const int nn[3] = {a.D, a.H, a.W};
    const double w0 = (double)zz * a.sp[0], w1 = (double)yy * a.sp[1];
    double base[3], ext[3], last[3];
    bool flip[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        base[r] = m[4 * r] * w0 + m[4 * r + 1] * w1;
        ext[r] = (double)nn[r] * a.sp[r];
        last[r] = (double)(nn[r] - 1) * a.sp[r];
        flip[r] = rec[r] != 0.0;
    }

    int src[VX];                                               // the voxel's source index in a channel, -1: the fill
#pragma unroll 1
    for (int v = 0; v < VX; ++v) {
        const int x = min(max(cx + v, 0), a.W - 1);            // a clipped voxel repeats its neighbour and is not stored
        const double w2 = (double)x * a.sp[2];
        double q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) q[r] = (base[r] + m[4 * r + 2] * w2) + m[4 * r + 3];
        if (elastic) {
            double B[3][4];
            int i0[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int mm = a.G[r] - 3;
                double g = (q[r] / ext[r]) * (double)mm;
                g = g >= 0.0 ? g : 0.0;                        // NaN -> 0
                g = g <= (double)mm ? g : (double)mm;
                const int i = min((int)floor(g), mm - 1);      // 0 .. G - 4
                i0[r] = i;
                bspline(g - (double)i, B[r]);
            }
            double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double wzy = B[0][l] * B[1][k];
                    const double* p = phi + ((i0[0] + l) * a.G[1] + (i0[1] + k)) * a.G[2] + i0[2];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double wt = wzy * B[2][j];
                        e0 = e0 + wt * p[j];
                        e1 = e1 + wt * p[g3 + j];
                        e2 = e2 + wt * p[2 * g3 + j];
                    }
                }
            }
            q[0] = q[0] + e0;
            q[1] = q[1] + e1;
            q[2] = q[2] + e2;
        }
        double f[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (flip[r]) q[r] = last[r] - q[r];
            f[r] = floor(q[r] / a.sp[r] + 0.5);
        }
        src[v] = within(f[0], nn[0]) && within(f[1], nn[1]) && within(f[2], nn[2])
                     ? ((int)f[0] * a.H + (int)f[1]) * a.W + (int)f[2] : -1;
    }
    for (int c = 0; c < a.C; ++c) {
        const T* ch = item + (int64_t)c * V;
        T* oc = orow + (int64_t)c * V;
        Chunk<T> res;
#pragma unroll
        for (int v = 0; v < VX; ++v) res.v[v] = src[v] >= 0 ? ch[src[v]] : (T)0;
        // a later channel's rows sit on another 16-byte grid when V sizeof(T) is no multiple of 16
        store(oc, s, res, (uintptr_t)(oc + cx) % 16 == 0);
    }
}

template <class T>
int launch(WarpArgs a, const void* in, void* out, hipStream_t st) {
    const Tiles tl = tiles(a.D, a.H, a.W, out, sizeof(T));
    a.ntx = tl.ntx;
    a.nty = tl.nty;
    const dim3 grid((unsigned)tl.blocks, (unsigned)a.N);
    const size_t lds = (size_t)3 * a.G[0] * a.G[1] * a.G[2] * sizeof(double);   // <= 41472 B
    spatial_warp_kernel<T><<<grid, SB, lds, st>>>(a, (const T*)in, (T*)out);
    CTU_CHECK_LAUNCH("spatial_warp");
    return CTU_OK;
}

bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

int check_grid(const char* who, int N, int D, int H, int W, const double* spacing, int gz, int gy, int gx) {
    CTU_REQUIRE(geometry_ok(N, D, H, W), "%s: bad shape N=%d %dx%dx%d (N <= 65535, every side >= 1, D*H*W < 2^31)", who, N, D, H, W);
    CTU_REQUIRE(spacing && steps_ok(spacing), "%s: spacing must be three positive finite numbers", who);
    CTU_REQUIRE(gz >= GMIN && gz <= GMAX && gy >= GMIN && gy <= GMAX && gx >= GMIN && gx <= GMAX,
                "%s: %dx%dx%d control points (each axis %d..%d)", who, gz, gy, gx, GMIN, GMAX);
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_spatial_draw(int N, int D, int H, int W, const double* spacing, const int64_t* seq, uint64_t seed,
                                int flip_mask, double flip_p, double affine_p, double elastic_p, const double* ranges,
                                int gz, int gy, int gx, int locked, double* record, double* control, void* stream) {
    if (int e = check_grid("spatial_draw", N, D, H, W, spacing, gz, gy, gx)) return e;
    CTU_REQUIRE(seq && ranges && record && control, "spatial_draw: null pointer");
    CTU_REQUIRE(flip_mask >= 0 && flip_mask <= 7, "spatial_draw: bad flip mask %d", flip_mask);
    CTU_REQUIRE(prob_ok(flip_p) && prob_ok(affine_p) && prob_ok(elastic_p), "spatial_draw: probabilities must lie in [0, 1]");
    CTU_REQUIRE(finite_n(ranges, 11), "spatial_draw: scales, degrees, translation and max_displacement must be finite");
    CTU_REQUIRE(locked >= 0 && locked <= 2 && 2 * locked < gz && 2 * locked < gy && 2 * locked < gx,
                "spatial_draw: locked_borders %d leaves no free control point of %dx%dx%d", locked, gz, gy, gx);
    DrawArgs a;
    a.n[0] = D; a.n[1] = H; a.n[2] = W;
    a.G[0] = gz; a.G[1] = gy; a.G[2] = gx;
    a.flip_mask = flip_mask; a.locked = locked;
    a.p_flip = flip_p; a.p_affine = affine_p; a.p_elastic = elastic_p;
    a.s_lo = ranges[0]; a.s_hi = ranges[1];
    for (int i = 0; i < 3; ++i) {
        a.sp[i] = spacing[i];
        a.deg[i] = ranges[2 + i];
        a.tr[i] = ranges[5 + i];
        a.md[i] = ranges[8 + i];
    }
    a.seq = seq;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.record = record; a.control = control;
    spatial_draw_kernel<<<N, SB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("spatial_draw");
    return CTU_OK;
}

extern "C" int ctu_spatial_warp(const void* in, int dtype, int N, int C, int D, int H, int W, const double* spacing,
                                int gz, int gy, int gx, const double* record, const double* control, int64_t* seq,
                                void* out, void* stream) {
    if (int e = check_grid("spatial_warp", N, D, H, W, spacing, gz, gy, gx)) return e;
    CTU_REQUIRE(in && out && record && control && seq, "spatial_warp: null pointer");
    CTU_REQUIRE(C >= 1 && C <= MAXC, "spatial_warp: %d channels (1..%d)", C, MAXC);
    CTU_REQUIRE(in != out, "spatial_warp: the gather cannot run in place");
    WarpArgs a;
    a.D = D; a.H = H; a.W = W; a.C = C; a.N = N;
    a.G[0] = gz; a.G[1] = gy; a.G[2] = gx;
    for (int i = 0; i < 3; ++i) a.sp[i] = spacing[i];
    a.record = record; a.control = control; a.seq = seq;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CTU_U8) return launch<uint8_t>(a, in, out, st);
    if (dtype == CTU_F32) return launch<float>(a, in, out, st);
    CTU_REQUIRE(false, "spatial_warp: unsupported dtype %d (uint8 or float32)", dtype);
}
