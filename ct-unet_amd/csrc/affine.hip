// Affine resampling of 3-D volumes through a 3x4 matrix held in DEVICE memory, gfx950: nearest, trilinear and label-aware
// trilinear (rule: ctunet_amd/resample.py, "affine_resample"; tests/affine_ref.py restates it).
//
// One launch per call, no workspace, no atomics, no host synchronisation; the matrix is read by the kernel, so the result
// of a registration feeds it without a read-back and a captured call follows the tensor it was captured with.  The output
// is tiled by chunk_tile.h: a block of 256 threads owns 4 planes x 4 rows x 16 chunks, a chunk being the 16 bytes of output
// one thread writes (4 float / 8 int16 / 16 uint8 voxels) on the 16-byte grid of its output row.  The tile is
// compact in the output, so under a rigid transform its source footprint is compact too; the inputs are plain gathers
// (profiles/affine.md says what was measured).  Every read is guarded by the comparison that declares its index inside the
// volume, so no matrix (NaN and infinite entries included) can take a read outside it.
// Coordinates: float64, every operation rounded on its own (contraction is off for the file):
//   w_a = out_origin_a + idx_a out_spacing_a;  s_a = ((m_a0 w_0 + m_a1 w_1) + m_a2 w_2) + m_a3;  u_a = (s_a - origin_a) / spacing_a
// Arithmetic of linear / label_linear: trilinear.h (lerp(p, q, w) = p + w (q - p) in float32, x then y then z; label_vote).
//
// No reference counterpart: the reference expects scans registered to its atlas by a host tool (ctunet/pytorch/datasets.py:22-45).
#include <type_traits>

#include "chunk_tile.h"
#include "common.h"
#include "trilinear.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_tile;
using namespace ctu_tri;

constexpr int MAX_BATCH = 65535;                // grid.y

struct AfArgs {
    int D, H, W;                                // input grid
    int d, h, w;                                // output grid
    int ntx, nty;
    int K;
    double sp[3], org[3], osp[3], oorg[3];      // (z, y, x)
    double fill;
    const double* m;                            // DEVICE: row-major, the first 12 entries are read
};

// NaN fails both comparisons
__device__ __forceinline__ bool within(double v, double lo, int n) { return v >= lo && v < (double)n; }

template <class T, int MODE>
__global__ void __launch_bounds__(SB) affine_kernel(AfArgs a, const T* __restrict__ in,
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
    const int cx = s.cx, xa = s.xa, xb = s.xb;

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
#pragma unroll
    for (int v = 0; v < VX; ++v) {
        const int x = min(max(cx + v, 0), a.w - 1);            // a clipped voxel repeats its neighbour and is not stored
        const double w2 = a.oorg[2] + (double)x * a.osp[2];
        double u[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) u[r] = (((base[r] + m[4 * r + 2] * w2) + m[4 * r + 3]) - a.org[r]) / a.sp[r];
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
            O c[8];                                            // a neighbour outside the volume reads as the fill
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int z = i0[0] + (j >> 2), y = i0[1] + ((j >> 1) & 1), xx = i0[2] + (j & 1);
                const bool ok = z >= 0 && z < a.D && y >= 0 && y < a.H && xx >= 0 && xx < a.W;
                c[j] = ok ? (O)item[(z * a.H + y) * a.W + xx] : fillv;
            }
            if constexpr (MODE == LINEAR) {
                val = tri(c, wt[2], wt[1], wt[0]);
            } else {
                val = (O)label_vote(c, a.K, wt[2], wt[1], wt[0]);
            }
        } else if constexpr (MODE == LABEL) {
            val = (unsigned)fillv < (unsigned)a.K ? fillv : (O)0;
        }
        res.v[v] = val;
    }
    // ctu_tile::store(orow, s, res, true), written out: through the call the compiler also prunes the clipped path's
    // comparisons, and the label_linear kernel that results (80 VGPRs instead of 82, 6 waves instead of 5) measured 13 % slower
    if (xb - xa == VX) {
        *reinterpret_cast<Chunk<O>*>(orow + cx) = res;
    } else {
#pragma unroll
        for (int v = 0; v < VX; ++v)
            if (cx + v >= xa && cx + v < xb) orow[cx + v] = res.v[v];
    }
}

template <class T, int MODE>
int launch(AfArgs a, const void* in, int64_t N, void* out, hipStream_t st) {
    typedef typename OutOf<T, MODE>::type O;
    const Tiles tl = tiles(a.d, a.h, a.w, out, sizeof(O));
    a.ntx = tl.ntx;
    a.nty = tl.nty;
    const int64_t vin = (int64_t)a.D * a.H * a.W, vout = (int64_t)a.d * a.h * a.w;
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const int64_t nb = N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH;
        const dim3 grid((unsigned)tl.blocks, (unsigned)nb);
        affine_kernel<T, MODE><<<grid, SB, 0, st>>>(a, (const T*)in + n0 * vin, (O*)out + n0 * vout);
        CTU_CHECK_LAUNCH("affine_resample");
    }
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_affine_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W,
                                   int d, int h, int w, const double* out_to_in, const double* spacing, const double* origin,
                                   const double* out_spacing, const double* out_origin, double fill, void* out, void* stream) {
    CTU_REQUIRE(in && out && out_to_in, "affine_resample: null pointer");
    CTU_REQUIRE(mode >= NEAREST && mode <= LABEL, "affine_resample: unknown mode %d", mode);
    CTU_REQUIRE(N > 0 && grid_ok(D, H, W) && grid_ok(d, h, w),
                "affine_resample: bad shape N=%lld in=%dx%dx%d out=%dx%dx%d (every side >= 1, D*H*W < 2^31 on either grid)",
                (long long)N, D, H, W, d, h, w);
    CTU_REQUIRE((!spacing || steps_ok(spacing)) && (!out_spacing || steps_ok(out_spacing)),
                "affine_resample: spacing must be positive and finite");
    CTU_REQUIRE((!origin || finite_n(origin, 3)) && (!out_origin || finite_n(out_origin, 3)),
                "affine_resample: origin must be finite");
    if (mode == LABEL)
        CTU_REQUIRE(num_classes >= 2 && num_classes <= 16, "affine_resample: num_classes must lie in 2..16, got %d", num_classes);
    AfArgs a;
    a.D = D; a.H = H; a.W = W; a.d = d; a.h = h; a.w = w;
    a.K = num_classes; a.m = out_to_in; a.fill = fill;
    for (int i = 0; i < 3; ++i) {
        a.sp[i] = spacing ? spacing[i] : 1.0;
        a.org[i] = origin ? origin[i] : 0.0;
        a.osp[i] = out_spacing ? out_spacing[i] : 1.0;
        a.oorg[i] = out_origin ? out_origin[i] : 0.0;
    }
    hipStream_t st = (hipStream_t)stream;
#define AF(T, MODE) return launch<T, MODE>(a, in, N, out, st)
    if (mode == NEAREST) {
        const bool whole = fill == (double)(long long)fill;
        if (dtype == CTU_U8) {
            CTU_REQUIRE(whole && fill >= 0 && fill <= 255, "affine_resample: fill %g is no uint8", fill);
            AF(uint8_t, NEAREST);
        }
        if (dtype == CTU_I16) {
            CTU_REQUIRE(whole && fill >= -32768 && fill <= 32767, "affine_resample: fill %g is no int16", fill);
            AF(int16_t, NEAREST);
        }
        if (dtype == CTU_F32) {
            CTU_REQUIRE((double)(float)fill - (double)(float)fill == 0.0, "affine_resample: fill %g is not finite in float32", fill);
            AF(float, NEAREST);
        }
        CTU_REQUIRE(false, "affine_resample: unsupported dtype %d for nearest (uint8, int16 or float32)", dtype);
    }
    if (mode == LINEAR) {
        CTU_REQUIRE((double)(float)fill - (double)(float)fill == 0.0, "affine_resample: fill %g is not finite in float32", fill);
        if (dtype == CTU_F32) AF(float, LINEAR);
        if (dtype == CTU_I16) AF(int16_t, LINEAR);
        if (dtype == CTU_U8) AF(uint8_t, LINEAR);
        CTU_REQUIRE(false, "affine_resample: unsupported dtype %d for linear (float32, int16 or uint8)", dtype);
    }
    CTU_REQUIRE(fill == (double)(long long)fill && fill >= 0 && fill <= 255, "affine_resample: fill %g is no uint8 label", fill);
    if (dtype == CTU_U8) AF(uint8_t, LABEL);
#undef AF
    CTU_REQUIRE(false, "affine_resample: unsupported dtype %d for label_linear (uint8)", dtype);
}
