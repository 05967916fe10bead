// On-device irregular craniectomy defects and random skull dilation, gfx950 (rules: ctunet_amd/transforms.py,
// "SkullRandomDefect" and "RandomDilate"; tests/defect_ref.py restates them).  No atomics, no host synchronisation, so the
// calls replay inside a captured graph and are bitwise reproducible:
//   ctu_defect_draw    one block per sample: the per-sample scalars, the chain of balls and the voxel box that holds them
//                      (float64 record), and the roughness lattice, from Philox4x32-10 and the instance's DEVICE counter.
//                      The centre is the k-th bone voxel behind ctu_flap_count's chunk counts (flap_pass.h).
//   ctu_defect_apply   the fused streaming pass of ctu_flap_apply (flap_pass.h: 4 voxels per thread, 16-byte stores where
//                      aligned, noise, atlas channel, one-hot targets) with the union of rough balls as the hole.  A block
//                      serves one sample and stages its record (64 doubles) in LDS; the shape test runs only for the bone
//                      voxels of the quads that meet the record's box -- a wave covers 256 voxels of a row, so nearly every
//                      wave takes or leaves that branch whole.  Inside, a voxel reads 8 lattice values (a few KB per
//                      sample, cache resident) and tests at most 12 balls in float64.
//   ctu_random_dilate  k iterations of the 6-neighbour cross = the L1 ball of radius k, as ONE gather: a lane owns 16
//                      x-consecutive voxels (voxel_rows.h) and ORs, over the rows (dz, dy) with |dz| + |dy| <= k, the row's
//                      bits spread by k - |dz| - |dy| along x (the few voxels either side are read one by one).
//                      Whether a sample is dilated is drawn on the device; a one-thread launch then advances the counter
//                      (the gather's blocks all read it).
// Coordinates: float64, every operation rounded on its own (contraction is off for the file).
//
// Replaces: the "complex defects" and "erosions / dilations" steps that the docstring of ctunet/pytorch/transforms.py:173-228
//           (cranioplasty_transform) lists and the reference does not implement; the rules are the port's own.
#include "flap_pass.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)

namespace {

using namespace ctu_flap;

constexpr int DREC = CTU_DEFECT_RECORD;
constexpr int MAXB = CTU_DEFECT_MAX_BALLS;
constexpr int MAXG = CTU_DEFECT_MAX_LATTICE;
constexpr int BALL0 = 16;                         // record: ball j at BALL0 + 4 j = (cz, cy, cx, r)
static_assert(BALL0 + 4 * MAXB == DREC, "record layout");

// ---------------------------------------------------------------------------------------------------------------- draw
struct DrawArgs {
    const void* skull;
    int u8, D, H, W, nchunks;
    int G[3];
    int balls_lo, balls_hi;
    const int32_t* counts;
    const int64_t* seq;
    uint32_t k0, k1;
    double p, sp[3], r_lo, r_hi, spread, shrink_lo, shrink_hi, amp;
    double* record;
    double* lattice;
};

__global__ void __launch_bounds__(AB) defect_draw_kernel(DrawArgs a) {
    const int n = blockIdx.x;
    const int64_t seq = a.seq[0] + n;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    const int g3 = a.G[0] * a.G[1] * a.G[2];
    double* lat = a.lattice + (int64_t)n * g3;
    for (int i = threadIdx.x; i < g3; i += AB) lat[i] = 2.0 * unif_f64(philox_seq((uint32_t)i, 1, seq, a.k0, a.k1).x) - 1.0;

    __shared__ int64_t tsum[AB];
    __shared__ int64_t sh_chunk, sh_kloc, sh_idx;
    __shared__ double ball[4 * MAXB];
    double* rec = a.record + (int64_t)n * DREC;
    const int32_t* cn = a.counts + (int64_t)n * a.nchunks;
    segment_counts(cn, a.nchunks, tsum);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint4 r = philox_seq(0, 0, seq, a.k0, a.k1);
        const int64_t total = bone_total(tsum);
        const int64_t k = total > 0 ? draw_int(r.y, 0, (uint64_t)total) : 0;
        int64_t chunk = -1, kloc = 0;
        if (total > 0) find_chunk(cn, a.nchunks, tsum, k, chunk, kloc);
        sh_chunk = chunk;
        sh_kloc = kloc;
        sh_idx = -1;
        const bool apply = unif_f64(r.x) < a.p;
        rec[0] = apply ? 1.0 : 0.0;
        rec[1] = (double)total;
        rec[2] = (double)k;
        rec[6] = (double)(a.balls_lo + (int)draw_int(r.w, 0, (uint64_t)(a.balls_hi - a.balls_lo + 1)));
        rec[7] = apply && total > 0 ? 1.0 : 0.0;
        ball[3] = a.r_lo + unif_f64(r.z) * (a.r_hi - a.r_lo);
    }
    __syncthreads();
    if (threadIdx.x < 64 && sh_chunk >= 0) scan_chunk(a.skull, a.u8, (int64_t)n * V, V, sh_chunk, sh_kloc, &sh_idx);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int64_t i = sh_idx;
    const int nn[3] = {a.D, a.H, a.W};
    if (i < 0) {                                      // no bone: no chain, an empty box
        for (int j = 3; j < DREC; ++j)
            if (j != 6 && j != 7) rec[j] = 0.0;
        for (int c = 0; c < 3; ++c) rec[3 + c] = rec[11 + c] = -1.0;
        return;
    }
    const int64_t hw = (int64_t)a.H * a.W;
    const int ctr[3] = {(int)(i / hw), (int)((i / a.W) % a.H), (int)(i % a.W)};
    const int K = (int)rec[6];
    for (int c = 0; c < 3; ++c) {
        rec[3 + c] = (double)ctr[c];
        ball[c] = (double)ctr[c] * a.sp[c];
    }
    for (int j = 1; j < K; ++j) {
        const uint4 q = philox_seq((uint32_t)(16 + 2 * j), 0, seq, a.k0, a.k1);
        const uint4 s = philox_seq((uint32_t)(17 + 2 * j), 0, seq, a.k0, a.k1);
        const double* par = ball + 4 * (int)draw_int(q.x, 0, (uint64_t)j);
        const uint32_t w[3] = {s.x, s.y, s.z};
        ball[4 * j + 3] = (a.shrink_lo + unif_f64(q.y) * (a.shrink_hi - a.shrink_lo)) * par[3];
        for (int c = 0; c < 3; ++c) ball[4 * j + c] = par[c] + ((2.0 * unif_f64(w[c]) - 1.0) * a.spread) * par[3];
    }
    for (int j = 0; j < 4 * MAXB; ++j) rec[BALL0 + j] = j < 4 * K ? ball[j] : 0.0;
    for (int c = 0; c < 3; ++c) {
        double mn = 0.0, mx = 0.0;
        for (int j = 0; j < K; ++j) {
            const double e = ball[4 * j + 3] + a.amp;
            const double lo = floor((ball[4 * j + c] - e) / a.sp[c]), hi = ceil((ball[4 * j + c] + e) / a.sp[c]);
            mn = j == 0 || lo < mn ? lo : mn;
            mx = j == 0 || hi > mx ? hi : mx;
        }
        rec[8 + c] = fmax(0.0, mn - 1.0);
        rec[11 + c] = fmin((double)(nn[c] - 1), mx + 1.0);
    }
    rec[14] = rec[15] = 0.0;
}

// --------------------------------------------------------------------------------------------------------------- apply
struct ApplyArgs {
    const void* skull;
    const float* atlas;
    const int32_t* params;        // ctu_flap_draw's records, noise fields (null without noise)
    const double* record;
    const double* lattice;
    int64_t* hole_seq;
    int64_t* noise_seq;
    float* noise_nd;
    float* x;
    float* full;
    float* flap;
    int u8, N, D, H, W, C, mode, decay, vec;
    int G[3];
    double sp[3], scale, amp;
    uint32_t nk0, nk1;
};

// the lattice cell and the fraction of world coordinate w on an axis with G lattice points; floor(w / scale) <= G - 2 by
// the choice of G, the minimum only keeps a read inside the lattice whatever the arguments
__device__ __forceinline__ void cell(double w, double scale, int G, int& i, double& f) {
    const double g = w / scale;
    i = max(0, min((int)floor(g), G - 2));
    f = g - (double)i;
}

__device__ __forceinline__ double lerp(double a, double b, double f) { return a + f * (b - a); }

__global__ void __launch_bounds__(AB) defect_apply_kernel(ApplyArgs a) {
    const int n = blockIdx.y;
    if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0)
        advance_state(a.mode, a.decay, a.N, a.params, a.hole_seq, a.noise_seq, a.noise_nd);
    __shared__ double tab[DREC];
    const bool cut = a.record[(int64_t)n * DREC + 7] != 0.0;                    // uniform over the block
    int lo[3] = {1, 1, 1}, hi[3] = {0, 0, 0}, K = 0;
    if (cut) {
        if (threadIdx.x < DREC) tab[threadIdx.x] = a.record[(int64_t)n * DREC + threadIdx.x];
        __syncthreads();
        K = min((int)tab[6], MAXB);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = (int)fmin(tab[8 + c], 2.0e9);
            hi[c] = (int)fmax(tab[11 + c], -1.0);
        }
    }
    const double* lat = a.lattice + (int64_t)n * a.G[0] * a.G[1] * a.G[2];
    const int32_t* rec = a.params ? a.params + (int64_t)n * REC : nullptr;
    const bool noisy = (a.mode & CTU_FLAP_NOISE) && rec[10];
    const uint32_t Wq = (uint32_t)(a.W + 3) >> 2;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    const uint32_t quads = (uint32_t)a.D * a.H * Wq;                            // < 2^32: check_shape
    for (uint64_t g64 = (uint64_t)blockIdx.x * AB + threadIdx.x; g64 < quads; g64 += (uint64_t)gridDim.x * AB) {
        const uint32_t g = (uint32_t)g64;
        const uint32_t row = g / Wq;
        const int xq = (int)(g - row * Wq);
        const int z = (int)(row / (uint32_t)a.H);
        const int y = (int)(row - (uint32_t)z * a.H);
        const int x = 4 * xq;
        const int64_t zyx = ((int64_t)z * a.H + y) * a.W + x;
        float val[4];
        read_quad(a.skull, a.u8, a.vec, (int64_t)n * V + zyx, x, a.W, val);
        float img[4], bone[4], fl[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            bone[l] = val[l] >= 1.0f ? 1.f : 0.f;
            img[l] = cut ? bone[l] : val[l];
            fl[l] = 0.f;
        }
        if (z >= lo[0] && z <= hi[0] && y >= lo[1] && y <= hi[1] && x + 3 >= lo[2] && x <= hi[2] &&
            bone[0] + bone[1] + bone[2] + bone[3] != 0.f) {
            int iz, iy;
            double fz, fy;
            const double wz = (double)z * a.sp[0], wy = (double)y * a.sp[1];
            cell(wz, a.scale, a.G[0], iz, fz);
            cell(wy, a.scale, a.G[1], iy, fy);
            const double* l00 = lat + ((int64_t)iz * a.G[1] + iy) * a.G[2];
            const double* l01 = l00 + a.G[2];
            const double* l10 = l00 + (int64_t)a.G[1] * a.G[2];
            const double* l11 = l10 + a.G[2];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (bone[l] == 0.f) continue;                                   // covers x + l >= W: no value was read there
                int ix;
                double fx;
                const double wx = (double)(x + l) * a.sp[2];
                cell(wx, a.scale, a.G[2], ix, fx);
                const double c0 = lerp(lerp(l00[ix], l00[ix + 1], fx), lerp(l01[ix], l01[ix + 1], fx), fy);
                const double c1 = lerp(lerp(l10[ix], l10[ix + 1], fx), lerp(l11[ix], l11[ix + 1], fx), fy);
                const double rough = a.amp * lerp(c0, c1, fz);
                bool in = false;
                for (int j = 0; j < K; ++j) {
                    const double* b = tab + BALL0 + 4 * j;
                    const double rho = b[3] + rough;
                    const double dz = wz - b[0], dy = wy - b[1], dx = wx - b[2];
                    in = in || (rho > 0.0 && (dz * dz + dy * dy) + dx * dx <= rho * rho);
                }
                if (in) { img[l] = 0.f; fl[l] = 1.f; }
            }
        }
        if (noisy) salt_pepper(rec, g, a.nk0, a.nk1, img);
        float* xo = a.x + (int64_t)n * a.C * V + zyx;
        write_quad(xo, a.atlas && a.C > 1 ? a.atlas + zyx : nullptr, a.full ? a.full + (int64_t)n * 2 * V + zyx : nullptr,
                   a.flap ? a.flap + (int64_t)n * 2 * V + zyx : nullptr, V, a.vec, x, a.W, img, bone, fl);
    }
}

// -------------------------------------------------------------------------------------------------------------- dilate
constexpr int MAX_ITER = CTU_DILATE_MAX_ITERATIONS;

// bone of either input type: the uint8 cast (truncation on [0, 256)) is nonzero
struct Bone {
    __device__ __forceinline__ bool operator()(uint8_t v) const { return v != 0; }
    __device__ __forceinline__ bool operator()(float v) const { return v >= 1.0f; }
};

// thread (row, q): the output voxels x = 16 q .. 16 q + 15 of one row of sample blockIdx.y
template <class T>
__global__ void __launch_bounds__(AB) random_dilate_kernel(const T* __restrict__ in, uint8_t* __restrict__ out, int D, int H,
                                                           int W, int iterations, const int64_t* __restrict__ seq,
                                                           uint32_t k0, uint32_t k1, double p) {
    const int n = blockIdx.y;
    const int Q = (W + 15) >> 4;
    const int64_t gid = (int64_t)blockIdx.x * AB + threadIdx.x;
    const int64_t row = gid / Q;
    if (row >= (int64_t)D * H) return;
    const int q = (int)(gid - row * Q);
    const int y = (int)(row % H), z = (int)(row / H);
    const int x0 = 16 * q;
    const int nv = min(16, W - x0);
    const int64_t V = (int64_t)D * H * W;
    const bool dilate = unif_f64(philox_seq(0, 0, seq[0] + n, k0, k1).x) < p;
    const int k = dilate ? iterations : 0;
    const T* item = in + (int64_t)n * V;
    uint32_t m = 0;
    for (int dz = -k; dz <= k; ++dz) {
        const int zz = z + dz, ky = k - abs(dz);
        if (zz < 0 || zz >= D) continue;
        for (int dy = -ky; dy <= ky; ++dy) {
            const int yy = y + dy, r = ky - abs(dy);
            if (yy < 0 || yy >= H) continue;
            const T* pr = item + ((int64_t)zz * H + yy) * W + x0;
            // bit i of the window = voxel x0 - MAX_ITER + i, spread by r along x
            uint32_t wide = ctu_vox::mask16(pr, nv, Bone{}) << MAX_ITER;
            for (int d = 1; d <= r; ++d) {
                if (x0 - d >= 0 && Bone{}(pr[-d])) wide |= 1u << (MAX_ITER - d);
                if (x0 + 15 + d < W && Bone{}(pr[15 + d])) wide |= 1u << (MAX_ITER + 15 + d);
            }
            uint32_t acc = wide;
            for (int s = 1; s <= r; ++s) acc |= (wide << s) | (wide >> s);
            m |= acc >> MAX_ITER;
        }
    }
    ctu_vox::store_mask16(out + (int64_t)n * V + row * W + x0, nv, m & 0xffffu);
}

__global__ void advance_kernel(int64_t* seq, int N) { seq[0] += N; }

bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

}  // namespace

extern "C" int ctu_defect_draw(const void* skull, int u8, int N, int D, int H, int W, const double* spacing,
                               const int32_t* counts, const int64_t* seq, uint64_t seed, double p, const double* ranges,
                               int balls_lo, int balls_hi, int gz, int gy, int gx, double* record, double* lattice,
                               void* stream) {
    if (int e = check_shape(N, D, H, W)) return e;
    CTU_REQUIRE(skull && spacing && counts && seq && ranges && record && lattice, "defect_draw: null pointer");
    CTU_REQUIRE(N <= 65535, "defect_draw: batch %d too large", N);
    CTU_REQUIRE(steps_ok(spacing), "defect_draw: spacing must be three positive finite numbers");
    CTU_REQUIRE(prob_ok(p), "defect_draw: p must lie in [0, 1]");
    CTU_REQUIRE(finite_n(ranges, 6), "defect_draw: radius, spread, shrink and roughness must be finite");
    CTU_REQUIRE(ranges[0] > 0.0 && ranges[0] <= ranges[1], "defect_draw: radius range must satisfy 0 < lo <= hi");
    CTU_REQUIRE(ranges[2] >= 0.0, "defect_draw: negative spread");
    CTU_REQUIRE(ranges[3] > 0.0 && ranges[3] <= ranges[4] && ranges[4] <= 1.0, "defect_draw: shrink must satisfy 0 < lo <= hi <= 1");
    CTU_REQUIRE(ranges[5] >= 0.0, "defect_draw: negative roughness");
    CTU_REQUIRE(balls_lo >= 1 && balls_lo <= balls_hi && balls_hi <= MAXB, "defect_draw: balls [%d, %d] outside 1..%d",
                balls_lo, balls_hi, MAXB);
    CTU_REQUIRE(gz >= 2 && gz <= MAXG && gy >= 2 && gy <= MAXG && gx >= 2 && gx <= MAXG,
                "defect_draw: %dx%dx%d lattice points (each axis 2..%d)", gz, gy, gx, MAXG);
    DrawArgs a;
    a.skull = skull;
    a.u8 = u8 ? 1 : 0;
    a.D = D; a.H = H; a.W = W;
    a.nchunks = (int)ceil_div64((int64_t)D * H * W, CTU_FLAP_CHUNK);
    a.G[0] = gz; a.G[1] = gy; a.G[2] = gx;
    a.balls_lo = balls_lo; a.balls_hi = balls_hi;
    a.counts = counts; a.seq = seq;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.p = p;
    for (int i = 0; i < 3; ++i) a.sp[i] = spacing[i];
    a.r_lo = ranges[0]; a.r_hi = ranges[1]; a.spread = ranges[2];
    a.shrink_lo = ranges[3]; a.shrink_hi = ranges[4]; a.amp = ranges[5];
    a.record = record; a.lattice = lattice;
    defect_draw_kernel<<<N, AB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("defect_draw");
    return CTU_OK;
}

extern "C" int ctu_defect_apply(const void* skull, int u8, const float* atlas, int N, int D, int H, int W,
                                const double* spacing, const double* record, const double* lattice, int gz, int gy, int gx,
                                double scale, double amp, const int32_t* params, int mode, int64_t* hole_seq,
                                int64_t* noise_seq, float* noise_nd, uint64_t noise_seed, int decay, float* x, int C,
                                float* full, float* flap, void* stream) {
    if (int e = check_shape(N, D, H, W)) return e;
    CTU_REQUIRE(skull && spacing && record && lattice && hole_seq && x, "defect_apply: null pointer");
    CTU_REQUIRE(N <= 65535, "defect_apply: batch %d too large", N);
    CTU_REQUIRE(mode == CTU_FLAP_HOLE || mode == (CTU_FLAP_HOLE | CTU_FLAP_NOISE), "defect_apply: bad mode %d", mode);
    CTU_REQUIRE(!(mode & CTU_FLAP_NOISE) || (params && noise_seq && noise_nd), "defect_apply: noise needs records, counter and density");
    CTU_REQUIRE(C == 1 || C == 2, "defect_apply: %d input channels (1, or 2 with the atlas)", C);
    CTU_REQUIRE((C == 2) == (atlas != nullptr), "defect_apply: the second input channel is the atlas");
    CTU_REQUIRE(steps_ok(spacing), "defect_apply: spacing must be three positive finite numbers");
    CTU_REQUIRE(scale > 0.0 && finite_n(&scale, 1) && amp >= 0.0 && finite_n(&amp, 1), "defect_apply: bad roughness scale or amplitude");
    CTU_REQUIRE(gz >= 2 && gz <= MAXG && gy >= 2 && gy <= MAXG && gx >= 2 && gx <= MAXG,
                "defect_apply: %dx%dx%d lattice points (each axis 2..%d)", gz, gy, gx, MAXG);
    ApplyArgs a;
    a.skull = skull; a.atlas = atlas; a.params = (mode & CTU_FLAP_NOISE) ? params : nullptr;
    a.record = record; a.lattice = lattice;
    a.hole_seq = hole_seq; a.noise_seq = noise_seq; a.noise_nd = noise_nd;
    a.x = x; a.full = full; a.flap = flap;
    a.u8 = u8 ? 1 : 0;
    a.N = N; a.D = D; a.H = H; a.W = W; a.C = C;
    a.mode = mode; a.decay = decay ? 1 : 0;
    a.vec = quad_vec(skull, a.u8, atlas, W, x, full, flap);
    a.G[0] = gz; a.G[1] = gy; a.G[2] = gx;
    for (int i = 0; i < 3; ++i) a.sp[i] = spacing[i];
    a.scale = scale; a.amp = amp;
    a.nk0 = (uint32_t)noise_seed; a.nk1 = (uint32_t)(noise_seed >> 32);
    const int64_t quads = (int64_t)D * H * ((W + 3) / 4);
    const int64_t cap = std::max<int64_t>(1, 2048 / N);                         // about 2048 blocks over the batch
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(quads, AB), cap)), (unsigned)N);
    defect_apply_kernel<<<grid, AB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("defect_apply");
    return CTU_OK;
}

extern "C" int ctu_random_dilate(const void* in, int dtype, int N, int D, int H, int W, int iterations, int64_t* seq,
                                 uint64_t seed, double p, uint8_t* out, void* stream) {
    CTU_REQUIRE(in && out && seq, "random_dilate: null pointer");
    CTU_REQUIRE(geometry_ok(N, D, H, W), "random_dilate: bad shape N=%d %dx%dx%d (N <= 65535, D*H*W < 2^31)", N, D, H, W);
    CTU_REQUIRE(iterations >= 1 && iterations <= MAX_ITER, "random_dilate: %d iterations (1..%d)", iterations, MAX_ITER);
    CTU_REQUIRE(prob_ok(p), "random_dilate: p must lie in [0, 1]");
    CTU_REQUIRE(in != (const void*)out, "random_dilate: the gather cannot run in place");
    hipStream_t st = (hipStream_t)stream;
    const int64_t threads = (int64_t)D * H * ((W + 15) / 16);
    const dim3 grid((unsigned)ceil_div64(threads, AB), (unsigned)N);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (dtype == CTU_U8)
        random_dilate_kernel<uint8_t><<<grid, AB, 0, st>>>((const uint8_t*)in, out, D, H, W, iterations, seq, k0, k1, p);
    else if (dtype == CTU_F32)
        random_dilate_kernel<float><<<grid, AB, 0, st>>>((const float*)in, out, D, H, W, iterations, seq, k0, k1, p);
    else
        CTU_REQUIRE(false, "random_dilate: unsupported dtype %d (uint8 or float32)", dtype);
    CTU_CHECK_LAUNCH("random_dilate");
    advance_kernel<<<1, 1, 0, st>>>(seq, N);
    CTU_CHECK_LAUNCH("random_dilate advance");
    return CTU_OK;
}
