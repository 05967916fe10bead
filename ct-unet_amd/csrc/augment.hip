// On-device flap-reconstruction augmentation, gfx950: the reference's SkullRandomHole (random hole in a binary skull) and
// SaltAndPepper (random zeroed / set voxels) for a batch of N skulls, in three launches and without atomics or host syncs,
// so the whole transform replays inside a captured graph and is bitwise reproducible:
//   ctu_flap_count  bone voxels per (sample, chunk of CTU_FLAP_CHUNK voxels in C order)
//   ctu_flap_draw   one block per sample: the per-sample scalars from Philox4x32-10 (philox.h) and the k-th bone voxel
//   ctu_flap_apply  one fused streaming pass: hole mask, noise, network input (+ atlas channel) and one-hot targets
// The rules (shapes, RNG streams, record layout) are pinned in ctunet_amd/transforms.py and include/ctunet_hip.h.
//
// Replaces: ctunet/pytorch/transforms.py:13-95 (SaltAndPepper, SkullRandomHole) and ctunet/utilities.py:127-178 (shape_3d),
//           ctunet/pytorch/transforms.py:241-300 (random_blank_patch), run per sample in NumPy on the host there.
#include "flap_pass.h"

namespace {

using namespace ctu_flap;

// --------------------------------------------------------------------------------------------------------------- count
// grid (nchunks, N): block (c, n) counts the bone voxels of flat indices [c CH, min(V, (c+1) CH)) of sample n.
// vec: the sample's bytes start 16-byte aligned (every chunk then does too), 16-byte loads of 4 floats / 16 bytes.
__global__ void __launch_bounds__(AB) flap_count_kernel(const void* __restrict__ skull, int u8, int64_t V, int nchunks,
                                                        int vec, int32_t* __restrict__ counts) {
    const int c = blockIdx.x, n = blockIdx.y;
    const int64_t s0 = (int64_t)c * CTU_FLAP_CHUNK, s1 = min(V, s0 + CTU_FLAP_CHUNK);
    const int64_t base = (int64_t)n * V;
    const int per = u8 ? 16 : 4;                      // voxels per 16 bytes
    int cnt = 0;
    for (int64_t s = s0 + (int64_t)threadIdx.x * per; s < s1; s += (int64_t)AB * per) {
        if (vec && s + per <= s1) {
            const uint4 q = *reinterpret_cast<const uint4*>(static_cast<const char*>(skull) + (base + s) * (u8 ? 1 : 4));
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u8) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) cnt += ((w[j] >> (8 * b)) & 0xFFu) != 0;
                } else {
                    cnt += __uint_as_float(w[j]) >= 1.0f;
                }
            }
        } else {
            for (int64_t i = s; i < min(s1, s + per); ++i) cnt += bone_at(skull, u8, base + i);
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    __shared__ int wsum[AB / 64];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < AB / 64; ++w) t += wsum[w];
        counts[(int64_t)n * nchunks + c] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- draw
struct DrawArgs {
    const void* skull;
    int u8, N, D, H, W, nchunks, mode, decay, size_lo, size_hi, shapes;
    const int32_t* counts;
    const int64_t* hole_seq;
    const int64_t* noise_seq;
    const float* noise_nd;
    uint32_t hk0, hk1, nk0, nk1;
    float p_hole, p_noise, salt_ratio;
    int32_t* params;
};

// one block per sample n; thread 0 draws the scalars, the block finds the centre (record layout: ctunet_hip.h)
__global__ void __launch_bounds__(AB) flap_draw_kernel(DrawArgs a) {
    const int n = blockIdx.x;
    int32_t* rec = a.params + (int64_t)n * REC;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    __shared__ int64_t tsum[AB];
    __shared__ int64_t sh_chunk, sh_kloc, sh_idx;
    if (a.mode & CTU_FLAP_HOLE) {
        const int64_t seq = a.hole_seq[0] + n;
        const int32_t* cn = a.counts + (int64_t)n * a.nchunks;
        segment_counts(cn, a.nchunks, tsum);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint4 r = philox_seq(0, 0, seq, a.hk0, a.hk1);
            const uint4 r2 = philox_seq(1, 0, seq, a.hk0, a.hk1);
            const int64_t total = bone_total(tsum);
            const int64_t k = total > 0 ? draw_int(r.y, 0, (uint64_t)total) : 0;
            int64_t chunk = -1, kloc = 0;
            if (total > 0) find_chunk(cn, a.nchunks, tsum, k, chunk, kloc);
            sh_chunk = chunk;
            sh_kloc = kloc;
            sh_idx = -1;
            const int size = (int)draw_int(r.z, a.size_lo, (uint64_t)(a.size_hi - a.size_lo));
            const int nsh = a.shapes & 3;
            const int shape = (a.shapes >> (2 + 2 * (int)draw_int(r.w, 0, (uint64_t)nsh))) & 3;
            // c_diam = U(0.25, 1) size / 4, every operation rounded separately (no contraction)
            const float cd = __fmul_rn(__fmul_rn(__fadd_rn(0.25f, __fmul_rn(0.75f, unif_f32(r2.x))), (float)size), 0.25f);
            rec[0] = unif_f32(r.x) < a.p_hole;
            rec[1] = (int32_t)total;
            rec[2] = (int32_t)k;
            rec[6] = size;
            rec[7] = shape;
            rec[8] = __float_as_int(cd);
            rec[9] = rec[0] && total > 0;
        }
        __syncthreads();
        if (threadIdx.x < 64 && sh_chunk >= 0) scan_chunk(a.skull, a.u8, (int64_t)n * V, V, sh_chunk, sh_kloc, &sh_idx);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int64_t i = sh_idx;
            const int64_t hw = (int64_t)a.H * a.W;
            rec[3] = i < 0 ? -1 : (int32_t)(i / hw);
            rec[4] = i < 0 ? -1 : (int32_t)((i / a.W) % a.H);
            rec[5] = i < 0 ? -1 : (int32_t)(i % a.W);
        }
    } else if (threadIdx.x == 0) {
        for (int j = 0; j < 10; ++j) rec[j] = 0;
        rec[3] = rec[4] = rec[5] = -1;
    }
    if (threadIdx.x != 0) return;
    if (a.mode & CTU_FLAP_NOISE) {
        const int64_t s0 = a.noise_seq[0];
        const int64_t seq = s0 + n;
        const uint4 q = philox_seq(0, 0, seq, a.nk0, a.nk1);
        float nd = a.noise_nd[0];
        if (a.decay) {                                // nd_j = U_j nd_{j-1} over the samples before this one, in order
            for (int j = 0; j <= n; ++j) nd = __fmul_rn(unif_f32(philox_seq(0, 0, s0 + j, a.nk0, a.nk1).y), nd);
        } else {
            nd = __fmul_rn(unif_f32(q.y), nd);
        }
        rec[10] = unif_f32(q.x) < a.p_noise;
        rec[11] = __float_as_int(nd);
        rec[12] = __float_as_int(__fmul_rn(nd, __fsub_rn(1.0f, a.salt_ratio)));
        rec[13] = __float_as_int(__fmul_rn(nd, a.salt_ratio));
        rec[14] = (int32_t)(uint32_t)(uint64_t)seq;
        rec[15] = (int32_t)(uint32_t)((uint64_t)seq >> 32);
    } else {
        for (int j = 10; j < REC; ++j) rec[j] = 0;
    }
}

// --------------------------------------------------------------------------------------------------------------- apply
struct ApplyArgs {
    const void* skull;
    const float* atlas;
    const int32_t* params;
    int64_t* hole_seq;
    int64_t* noise_seq;
    float* noise_nd;
    float* x;
    float* full;
    float* flap;
    int u8, N, D, H, W, C, mode, decay, vec;
    uint32_t nk0, nk1;
};

// inside the hole shape of record rec at voxel (z, y, x); integer tests, the flap cylinders in doubled coordinates
__device__ __forceinline__ bool inside(int shape, int size, float cd2, int dz, int dy, int dx, int y2c, int x2c1, int x2c2,
                                       int y, int x) {
    const int64_t lz = dz, ly = dy, lx = dx, s = size;
    if (shape == CTU_FLAP_SPHERE) return s >= 0 && lz * lz + ly * ly + lx * lx <= s * s;
    const int64_t az = lz < 0 ? -lz : lz, ay = ly < 0 ? -ly : ly, ax = lx < 0 ? -lx : lx;
    if (shape == CTU_FLAP_BOX) return az <= s && ay <= s && ax <= s;
    if (2 * az > s) return false;                     // cube and both cylinders: |z - cz| <= size / 2
    if (2 * ay <= s && 2 * ax <= s) return true;
    const int64_t ey = 2 * (int64_t)y - y2c, e1 = 2 * (int64_t)x - x2c1, e2 = 2 * (int64_t)x - x2c2;
    return (double)(ey * ey + e1 * e1) <= (double)cd2 || (double)(ey * ey + e2 * e2) <= (double)cd2;
}

__global__ void __launch_bounds__(AB) flap_apply_kernel(ApplyArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) advance_state(a.mode, a.decay, a.N, a.params, a.hole_seq, a.noise_seq, a.noise_nd);
    const int Wq = (a.W + 3) >> 2;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    const int64_t total = (int64_t)a.N * a.D * a.H * Wq;
    for (int64_t g = (int64_t)blockIdx.x * AB + threadIdx.x; g < total; g += (int64_t)gridDim.x * AB) {
        const int xq = (int)(g % Wq);
        const int64_t row = g / Wq;
        const int y = (int)(row % a.H);
        const int z = (int)((row / a.H) % a.D);
        const int n = (int)(row / ((int64_t)a.H * a.D));
        const int x = 4 * xq;
        const int64_t zyx = ((int64_t)z * a.H + y) * a.W + x;
        const int64_t src = (int64_t)n * V + zyx;
        const int32_t* rec = a.params + (int64_t)n * REC;
        float val[4];
        read_quad(a.skull, a.u8, a.vec, src, x, a.W, val);
        float img[4], bone[4], fl[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            bone[l] = val[l] >= 1.0f ? 1.f : 0.f;
            img[l] = val[l];
            fl[l] = 0.f;
        }
        if ((a.mode & CTU_FLAP_HOLE) && rec[9]) {
            const int cz = rec[3], cy = rec[4], cx = rec[5], size = rec[6], shape = rec[7];
            const float cd = __int_as_float(rec[8]);
            const float cd2 = __fmul_rn(2.f * cd, 2.f * cd);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const bool in = inside(shape, size, cd2, z - cz, y - cy, x + l - cx, 2 * cy - size, 2 * cx - size,
                                       2 * cx + size, y, x + l);
                const bool b = bone[l] != 0.f;
                img[l] = b && !in ? 1.f : 0.f;
                fl[l] = b && in ? 1.f : 0.f;
            }
        }
        if ((a.mode & CTU_FLAP_NOISE) && rec[10])
            salt_pepper(rec, (uint32_t)(((int64_t)z * a.H + y) * Wq + xq), a.nk0, a.nk1, img);
        float* xo = a.x + (int64_t)n * a.C * V + zyx;
        write_quad(xo, a.atlas && a.C > 1 ? a.atlas + zyx : nullptr, a.full ? a.full + (int64_t)n * 2 * V + zyx : nullptr,
                   a.flap ? a.flap + (int64_t)n * 2 * V + zyx : nullptr, V, a.vec, x, a.W, img, bone, fl);
    }
}

}  // namespace

extern "C" int ctu_flap_count(const void* skull, int u8, int N, int64_t V, int32_t* counts, void* stream) {
    CTU_REQUIRE(skull && counts, "flap_count: null pointer");
    CTU_REQUIRE(N > 0 && N <= 65535 && V > 0 && V < ((int64_t)1 << 31), "flap_count: bad shape N=%d V=%lld", N, (long long)V);
    const int nchunks = (int)ceil_div64(V, CTU_FLAP_CHUNK);
    const int vec = aligned(skull, 16) && (V * (u8 ? 1 : 4)) % 16 == 0;
    flap_count_kernel<<<dim3(nchunks, N), AB, 0, (hipStream_t)stream>>>(skull, u8 ? 1 : 0, V, nchunks, vec, counts);
    CTU_CHECK_LAUNCH("flap_count");
    return CTU_OK;
}

extern "C" int ctu_flap_draw(const void* skull, int u8, int N, int D, int H, int W, const int32_t* counts, int mode,
                             const int64_t* hole_seq, uint64_t hole_seed, float p_hole, int size_lo, int size_hi,
                             int shapes, const int64_t* noise_seq, const float* noise_nd, uint64_t noise_seed,
                             float p_noise, float salt_ratio, int decay, int32_t* params, void* stream) {
    if (int e = check_shape(N, D, H, W)) return e;
    CTU_REQUIRE(params && mode >= 1 && mode <= 3, "flap_draw: null params or bad mode %d", mode);
    CTU_REQUIRE(!(mode & CTU_FLAP_HOLE) || (skull && counts && hole_seq), "flap_draw: hole needs skull, counts, counter");
    CTU_REQUIRE(!(mode & CTU_FLAP_NOISE) || (noise_seq && noise_nd), "flap_draw: noise needs counter and density");
    CTU_REQUIRE(N <= 65535, "flap_draw: batch %d too large", N);
    if (mode & CTU_FLAP_HOLE) {
        const int nsh = shapes & 3;
        CTU_REQUIRE(nsh >= 1, "flap_draw: empty shape list");
        for (int i = 0; i < nsh; ++i) CTU_REQUIRE(((shapes >> (2 + 2 * i)) & 3) <= CTU_FLAP_FLAP, "flap_draw: bad shape code");
        CTU_REQUIRE(size_hi > size_lo, "flap_draw: empty size range [%d, %d)", size_lo, size_hi);
    }
    DrawArgs a;
    a.skull = skull;
    a.u8 = u8 ? 1 : 0;
    a.N = N; a.D = D; a.H = H; a.W = W;
    a.nchunks = (int)ceil_div64((int64_t)D * H * W, CTU_FLAP_CHUNK);
    a.mode = mode; a.decay = decay ? 1 : 0;
    a.size_lo = size_lo; a.size_hi = size_hi; a.shapes = shapes;
    a.counts = counts; a.hole_seq = hole_seq; a.noise_seq = noise_seq; a.noise_nd = noise_nd;
    a.hk0 = (uint32_t)hole_seed; a.hk1 = (uint32_t)(hole_seed >> 32);
    a.nk0 = (uint32_t)noise_seed; a.nk1 = (uint32_t)(noise_seed >> 32);
    a.p_hole = p_hole; a.p_noise = p_noise; a.salt_ratio = salt_ratio;
    a.params = params;
    flap_draw_kernel<<<N, AB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("flap_draw");
    return CTU_OK;
}

extern "C" int ctu_flap_apply(const void* skull, int u8, const float* atlas, int N, int D, int H, int W,
                              const int32_t* params, int mode, int64_t* hole_seq, int64_t* noise_seq, float* noise_nd,
                              uint64_t noise_seed, int decay, float* x, int C, float* full, float* flap, void* stream) {
    if (int e = check_shape(N, D, H, W)) return e;
    CTU_REQUIRE(skull && params && x, "flap_apply: null pointer");
    CTU_REQUIRE(mode >= 1 && mode <= 3, "flap_apply: bad mode %d", mode);
    CTU_REQUIRE(!(mode & CTU_FLAP_HOLE) || hole_seq, "flap_apply: hole needs its counter");
    CTU_REQUIRE(!(mode & CTU_FLAP_NOISE) || (noise_seq && noise_nd), "flap_apply: noise needs counter and density");
    CTU_REQUIRE(C == 1 || C == 2, "flap_apply: %d input channels (1, or 2 with the atlas)", C);
    CTU_REQUIRE((C == 2) == (atlas != nullptr), "flap_apply: the second input channel is the atlas");
    ApplyArgs a;
    a.skull = skull; a.atlas = atlas; a.params = params;
    a.hole_seq = hole_seq; a.noise_seq = noise_seq; a.noise_nd = noise_nd;
    a.x = x; a.full = full; a.flap = flap;
    a.u8 = u8 ? 1 : 0;
    a.N = N; a.D = D; a.H = H; a.W = W; a.C = C;
    a.mode = mode; a.decay = decay ? 1 : 0;
    a.vec = quad_vec(skull, a.u8, atlas, W, x, full, flap);
    a.nk0 = (uint32_t)noise_seed; a.nk1 = (uint32_t)(noise_seed >> 32);
    const int64_t quads = (int64_t)N * D * H * ((W + 3) / 4);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(quads, AB), 2048));
    flap_apply_kernel<<<grid, AB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("flap_apply");
    return CTU_OK;
}
