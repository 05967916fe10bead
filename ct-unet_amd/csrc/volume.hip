// Whole-volume helpers either side of the patch path, gfx950: patch tiling + stitching of skull volumes
// (BASELINE config 4: "skull volumes tiled to 192^3 patches").  Index work on NCDHW volumes: HBM-bound streaming.  The
// Hausdorff metric of the inference tail (ctu_hausdorff) lives in surface.hip with the other surface metrics.
//
// Replaces: nothing in the reference: its datasets feed whole pre-resized volumes (ctunet/pytorch/datasets.py:89-112,
//           195-235); the tiles carry the same sample schema.
#include "common.h"

namespace {

constexpr int VB = 256;

// ------------------------------------------------------------------------------------------------ tiling
// out[p][c][z][y][x] = vol[c][z0+z][y0+y][x0+x], zero outside the volume (volumes smaller than a patch)
__global__ void extract_patches_kernel(const float* __restrict__ vol, const int32_t* __restrict__ coords, int P, int C, int D,
                                       int H, int W, int pd, int ph, int pw, float* __restrict__ out) {
    const int64_t pv = (int64_t)pd * ph * pw;
    const int64_t total = (int64_t)P * C * pv;
    for (int64_t idx = (int64_t)blockIdx.x * VB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * VB) {
        const int64_t v = idx % pv;
        const int c = (int)((idx / pv) % C), p = (int)(idx / (pv * C));
        const int x = (int)(v % pw), y = (int)((v / pw) % ph), z = (int)(v / ((int64_t)pw * ph));
        const int gz = coords[p * 3] + z, gy = coords[p * 3 + 1] + y, gx = coords[p * 3 + 2] + x;
        float r = 0.f;
        if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) r = vol[(((int64_t)c * D + gz) * H + gy) * W + gx];
        out[idx] = r;
    }
}

// gather form (no atomics, fixed patch order => bitwise reproducible): out[c][v] = mean over the patches that cover v
__global__ void stitch_kernel(const float* __restrict__ patches, const int32_t* __restrict__ coords, int P, int C, int D, int H,
                              int W, int pd, int ph, int pw, float* __restrict__ out) {
    const int64_t V = (int64_t)D * H * W, pv = (int64_t)pd * ph * pw;
    const int64_t total = (int64_t)C * V;
    for (int64_t idx = (int64_t)blockIdx.x * VB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * VB) {
        const int64_t v = idx % V;
        const int c = (int)(idx / V);
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((int64_t)W * H));
        float s = 0.f;
        int cnt = 0;
        for (int p = 0; p < P; ++p) {
            const int lz = z - coords[p * 3], ly = y - coords[p * 3 + 1], lx = x - coords[p * 3 + 2];
            if (lz >= 0 && lz < pd && ly >= 0 && ly < ph && lx >= 0 && lx < pw) {
                s += patches[((int64_t)p * C + c) * pv + ((int64_t)lz * ph + ly) * pw + lx];
                ++cnt;
            }
        }
        out[idx] = cnt ? s / (float)cnt : 0.f;
    }
}

}  // namespace

extern "C" int ctu_extract_patches(const float* vol, const int32_t* coords, int P, int C, int D, int H, int W, int pd, int ph,
                                   int pw, float* out, void* stream) {
    CTU_REQUIRE(vol && coords && out, "extract_patches: null pointer");
    CTU_REQUIRE(P > 0 && C > 0 && D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "extract_patches: bad shape");
    const int64_t total = (int64_t)P * C * pd * ph * pw;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64(total, VB), 1 << 20);
    extract_patches_kernel<<<grid, VB, 0, (hipStream_t)stream>>>(vol, coords, P, C, D, H, W, pd, ph, pw, out);
    CTU_CHECK_LAUNCH("extract_patches");
    return CTU_OK;
}

extern "C" int ctu_stitch_patches(const float* patches, const int32_t* coords, int P, int C, int D, int H, int W, int pd, int ph,
                                  int pw, float* out, void* stream) {
    CTU_REQUIRE(patches && coords && out, "stitch_patches: null pointer");
    CTU_REQUIRE(P > 0 && C > 0 && D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0, "stitch_patches: bad shape");
    const int64_t total = (int64_t)C * D * H * W;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64(total, VB), 1 << 20);
    stitch_kernel<<<grid, VB, 0, (hipStream_t)stream>>>(patches, coords, P, C, D, H, W, pd, ph, pw, out);
    CTU_CHECK_LAUNCH("stitch_patches");
    return CTU_OK;
}
