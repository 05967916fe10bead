// Binary morphology of 3-D masks on bit images, gfx950: erosion, dilation, opening, closing with any 3x3x3 structure, and
// the implant mask of the double-output nets (definitions: ctunet_amd/postprocess.py; scipy.ndimage's, bit for bit).
//
// A call is pack -> steps -> unpack, one launch each, no host synchronisation and no atomics:
//   1. pack:   the label map is read once (16-byte loads where aligned) into a bit image, one bit per voxel along x, 64
//              voxels per uint64 (bit i of word w = voxel x = 64 w + i), rows padded to whole words, the padding bits set
//              to the border value.  The foreground test (nonzero, == label, or full != 0 && defective == 0) happens
//              here: a thread tests 16 voxels, four neighbouring lanes combine their 16 bits with two shuffles.
//   2. steps:  out[v] = AND / OR over the structure's set offsets of in[v + s] (dilation: the reflected structure).  y / z
//              offsets are neighbouring rows, x offsets funnel shifts across the neighbouring word, everything outside
//              the volume is the border constant.  One block loads an 8 x 16 rows x 8 words tile plus a halo of t rows and
//              planes and one word each side in x into LDS and applies up to t = 4 steps there (temporal blocking: the
//              valid region shrinks by one row per step; a wrong bit entering a halo word's far end needs 64 steps to
//              reach the tile), ping-ponging between two LDS copies, then writes the tile.  The steps of one launch may
//              change operation once, so opening x2 (2 erosions + 2 dilations) is one launch.  Launches ping-pong between
//              the two bit images of the workspace.
//   3. unpack: one byte per voxel, 16-byte stores where aligned.
// By construction a call reads the label map once and writes the output once; the bit images are 1/8 byte per voxel (7.3 MB
// at 224x512x512).  Measured times per kernel: profiles/morphology.md (HBM bytes and cache residency were not read from
// counters; the tile and MT were not chosen from a sweep).
//
// Replaces: erode / dilate / ErodeDilate of ctunet/pytorch/transforms.py:97-127,356-377 (SimpleITK on the host; its ball
// convention is not pinned here, scipy.ndimage's 3x3x3 structures are).
#include "common.h"
#include "voxel_rows.h"

namespace {

using ctu_vox::Foreground;
using ctu_vox::mask16;
using ctu_vox::store_mask16;

typedef unsigned long long u64;

#ifndef CTU_MORPH_MT                                            // dev A/B: make EXTRA=-DCTU_MORPH_MT=2 (profiles/morphology.md)
#define CTU_MORPH_MT 4
#endif
constexpr int MT = CTU_MORPH_MT;                               // steps per launch
constexpr int TZ = 8, TY = 16, TXW = 8;                        // tile: planes, rows, words
constexpr int LZ = TZ + 2 * MT, LY = TY + 2 * MT, LX = TXW + 2;
constexpr int LW = LZ * LY * LX;                               // 3840 words = 30 KB per copy
constexpr int SB = 256;
constexpr int MAX_ITER = 64;
constexpr int MODE_ERODE = CTU_MORPH_ERODE, MODE_OPEN = CTU_MORPH_OPEN, MODE_CLOSE = CTU_MORPH_CLOSE;
constexpr int WS_MORPH = CTU_MORPH_WS_MORPH, WS_FILL = CTU_MORPH_WS_FILL, WS_IMPLANT = CTU_MORPH_WS_IMPLANT;
constexpr uint32_t CODE_ALL = (1u << 27) - 1;

struct None {};                                                // no second input: no voxel of it is set
template <class Pred> __device__ __forceinline__ uint32_t mask16(const None*, int, Pred) { return 0; }

// ------------------------------------------------------------------------------------------------ 1. pack
// thread (row, q): voxels x = 16 q .. 16 q + 15 of one row; lanes 4 j .. 4 j + 3 share word q / 4
template <class TA, class TB>
__global__ void __launch_bounds__(SB) morph_pack_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int64_t V,
                                                        int64_t rows, int W, int WW, int has_label, long long label,
                                                        int border, u64* __restrict__ bits) {
    const int n = blockIdx.y;
    const int qr = WW * 4;
    const int64_t gid = (int64_t)blockIdx.x * SB + threadIdx.x;
    const int64_t row = gid / qr;
    const int q = (int)(gid - row * qr);
    const bool live = row < rows;
    const int x0 = q * 16;
    const int nv = live ? max(0, min(W - x0, 16)) : 0;
    uint32_t m = 0;
    if (nv) {
        const int64_t off = n * V + row * W + x0;
        m = mask16(a + off, nv, Foreground{has_label, label});
        m &= ~mask16(b + off, nv, Foreground{0, 0});
    }
    if (border && nv < 16) m |= (0xffffu << nv) & 0xffffu;      // padding bits carry the border value
    u64 w = (u64)m << (16 * (q & 3));
    w |= __shfl_xor(w, 1);
    w |= __shfl_xor(w, 2);
    if (live && (q & 3) == 0) bits[(n * rows + row) * WW + (q >> 2)] = w;
}

// ------------------------------------------------------------------------------------------------ 3. unpack
__global__ void __launch_bounds__(SB) morph_unpack_kernel(const u64* __restrict__ bits, int64_t V, int64_t rows, int W,
                                                          int WW, uint8_t* __restrict__ out) {
    const int n = blockIdx.y;
    const int qr = WW * 4;
    const int64_t gid = (int64_t)blockIdx.x * SB + threadIdx.x;
    const int64_t row = gid / qr;
    if (row >= rows) return;
    const int q = (int)(gid - row * qr);
    const int x0 = q * 16;
    const int nv = min(W - x0, 16);
    if (nv <= 0) return;
    const uint32_t m = (uint32_t)(bits[(n * rows + row) * WW + (q >> 2)] >> (16 * (q & 3))) & 0xffffu;
    store_mask16(out + n * V + row * W + x0, nv, m);
}

// ------------------------------------------------------------------------------------------------ 2. steps
struct StepArgs {
    int D, H, W, WW;
    int ntx, nty;                   // tiles along x (words) and y
    int t, nA;                      // steps of this launch (1..MT); the first nA use A, the rest B
    uint32_t codeA, codeB;          // bit (i*3+j)*3+k: the step reads in[v + (i-1, j-1, k-1)]
    int andA, andB;                 // 1: AND (erosion), 0: OR (dilation)
    int border;
};

__device__ __forceinline__ u64 step_word(const u64* __restrict__ src, int a, int b, int c, uint32_t code, bool is_and, u64 bw) {
    u64 acc = is_and ? ~0ull : 0ull;
#pragma unroll
    for (int zy = 0; zy < 9; ++zy) {
        const uint32_t m = (code >> (3 * zy)) & 7u;
        if (!m) continue;                                       // block-uniform
        const u64* p = src + ((a + zy / 3 - 1) * LY + (b + zy % 3 - 1)) * LX + c;
        const u64 cw = p[0];
        if (m & 2u) acc = is_and ? acc & cw : acc | cw;
        if (m & 1u) {                                           // x - 1
            const u64 l = c > 0 ? p[-1] : bw;
            const u64 v = (cw << 1) | (l >> 63);
            acc = is_and ? acc & v : acc | v;
        }
        if (m & 4u) {                                           // x + 1
            const u64 r = c < LX - 1 ? p[1] : bw;
            const u64 v = (cw >> 1) | (r << 63);
            acc = is_and ? acc & v : acc | v;
        }
    }
    return acc;
}

__global__ void __launch_bounds__(SB) morph_step_kernel(StepArgs s, const u64* __restrict__ in, u64* __restrict__ out) {
    __shared__ u64 buf[2][LW];
    const int n = blockIdx.y;
    int bi = blockIdx.x;
    const int tx = bi % s.ntx;
    bi /= s.ntx;
    const int ty = bi % s.nty, tz = bi / s.nty;
    const int t = s.t;
    const int z0 = tz * TZ - t, y0 = ty * TY - t, w0 = tx * TXW - 1;    // volume coordinates of local (0, 0, 0)
    const int lz = TZ + 2 * t, ly = TY + 2 * t;
    const u64 bw = s.border ? ~0ull : 0ull;
    const int64_t item = (int64_t)n * s.D * s.H * s.WW;
    const u64* src_g = in + item;
    const int nloc = lz * ly * LX;
    for (int i = threadIdx.x; i < nloc; i += SB) {
        const int c = i % LX, r = i / LX;
        const int b = r % ly, a = r / ly;
        const int z = z0 + a, y = y0 + b, w = w0 + c;
        const bool inside = z >= 0 && z < s.D && y >= 0 && y < s.H && w >= 0 && w < s.WW;
        const int li = (a * LY + b) * LX + c;
        buf[0][li] = inside ? src_g[((int64_t)z * s.H + y) * s.WW + w] : bw;
        buf[1][li] = bw;                                        // positions outside the volume stay the border in both
    }
    __syncthreads();
    const int tail = s.W & 63;
    const u64 vmask = tail ? (1ull << tail) - 1 : ~0ull;        // voxel bits of a row's last word
    int cur = 0;
    for (int k = 1; k <= t; ++k) {
        const bool first = k <= s.nA;
        const uint32_t code = first ? s.codeA : s.codeB;
        const bool is_and = (first ? s.andA : s.andB) != 0;
        const int rz = lz - 2 * k, ry = ly - 2 * k;             // rows still exact after k steps
        const int nreg = rz * ry * LX;
        const u64* src = buf[cur];
        u64* dst = buf[cur ^ 1];
        for (int i = threadIdx.x; i < nreg; i += SB) {
            const int c = i % LX, r = i / LX;
            const int b = k + r % ry, a = k + r / ry;
            const int z = z0 + a, y = y0 + b, w = w0 + c;
            if (z < 0 || z >= s.D || y < 0 || y >= s.H || w < 0 || w >= s.WW) continue;
            u64 v = step_word(src, a, b, c, code, is_and, bw);
            if (w == s.WW - 1) v = (v & vmask) | (bw & ~vmask);
            dst[(a * LY + b) * LX + c] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
    u64* dst_g = out + item;
    const u64* res = buf[cur];
    for (int i = threadIdx.x; i < TZ * TY * TXW; i += SB) {
        const int c = i % TXW, r = i / TXW;
        const int b = r % TY, a = r / TY;
        const int z = tz * TZ + a, y = ty * TY + b, w = tx * TXW + c;
        if (z < s.D && y < s.H && w < s.WW) dst_g[((int64_t)z * s.H + y) * s.WW + w] = res[((a + t) * LY + b + t) * LX + c + 1];
    }
}

// ------------------------------------------------------------------------------------------------ host
size_t bit_image_bytes(int N, int D, int H, int W) { return align256((size_t)N * D * H * ceil_div(W, 64) * 8); }

uint32_t reflect(uint32_t code) {
    uint32_t r = 0;
    for (int i = 0; i < 27; ++i) r |= ((code >> i) & 1u) << (26 - i);
    return r;
}

template <class TA, class TB>
int launch_pack(const void* a, const void* b, int N, int D, int H, int W, int has_label, long long label, int border,
                u64* bits, hipStream_t st) {
    const int WW = ceil_div(W, 64);
    const int64_t rows = (int64_t)D * H;
    const dim3 grid((unsigned)ceil_div64(rows * WW * 4, SB), (unsigned)N);
    morph_pack_kernel<TA, TB><<<grid, SB, 0, st>>>((const TA*)a, (const TB*)b, (int64_t)D * H * W, rows, W, WW, has_label,
                                                    label, border, bits);
    CTU_CHECK_LAUNCH("morphology pack");
    return CTU_OK;
}

int launch_unpack(const u64* bits, int N, int D, int H, int W, uint8_t* out, hipStream_t st) {
    const int WW = ceil_div(W, 64);
    const int64_t rows = (int64_t)D * H;
    const dim3 grid((unsigned)ceil_div64(rows * WW * 4, SB), (unsigned)N);
    morph_unpack_kernel<<<grid, SB, 0, st>>>(bits, (int64_t)D * H * W, rows, W, WW, out);
    CTU_CHECK_LAUNCH("morphology unpack");
    return CTU_OK;
}

// `iterations` steps of each operation of `mode` from bit image b[0], MT steps per launch; *res = the image holding the result
int run_steps(int mode, uint32_t code, int iterations, int border, int N, int D, int H, int W, u64* b[2], int* res,
              hipStream_t st) {
    const bool two = mode == MODE_OPEN || mode == MODE_CLOSE;
    const bool and_first = mode == MODE_ERODE || mode == MODE_OPEN;
    const int total = two ? 2 * iterations : iterations;
    StepArgs s;
    s.D = D; s.H = H; s.W = W; s.WW = ceil_div(W, 64);
    s.ntx = ceil_div(s.WW, TXW); s.nty = ceil_div(H, TY);
    s.border = border;
    const dim3 grid((unsigned)(s.ntx * s.nty * ceil_div(D, TZ)), (unsigned)N);
    int cur = 0;
    for (int done = 0; done < total; done += MT) {
        s.t = total - done < MT ? total - done : MT;
        // steps done .. done + t - 1: step i is the first operation iff i < iterations
        const bool a_first = done < iterations;
        s.nA = a_first ? (iterations - done < s.t ? iterations - done : s.t) : s.t;
        s.andA = (a_first ? and_first : !and_first) ? 1 : 0;
        s.andB = s.andA ^ 1;
        s.codeA = s.andA ? code : reflect(code);
        s.codeB = s.andB ? code : reflect(code);
        morph_step_kernel<<<grid, SB, 0, st>>>(s, b[cur], b[cur ^ 1]);
        CTU_CHECK_LAUNCH("morphology step");
        cur ^= 1;
    }
    *res = cur;
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_morphology_ws_bytes(int N, int D, int H, int W, int kind) {
    if (!geometry_ok(N, D, H, W) || kind < WS_MORPH || kind > WS_IMPLANT) return 0;
    const size_t images = 2 * bit_image_bytes(N, D, H, W);
    const size_t fill = align256(ctu_components_ws_bytes(N, D, H, W)) + align256((size_t)N * D * H * W);
    return kind == WS_MORPH ? images : kind == WS_FILL ? fill : images + fill;
}

extern "C" int ctu_binary_morphology(const void* in, int dtype, int N, int D, int H, int W, int mode, uint32_t structure,
                                     int iterations, int border, int has_label, int64_t label, uint8_t* out, void* ws,
                                     void* stream) {
    CTU_REQUIRE(in && out && ws, "binary_morphology: null pointer");
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64, "binary_morphology: unsupported dtype %d (uint8 or int64)", dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "binary_morphology: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)",
                N, D, H, W);
    CTU_REQUIRE(mode >= MODE_ERODE && mode <= MODE_CLOSE, "binary_morphology: unknown mode %d", mode);
    CTU_REQUIRE(structure != 0 && structure <= CODE_ALL, "binary_morphology: structure must be a nonzero 27-bit code, got %u",
                structure);
    CTU_REQUIRE(iterations >= 1 && iterations <= MAX_ITER, "binary_morphology: iterations must lie in 1..%d, got %d",
                MAX_ITER, iterations);
    CTU_REQUIRE(border == 0 || border == 1, "binary_morphology: border value must be 0 or 1, got %d", border);
    hipStream_t st = (hipStream_t)stream;
    u64* b[2] = {(u64*)ws, (u64*)((uint8_t*)ws + bit_image_bytes(N, D, H, W))};
    int rc = dtype == CTU_U8 ? launch_pack<uint8_t, None>(in, nullptr, N, D, H, W, has_label != 0, label, border, b[0], st)
                             : launch_pack<long long, None>(in, nullptr, N, D, H, W, has_label != 0, label, border, b[0], st);
    if (rc != CTU_OK) return rc;
    int res;
    rc = run_steps(mode, structure, iterations, border, N, D, H, W, b, &res, st);
    if (rc != CTU_OK) return rc;
    return launch_unpack(b[res], N, D, H, W, out, st);
}

extern "C" int ctu_implant_mask(const void* full, int full_dtype, const void* defective, int defective_dtype, int N, int D,
                                int H, int W, uint32_t structure, int opening_iterations, int fill_holes, int connectivity,
                                int num_components, uint8_t* out, void* ws, void* stream) {
    CTU_REQUIRE(full && defective && out && ws, "implant_mask: null pointer");
    CTU_REQUIRE((full_dtype == CTU_U8 || full_dtype == CTU_I64) && (defective_dtype == CTU_U8 || defective_dtype == CTU_I64),
                "implant_mask: unsupported dtype %d / %d (uint8 or int64)", full_dtype, defective_dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "implant_mask: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)", N, D,
                H, W);
    CTU_REQUIRE(structure != 0 && structure <= CODE_ALL, "implant_mask: structure must be a nonzero 27-bit code, got %u",
                structure);
    CTU_REQUIRE(opening_iterations >= 0 && opening_iterations <= MAX_ITER,
                "implant_mask: opening iterations must lie in 0..%d, got %d", MAX_ITER, opening_iterations);
    CTU_REQUIRE(connectivity >= 1 && connectivity <= 3, "implant_mask: connectivity must be 1, 2 or 3, got %d", connectivity);
    CTU_REQUIRE(num_components >= 1 && num_components <= 8, "implant_mask: num_components must lie in 1..8, got %d",
                num_components);
    hipStream_t st = (hipStream_t)stream;
    const size_t image = bit_image_bytes(N, D, H, W);
    u64* b[2] = {(u64*)ws, (u64*)((uint8_t*)ws + image)};
    void* cws = (uint8_t*)ws + 2 * image;
    int rc;
    if (full_dtype == CTU_U8)
        rc = defective_dtype == CTU_U8 ? launch_pack<uint8_t, uint8_t>(full, defective, N, D, H, W, 0, 0, 0, b[0], st)
                                       : launch_pack<uint8_t, long long>(full, defective, N, D, H, W, 0, 0, 0, b[0], st);
    else
        rc = defective_dtype == CTU_U8 ? launch_pack<long long, uint8_t>(full, defective, N, D, H, W, 0, 0, 0, b[0], st)
                                       : launch_pack<long long, long long>(full, defective, N, D, H, W, 0, 0, 0, b[0], st);
    if (rc != CTU_OK) return rc;
    int res = 0;
    if (opening_iterations > 0) {
        rc = run_steps(MODE_OPEN, structure, opening_iterations, 0, N, D, H, W, b, &res, st);
        if (rc != CTU_OK) return rc;
    }
    rc = launch_unpack(b[res], N, D, H, W, out, st);
    if (rc != CTU_OK) return rc;
    if (fill_holes) {
        rc = ctu_fill_holes(out, CTU_U8, N, D, H, W, 1, 0, 0, out, cws, st);
        if (rc != CTU_OK) return rc;
    }
    return ctu_filter_components(out, CTU_U8, N, D, H, W, connectivity, nullptr, 0, CTU_CC_LARGEST, num_components, out, cws, st);
}
