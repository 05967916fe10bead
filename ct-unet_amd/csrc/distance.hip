// Exact Euclidean distance transform of 3-D masks, gfx950: distance, squared distance, signed distance, nearest-site
// indices and the ball threshold behind ball erosion / dilation (definitions: ctunet_amd/postprocess.py; pinned on
// scipy.ndimage.distance_transform_edt).
//
// The sites are the background voxels (invert: the foreground voxels); every voxel gets the distance to its nearest site.
//   1. x pass:  one wave per image row reads the foreground (nonzero or == label) of the map as one 16-bit mask per lane
//               (mask16 of voxel_rows.h) and writes the 1-D squared distance to the nearest site of the row (row_nearest of
//               edt_line.h); with indices, the nearest site's x as int16.  The signed map needs both transforms: the x pass
//               writes both planes from the one membership mask it has read.
//   2. y, z:    one lane per line, lanes at consecutive x (coalesced), the lower envelope of edt_line.h with its stack in
//               LDS, in place; with indices, the chosen y / z as int16.
//   3. finish:  the virtual border, sqrt, sign, threshold and the index gather iz = zsel[v], iy = ysel[iz, y, x],
//               ix = xsel[iz, iy, x]; 16-byte loads and stores where the addresses are aligned, scalar otherwise.
// The 4-byte maps live in `out` itself wherever out has 4 bytes per voxel (the finish kernel rewrites it in place); only the
// second plane of the signed map and the plane behind the 1-byte ball result need workspace.
// Unit spacing: int32 squared distances, exact.  Otherwise fp32 sum (k_i s_i)^2, as surface.hip.
// Virtual border (border_background): the voxels outside the volume are sites.  The nearest of them lies straight across
// the nearest face, so the finish kernel takes min(d2, min_axis ((min(k, L - 1 - k) + 1) s)^2): no line pass sees it.
// An item without any site (and no virtual border) gets +inf / INT32_MAX and indices -1.
// Limits: every side <= 1024 (the x pass gives a lane 16 voxels; a line pass stacks 6 bytes per element of a line in LDS,
// 1365 elements at 8 lanes per block), D*H*W < 2^31, N <= 65535.
// No host synchronisation, allocation or copy and no atomics: capture-safe and bitwise reproducible.
//
// Replaces: nothing in the reference (its erode / dilate go through SimpleITK balls on the host,
//           ctunet/pytorch/transforms.py:97-127); users would call scipy.ndimage.distance_transform_edt on the CPU.
#include "common.h"
#include "edt_line.h"

namespace {

using namespace ctu_edt;
using namespace ctu_vox;

constexpr int XB = 256;                 // x pass block: 4 waves, one row per wave
constexpr int FB = 256;                 // finish block
constexpr int MAXG = 64;                // items per launch with a spacing table in the kernel arguments
constexpr int MAXU = 32768;             // items per launch at unit spacing (grid.y)
constexpr int KIND_DIST = CTU_DIST_EDT, KIND_SQ = CTU_DIST_SQUARED, KIND_SIGNED = CTU_DIST_SIGNED, KIND_BALL = CTU_DIST_BALL;

struct DArgs {
    const void* in;
    int dtype, has_label;
    long long label;
    int D, H, W;
    int n0;                             // first item of this launch (blockIdx.y counts from it)
    int invert, both;                   // both: plane 0 = sites background, plane 1 = sites foreground
    int border;
    float r2;
    float sp[MAXG][3];                  // (z, y, x) spacing of each item of the launch (read at non-unit spacing only)
};

// ------------------------------------------------------------------------------------------------ 1. x pass
template <bool FLT, bool TRACK>
__global__ void __launch_bounds__(XB) dist_x_kernel(DArgs a, void* __restrict__ p0, void* __restrict__ p1,
                                                    int16_t* __restrict__ xsel) {
    typedef typename DistT<FLT>::T T;
    const int lane = threadIdx.x & 63;
    const int il = blockIdx.y;
    const int D = a.D, H = a.H, W = a.W;
    const int64_t V = (int64_t)D * H * W;
    const int64_t item = (int64_t)(a.n0 + il) * V;
    float sx2 = 1.f;
    if (FLT) sx2 = a.sp[il][2] * a.sp[il][2];
    const int x0 = lane * 16;
    const int nv = min(max(W - x0, 0), 16);
    const uint32_t valid = (1u << nv) - 1u;
    const int nrows = D * H;
    const int nwaves = gridDim.x * (XB / 64);
    const int nsides = a.both ? 2 : 1;
    const Foreground fg{a.has_label, a.label};
    for (int r = blockIdx.x * (XB / 64) + (threadIdx.x >> 6); r < nrows; r += nwaves) {    // wave-uniform
        const int64_t vrow = item + (int64_t)r * W + x0;
        uint32_t m = 0;
        if (nv) {
            m = a.dtype == CTU_U8 ? mask16((const uint8_t*)a.in + vrow, nv, fg) : mask16((const long long*)a.in + vrow, nv, fg);
        }
        for (int s = 0; s < nsides; ++s) {
            const int inv = a.both ? s : a.invert;
            const uint32_t es = inv ? m : (~m & valid);            // the sites of this lane's voxels
            T val[16];
            int16_t pos[16];
            row_nearest<FLT, TRACK>(es, x0, lane, sx2, val, pos);
            if (nv) {
                store16((T*)(s ? p1 : p0) + vrow, nv, val);
                if (TRACK) store16(xsel + vrow, nv, pos);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2. y / z passes
// blockIdx.x = o * nbx + x block, blockIdx.y = item of the launch, blockIdx.z = plane; the line of lane x starts at
// o * ostride + x of its item.  Dynamic LDS: 6 L blockDim.x bytes (edt_line.h).
template <bool FLT, bool TRACK>
__global__ void dist_line_kernel(DArgs a, void* __restrict__ p0, void* __restrict__ p1, int16_t* __restrict__ sel, int L,
                                 int64_t lstride, int64_t ostride, int nbx, int axis) {
    typedef typename DistT<FLT>::T T;
    extern __shared__ uint8_t smem[];
    const int NL = blockDim.x, lane = threadIdx.x;
    T* Fs = reinterpret_cast<T*>(smem);
    uint16_t* Vs = reinterpret_cast<uint16_t*>(Fs + (size_t)L * NL);
    const int il = blockIdx.y;
    const int xb = blockIdx.x % nbx, o = blockIdx.x / nbx;
    const int x = xb * NL + lane;
    if (x >= a.W) return;                 // no barriers below
    T s2 = (T)1;
    if (FLT) { const float sp = a.sp[il][axis]; s2 = (T)(sp * sp); }
    const int64_t off = (int64_t)(a.n0 + il) * a.D * a.H * a.W + (int64_t)o * ostride + x;
    T* d = (T*)(blockIdx.z ? p1 : p0) + off;
    edt_line<FLT, TRACK>(d, L, lstride, s2, Fs, Vs, NL, lane, TRACK ? sel + off : nullptr);
}

// ------------------------------------------------------------------------------------------------ 3. finish
template <bool FLT> __device__ __forceinline__ float key_d2(uint32_t k) {      // squared distance as a float, +inf = none
    if (FLT) return __uint_as_float(k);
    return (int)k == INF_I ? __builtin_inff() : (float)(int)k;                 // exact below 2^24 (3 * 1023^2 is)
}
template <bool FLT> __device__ __forceinline__ float key_dist(uint32_t k) {
    if (FLT) return sqrtf(__uint_as_float(k));
    const int n = (int)k;
    if (n == INF_I) return __builtin_inff();
    return n < (1 << 24) ? sqrtf((float)n) : (float)sqrt((double)n);
}

// VPT flat-consecutive voxels of one item per thread: 4 where out has 4 bytes per voxel, 16 for the 1-byte ball result.
// src0 / src1: the planes of squared distances (KIND_SIGNED: sites background / foreground; otherwise src0 only).  out may be
// one of them: a thread reads its voxels before it writes them and no other thread touches them.
template <bool FLT, int KIND>
__global__ void __launch_bounds__(FB) dist_finish_kernel(DArgs a, const uint32_t* src0, const uint32_t* src1, void* out,
                                                         const int16_t* __restrict__ xsel, const int16_t* __restrict__ ysel,
                                                         const int16_t* __restrict__ zsel, int32_t* __restrict__ indices) {
    constexpr int VPT = KIND == KIND_BALL ? 16 : 4;
    const int il = blockIdx.y;
    const int n = a.n0 + il;
    const int H = a.H, W = a.W;
    const int64_t V = (int64_t)a.D * H * W;
    const int64_t v0 = ((int64_t)blockIdx.x * FB + threadIdx.x) * VPT;
    if (v0 >= V) return;
    const int nv = (int)min((int64_t)VPT, V - v0);
    const int64_t base = (int64_t)n * V + v0;
    uint32_t k0[VPT], k1[VPT];
    auto load = [&](const uint32_t* sp, uint32_t* k) {
        if (nv == VPT && ((uintptr_t)sp & 15) == 0) {
#pragma unroll
            for (int j = 0; j < VPT / 4; ++j) {
                const uint4 w = reinterpret_cast<const uint4*>(sp)[j];
                k[4 * j] = w.x; k[4 * j + 1] = w.y; k[4 * j + 2] = w.z; k[4 * j + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int u = 0; u < VPT; ++u) k[u] = u < nv ? sp[u] : 0u;
        }
    };
    load(src0 + base, k0);
    if (KIND == KIND_SIGNED) load(src1 + base, k1);
    // coordinates of the first voxel; the others follow by carrying
    int x = (int)(v0 % W);
    const int64_t row = v0 / W;
    int y = (int)(row % H), z = (int)(row / H);
    float sz2 = 1.f, sy2 = 1.f, sx2 = 1.f;
    if (FLT) { sz2 = a.sp[il][0] * a.sp[il][0]; sy2 = a.sp[il][1] * a.sp[il][1]; sx2 = a.sp[il][2] * a.sp[il][2]; }
    uint32_t res[VPT];
    int32_t iz[VPT], iy[VPT], ix[VPT];
    uint32_t ballbits = 0;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        uint32_t key = k0[u];
        if (a.border) {                                       // the nearest voxel outside the volume: across the nearest face
            const int mz = min(z, a.D - 1 - z) + 1, my = min(y, H - 1 - y) + 1, mx = min(x, W - 1 - x) + 1;
            if (FLT) {
                const float b = fminf(fminf(sz2 * (float)(mz * mz), sy2 * (float)(my * my)), sx2 * (float)(mx * mx));
                key = __float_as_uint(fminf(__uint_as_float(key), b));
            } else {
                const int m = min(min(mz, my), mx);
                key = (uint32_t)min((int)key, m * m);
            }
        }
        if (KIND == KIND_DIST) {
            res[u] = __float_as_uint(key_dist<FLT>(key));
        } else if (KIND == KIND_SQ) {
            res[u] = FLT ? key : ((int)key == INF_I ? 0x7fffffffu : key);
        } else if (KIND == KIND_SIGNED) {
            res[u] = __float_as_uint(key_dist<FLT>(k1[u]) - key_dist<FLT>(key));
        } else {
            const float d2 = key_d2<FLT>(key);
            ballbits |= (uint32_t)(a.invert ? d2 <= a.r2 : d2 > a.r2) << u;
        }
        if (indices && u < nv) {
            const int64_t ib = (int64_t)n * V;
            const int cz = zsel[ib + v0 + u];
            int cy = -1, cx = -1;
            if (cz >= 0) {
                cy = ysel[ib + ((int64_t)cz * H + y) * W + x];
                if (cy >= 0) cx = xsel[ib + ((int64_t)cz * H + cy) * W + x];
            }
            iz[u] = cz; iy[u] = cy; ix[u] = cx;
        }
        if (++x == W) { x = 0; if (++y == H) { y = 0; ++z; } }
    }
    if (KIND == KIND_BALL) {
        store_mask16((uint8_t*)out + base, nv, ballbits);
    } else {
        uint32_t* op = (uint32_t*)out + base;
        if (nv == VPT && ((uintptr_t)op & 15) == 0) {
            *reinterpret_cast<uint4*>(op) = make_uint4(res[0], res[1], res[2], res[3]);
        } else {
#pragma unroll
            for (int u = 0; u < VPT; ++u)
                if (u < nv) op[u] = res[u];
        }
        if (indices) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int32_t* src = c == 0 ? iz : c == 1 ? iy : ix;
                int32_t* ip = indices + ((int64_t)n * 3 + c) * V + v0;
                if (nv == VPT && ((uintptr_t)ip & 15) == 0) {
                    *reinterpret_cast<int4*>(ip) = make_int4(src[0], src[1], src[2], src[3]);
                } else {
#pragma unroll
                    for (int u = 0; u < VPT; ++u)
                        if (u < nv) ip[u] = src[u];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct Layout {
    size_t plane, xsel, ysel, zsel, total;
};

Layout layout(int N, int D, int H, int W, int kind, int want_indices) {
    Layout l;
    const size_t NV = (size_t)N * D * H * W;
    size_t off = 0;
    l.plane = off;
    if (kind == KIND_SIGNED || kind == KIND_BALL) off = align256(off + NV * 4);
    l.xsel = off;
    if (want_indices) off = align256(off + NV * 2);
    l.ysel = off;
    if (want_indices) off = align256(off + NV * 2);
    l.zsel = off;
    if (want_indices) off = align256(off + NV * 2);
    l.total = off ? off : 256;                                    // never 0: 0 reports invalid geometry
    return l;
}

bool shape_ok(int N, int D, int H, int W) { return geometry_ok(N, D, H, W) && sides_ok(D, H, W); }

template <bool FLT, int KIND>
int launch_finish(const DArgs& a, int np, const uint32_t* s0, const uint32_t* s1, void* out, const int16_t* xs,
                  const int16_t* ys, const int16_t* zs, int32_t* indices, hipStream_t st) {
    constexpr int VPT = KIND == KIND_BALL ? 16 : 4;
    const int64_t V = (int64_t)a.D * a.H * a.W;
    const dim3 grid((unsigned)ceil_div64(V, (int64_t)FB * VPT), (unsigned)np);
    dist_finish_kernel<FLT, KIND><<<grid, FB, 0, st>>>(a, s0, s1, out, xs, ys, zs, indices);
    CTU_CHECK_LAUNCH("distance finish");
    return CTU_OK;
}

template <bool FLT, bool TRACK>
int run_chunk(const DArgs& a, int np, int kind, void* out, int32_t* indices, uint8_t* ws, const Layout& lay, hipStream_t st) {
    const int D = a.D, H = a.H, W = a.W;
    void* plane = ws + lay.plane;
    int16_t* xs = TRACK ? (int16_t*)(ws + lay.xsel) : nullptr;
    int16_t* ys = TRACK ? (int16_t*)(ws + lay.ysel) : nullptr;
    int16_t* zs = TRACK ? (int16_t*)(ws + lay.zsel) : nullptr;
    // plane 0 / plane 1 of the passes: the signed map keeps "sites background" in the workspace and "sites foreground" in out
    void* p0 = kind == KIND_BALL || kind == KIND_SIGNED ? plane : out;
    void* p1 = kind == KIND_SIGNED ? out : nullptr;
    const unsigned sides = kind == KIND_SIGNED ? 2 : 1;

    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64((int64_t)D * H, XB / 64), 2048);
    dist_x_kernel<FLT, TRACK><<<dim3(gx, np), XB, 0, st>>>(a, p0, p1, xs);
    CTU_CHECK_LAUNCH("distance x pass");
    const int ly = line_lanes(H), lz = line_lanes(D);
    const int nby = ceil_div(W, ly), nbz = ceil_div(W, lz);
    dist_line_kernel<FLT, TRACK><<<dim3((unsigned)(D * nby), np, sides), ly, (size_t)6 * H * ly, st>>>(
        a, p0, p1, ys, H, (int64_t)W, (int64_t)H * W, nby, 1);
    CTU_CHECK_LAUNCH("distance y pass");
    dist_line_kernel<FLT, TRACK><<<dim3((unsigned)(H * nbz), np, sides), lz, (size_t)6 * D * lz, st>>>(
        a, p0, p1, zs, D, (int64_t)H * W, (int64_t)W, nbz, 0);
    CTU_CHECK_LAUNCH("distance z pass");
    const uint32_t* s0 = (const uint32_t*)p0;
    const uint32_t* s1 = (const uint32_t*)p1;
    switch (kind) {
        case KIND_DIST: return launch_finish<FLT, KIND_DIST>(a, np, s0, s1, out, xs, ys, zs, indices, st);
        case KIND_SQ:
            if (FLT && !TRACK && !a.border) return CTU_OK;         // the passes left the answer in out
            return launch_finish<FLT, KIND_SQ>(a, np, s0, s1, out, xs, ys, zs, indices, st);
        case KIND_SIGNED: return launch_finish<FLT, KIND_SIGNED>(a, np, s0, s1, out, xs, ys, zs, indices, st);
        default: return launch_finish<FLT, KIND_BALL>(a, np, s0, s1, out, xs, ys, zs, indices, st);
    }
}

}  // namespace

extern "C" size_t ctu_distance_ws_bytes(int N, int D, int H, int W, int out_kind, int want_indices) {
    if (!shape_ok(N, D, H, W) || out_kind < KIND_DIST || out_kind > KIND_BALL) return 0;
    return layout(N, D, H, W, out_kind, want_indices != 0).total;
}

extern "C" int ctu_distance_transform(const void* in, int dtype, int N, int D, int H, int W, int has_label, int64_t label,
                                      int invert, int border_background, const float* spacing, int out_kind, void* out,
                                      int32_t* indices, float ball_r2, void* ws, void* stream) {
    CTU_REQUIRE(in && out && ws, "distance_transform: null pointer");
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I64, "distance_transform: unsupported dtype %d (uint8 or int64)", dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W), "distance_transform: bad shape N=%d D=%d H=%d W=%d (every side >= 1, D*H*W < 2^31)",
                N, D, H, W);
    CTU_REQUIRE(sides_ok(D, H, W), "distance_transform: volume side above %d (shape %d %d %d)",
                MAX_SIDE, D, H, W);
    CTU_REQUIRE(out_kind >= KIND_DIST && out_kind <= KIND_BALL, "distance_transform: unknown out_kind %d", out_kind);
    CTU_REQUIRE(!indices || ((out_kind == KIND_DIST || out_kind == KIND_SQ) && !border_background),
                "distance_transform: indices go with out_kind 0 / 1 and no virtual border only");
    CTU_REQUIRE(out_kind != KIND_BALL || (ball_r2 >= 0.f && ball_r2 < __builtin_inff()),
                "distance_transform: ball_r2 must be finite and >= 0");
    bool unit = true;
    if (spacing) {
        for (int i = 0; i < 3 * N; ++i) {
            CTU_REQUIRE(spacing[i] > 0.f && spacing[i] < __builtin_inff(), "distance_transform: spacing must be positive and finite");
            unit = unit && spacing[i] == 1.f;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const Layout lay = layout(N, D, H, W, out_kind, indices != nullptr);
    DArgs a;
    a.in = in; a.dtype = dtype; a.has_label = has_label != 0; a.label = label;
    a.D = D; a.H = H; a.W = W;
    a.invert = invert != 0; a.both = out_kind == KIND_SIGNED; a.border = border_background != 0;
    a.r2 = ball_r2;
    const int chunk = unit ? MAXU : MAXG;
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int np = std::min(chunk, N - n0);
        a.n0 = n0;
        for (int i = 0; i < MAXG; ++i)
            for (int k = 0; k < 3; ++k) a.sp[i][k] = (spacing && !unit) ? spacing[3 * (n0 + std::min(i, np - 1)) + k] : 1.f;
        int rc;
        if (unit) rc = indices ? run_chunk<false, true>(a, np, out_kind, out, indices, (uint8_t*)ws, lay, st)
                               : run_chunk<false, false>(a, np, out_kind, out, indices, (uint8_t*)ws, lay, st);
        else rc = indices ? run_chunk<true, true>(a, np, out_kind, out, indices, (uint8_t*)ws, lay, st)
                          : run_chunk<true, false>(a, np, out_kind, out, indices, (uint8_t*)ws, lay, st);
        if (rc != CTU_OK) return rc;
    }
    return CTU_OK;
}
