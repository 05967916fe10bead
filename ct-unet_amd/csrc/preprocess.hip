// CT preprocessing on the device, gfx950: the step from a scanner's int16 volume to the binary skull the rest of the
// package works on.  Gaussian filter, histogram, Otsu's threshold and a range test (rules: ctunet_amd/preprocess.py;
// tests/preprocess_ref.py restates them).  No host synchronisation, nothing allocated, every launch on the given stream.
//
//   gaussian    two launches.  gauss_xy: a block owns 32 rows x 64 voxels of one plane; it stages the tile with its halo of
//               (ry, rx) voxels in LDS as float32 (the input dtype is converted when it is read; the border rule is applied
//               to the index of each staged voxel, so the passes themselves know no border), runs the x pass over every
//               staged row into a second LDS buffer and the y pass from there (a lane forms four rows at a time in
//               either pass: a weight serves four voxels, and in the y pass two LDS reads a tap do).  gauss_z: a block owns 32 planes x 128
//               voxels of the flattened (y, x) plane; it stages them with rz planes either side by 16-byte loads and every
//               thread forms four voxels at a time.  The intermediate lives in the caller's workspace with its plane
//               stride rounded up to 4 floats, so each of those loads is aligned whatever H * W is; the stores are 16 bytes
//               where the output address allows.  rz = 0 (w_0 = 1, the identity) skips gauss_z and the workspace.
//               Arithmetic: acc = w_0 v[i]; acc = acc + w_k (v[i-k] + v[i+k]), k = 1..R, every operation rounded on its
//               own (contraction is off for the file).  The weights arrive from the host in the kernel arguments.
//   histogram   block-private counts in LDS (integer LDS atomics, a lane merges equal neighbours of its 16 bytes first),
//               grid-stride 16-byte loads, one integer global atomic per non-empty bin per block.  Integer adds commute, so
//               two calls agree bit for bit.  range = NULL-able DEVICE double [2]: the kernel reads it, nothing comes back.
//   minmax      finite minimum and maximum: one row of (min, max) per block in the workspace, a second launch folds the rows.
//   otsu        one block; exact int64 prefixes by block_exclusive_scan, the variance in float64, the first maximum.
//   binarize    16 voxels per lane on the 16-byte grid of the OUTPUT (voxel_rows.h: mask16 reads, store_mask16 writes).
// Measured: profiles/preprocess.md.
//
// No reference counterpart: the reference's datasets load skulls that were thresholded before training
// (ctunet/pytorch/datasets.py:22-45).
#include <limits.h>

#include "common.h"
#include "scan.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int PB = 256;
constexpr int MAX_R = CTU_GAUSS_MAX_RADIUS;
constexpr int TX = 64, TY = 32;                 // gauss_xy: voxels and rows of a tile (TX = one wave)
constexpr int SR = 8;                           // gauss_xy: rows a wave stages at a time
constexpr int TZ = 32, TC = 128;                // gauss_z: planes and plane voxels of a tile (TC / 4 = 32 chunks, 8 plane groups)
constexpr int MAX_BATCH = 65535;                // grid.y
constexpr int MAX_BLOCKS = 2048;                // grid-stride kernels
constexpr int NEAREST = CTU_GAUSS_NEAREST, REFLECT = CTU_GAUSS_REFLECT, CONSTANT = CTU_GAUSS_CONSTANT;

struct GaussArgs {
    int D, H, W;
    int rz, ry, rx;
    int mode;
    float cval;
    int ntx, nty;
    int64_t oplane;                             // floats between two planes of gauss_xy's output
    float wz[MAX_R + 1], wy[MAX_R + 1], wx[MAX_R + 1];
};

// index of the voxel that position i of an axis of n voxels reads; -1: the constant
__device__ __forceinline__ int border(int i, int n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == NEAREST) return i < 0 ? 0 : n - 1;
    if (mode == REFLECT) {                      // d c b a | a b c d | d c b a, period 2 n
        const int p = 2 * n;
        int m = i % p;
        if (m < 0) m += p;
        return m < n ? m : p - 1 - m;
    }
    return -1;
}

template <class T>
__global__ void __launch_bounds__(PB) gauss_xy_kernel(GaussArgs a, const T* __restrict__ in, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int sw = TX + 2 * a.rx, sh = TY + 2 * a.ry;
    float* src = reinterpret_cast<float*>(smem);            // [sh][sw]: the tile and its halo
    float* mid = src + sh * sw;                             // [sh][TX]: after the x pass
    int bi = blockIdx.x;
    const int tx = bi % a.ntx;
    bi /= a.ntx;
    const int ty = bi % a.nty, z = bi / a.nty;
    const int X0 = tx * TX, Y0 = ty * TY;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    const T* plane = in + (int64_t)blockIdx.y * vox + (int64_t)z * a.H * a.W;
    // staging: sw <= 2 * 64, so a lane owns columns lane and lane + 64 of a row; the loads of SR rows are issued before the
    // first of them is used (a voxel that reads the constant loads voxel 0 of the plane instead and drops it: no branch
    // stands between two loads)
    const int c1 = lane + 64;
    const int x0 = border(X0 - a.rx + lane, a.W, a.mode), x1 = c1 < sw ? border(X0 - a.rx + c1, a.W, a.mode) : -1;
    for (int rb = wv; rb < sh; rb += SR * (PB / 64)) {
        T v[SR][2];
        int ys[SR];
#pragma unroll
        for (int i = 0; i < SR; ++i) {
            const int r = rb + i * (PB / 64);
            ys[i] = r < sh ? border(Y0 - a.ry + r, a.H, a.mode) : -1;
            v[i][0] = plane[(ys[i] < 0 || x0 < 0) ? 0 : ys[i] * a.W + x0];
            v[i][1] = plane[(ys[i] < 0 || x1 < 0) ? 0 : ys[i] * a.W + x1];
        }
#pragma unroll
        for (int i = 0; i < SR; ++i) {
            const int r = rb + i * (PB / 64);
            if (r >= sh) break;
            float* dst = src + r * sw;
            dst[lane] = (ys[i] < 0 || x0 < 0) ? a.cval : (float)v[i][0];
            if (c1 < sw) dst[c1] = (ys[i] < 0 || x1 < 0) ? a.cval : (float)v[i][1];
        }
    }
    __syncthreads();
    // x pass: a lane forms its voxel of 4 rows at a time, so a weight is fetched once for the four
    for (int r0 = 4 * wv; r0 < sh; r0 += 4 * (PB / 64)) {
        const float* p = src + r0 * sw + a.rx + lane;
        int off[4];
        float acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            off[j] = min(j, sh - 1 - r0) * sw;             // a row past the last is the last again, and is not stored
            acc[j] = a.wx[0] * p[off[j]];
        }
        for (int k = 1; k <= a.rx; ++k) {
            const float w = a.wx[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = p[off[j] - k] + p[off[j] + k];
                const float t = w * s;
                acc[j] = acc[j] + t;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // a row outside the volume reads as the constant in the y pass: it is not the x pass of a constant row
            if (r0 + j < sh) mid[(r0 + j) * TX + lane] = border(Y0 - a.ry + r0 + j, a.H, a.mode) >= 0 ? acc[j] : a.cval;
        }
    }
    __syncthreads();
    // y pass: a lane forms 4 consecutive rows of its column; l[j] = v[j - k] and h[j] = v[j + k] slide by one row per tap,
    // two LDS reads for the four voxels
    float* oplane = out + (int64_t)blockIdx.y * a.D * a.oplane + (int64_t)z * a.oplane;
    const int x = X0 + lane;
    for (int r0 = 4 * wv; r0 < TY; r0 += 4 * (PB / 64)) {
        if (Y0 + r0 >= a.H || x >= a.W) continue;
        const float* p = mid + (r0 + a.ry) * TX + lane;
        float l[4], h[4], acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            l[j] = h[j] = p[j * TX];
            acc[j] = a.wy[0] * l[j];
        }
        for (int k = 1; k <= a.ry; ++k) {
            const float w = a.wy[k];
            l[3] = l[2]; l[2] = l[1]; l[1] = l[0]; l[0] = p[-k * TX];
            h[0] = h[1]; h[1] = h[2]; h[2] = h[3]; h[3] = p[(3 + k) * TX];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = l[j] + h[j];
                const float t = w * s;
                acc[j] = acc[j] + t;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (Y0 + r0 + j < a.H) oplane[(Y0 + r0 + j) * a.W + x] = acc[j];
    }
}

// tmp: [N][D][a.oplane] floats, a.oplane = H * W rounded up to 4; the floats past H * W of a plane are never written and
// feed only lanes that store nothing
__global__ void __launch_bounds__(PB) gauss_z_kernel(GaussArgs a, const float* __restrict__ tmp, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    f32x4* box = reinterpret_cast<f32x4*>(smem);            // [TZ + 2 rz][TC / 4]
    const int HW = a.H * a.W;
    const int nct = (HW + TC - 1) / TC;
    const int C0 = (blockIdx.x % nct) * TC, Z0 = (blockIdx.x / nct) * TZ;
    const int ch = threadIdx.x & 31, zg = threadIdx.x >> 5;
    const int c = C0 + 4 * ch;
    const int sh = TZ + 2 * a.rz;
    const float* titem = tmp + (int64_t)blockIdx.y * a.D * a.oplane;
    for (int r = zg; r < sh; r += PB / 32) {
        const int z = border(Z0 - a.rz + r, a.D, a.mode);
        f32x4 v = {a.cval, a.cval, a.cval, a.cval};
        if (z >= 0 && c < HW) v = *reinterpret_cast<const f32x4*>(titem + (int64_t)z * a.oplane + c);
        box[r * (TC / 4) + ch] = v;
    }
    __syncthreads();
    if (c >= HW) return;
    float* oitem = out + (int64_t)blockIdx.y * a.D * HW;
    for (int r = zg; r < TZ; r += PB / 32) {
        const int z = Z0 + r;
        if (z >= a.D) break;
        const f32x4* p = box + (r + a.rz) * (TC / 4) + ch;
        f32x4 acc = a.wz[0] * p[0];
        for (int k = 1; k <= a.rz; ++k) {
            const f32x4 s = p[-k * (TC / 4)] + p[k * (TC / 4)];
            const f32x4 t = a.wz[k] * s;
            acc = acc + t;
        }
        float* o = oitem + (int64_t)z * HW + c;
        if (c + 4 <= HW && ((uintptr_t)o & 15) == 0) {
            *reinterpret_cast<f32x4*>(o) = acc;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c + u < HW) o[u] = acc[u];
        }
    }
}

size_t gauss_xy_lds(int ry, int rx) { return (size_t)(TY + 2 * ry) * (TX + 2 * rx + TX) * sizeof(float); }

template <class T>
int launch_gauss(GaussArgs a, const void* in, int64_t N, float* out, float* tmp, hipStream_t st) {
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    const int HW = a.H * a.W;
    const bool zpass = a.rz > 0;
    const int64_t tplane = ((int64_t)HW + 3) / 4 * 4;
    a.ntx = ceil_div(a.W, TX);
    a.nty = ceil_div(a.H, TY);
    a.oplane = zpass ? tplane : HW;
    const size_t lds_xy = gauss_xy_lds(a.ry, a.rx), lds_z = (size_t)(TZ + 2 * a.rz) * TC * sizeof(float);
    static size_t raised = 64 * 1024;
    const int rc = raise_lds(gauss_xy_kernel<T>, lds_xy, &raised, "gaussian_filter");
    if (rc != CTU_OK) return rc;
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const unsigned nb = (unsigned)(N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH);
        float* o = out + n0 * vox;
        gauss_xy_kernel<T><<<dim3((unsigned)(a.ntx * a.nty * a.D), nb), PB, lds_xy, st>>>(a, (const T*)in + n0 * vox,
                                                                                       zpass ? tmp : o);
        CTU_CHECK_LAUNCH("gaussian_filter (x, y)");
        if (zpass) {                            // the workspace holds one launch's items: the next launch reuses it
            gauss_z_kernel<<<dim3((unsigned)(ceil_div(HW, TC) * ceil_div(a.D, TZ)), nb), PB, lds_z, st>>>(a, tmp, o);
            CTU_CHECK_LAUNCH("gaussian_filter (z)");
        }
    }
    return CTU_OK;
}

// ------------------------------------------------------------------------------------------------ histogram and Otsu
struct Range {
    const double* dev;                          // DEVICE [2], or NULL: lo, hi below
    double lo, hi;
};

__device__ __forceinline__ void resolve(const Range& r, double& lo, double& hi) {
    lo = r.dev ? r.dev[0] : r.lo;
    hi = r.dev ? r.dev[1] : r.hi;
    if (hi == lo) {                             // numpy's rule for an empty range
        lo = lo - 0.5;
        hi = hi + 0.5;
    }
}

template <class T>
__device__ __forceinline__ int bin_of(T v, double lo, double hi, double scale, int bins) {
    const double d = (double)v;
    if (!(d >= lo && d <= hi)) return -1;       // outside, or NaN
    const double f = floor((d - lo) * scale);
    return f >= (double)bins ? bins - 1 : (int)f;
}

// the 16-byte grid of a flat array: `head` elements in front of the first aligned address, then `nvec` whole vectors
template <class T>
__device__ __forceinline__ void split16(const T* p, int64_t n, int64_t& head, int64_t& nvec) {
    constexpr int PER = 16 / (int)sizeof(T);
    head = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    nvec = (n - head) / PER;
}

template <class T>
__global__ void __launch_bounds__(PB) histogram_kernel(const T* __restrict__ in, int64_t n, int bins, Range rg,
                                                       unsigned long long* __restrict__ out) {
    constexpr int PER = 16 / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(PER)));
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem);
    for (int i = threadIdx.x; i < bins; i += PB) cnt[i] = 0;
    __syncthreads();
    double lo, hi;
    resolve(rg, lo, hi);
    const double scale = (double)bins / (hi - lo);
    int64_t head, nvec;
    split16(in, n, head, nvec);
    const Vec* vp = reinterpret_cast<const Vec*>(in + head);
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PB) {
        const Vec v = vp[i];
        int rb = -1;                            // a run of equal bins among the vector's voxels: one LDS atomic
        uint32_t rc = 0;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int b = bin_of(v[u], lo, hi, scale, bins);
            if (b == rb) {
                ++rc;
            } else {
                if (rb >= 0) atomicAdd(&cnt[rb], rc);
                rb = b;
                rc = 1;
            }
        }
        if (rb >= 0) atomicAdd(&cnt[rb], rc);
    }
    if (blockIdx.x == 0) {                      // the elements off the grid: fewer than 2 PER
        const int64_t tail0 = head + nvec * PER;
        for (int64_t i = threadIdx.x; i < head + (n - tail0); i += PB) {
            const int b = bin_of(in[i < head ? i : tail0 + (i - head)], lo, hi, scale, bins);
            if (b >= 0) atomicAdd(&cnt[b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += PB)
        if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

__device__ __forceinline__ bool finite_d(double d) { return d - d == 0.0; }

// (min, max) of the block's finite values in row blockIdx.x of `rows`
template <class T>
__global__ void __launch_bounds__(PB) minmax_kernel(const T* __restrict__ in, int64_t n, double* __restrict__ rows) {
    constexpr int PER = 16 / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(PER)));
    __shared__ double red[2][PB / 64];
    double mn = __builtin_inf(), mx = -__builtin_inf();
    int64_t head, nvec;
    split16(in, n, head, nvec);
    const Vec* vp = reinterpret_cast<const Vec*>(in + head);
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * PB) {
        const Vec v = vp[i];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const double d = (double)v[u];
            if (finite_d(d)) {
                mn = d < mn ? d : mn;
                mx = d > mx ? d : mx;
            }
        }
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + nvec * PER;
        for (int64_t i = threadIdx.x; i < head + (n - tail0); i += PB) {
            const double d = (double)in[i < head ? i : tail0 + (i - head)];
            if (finite_d(d)) {
                mn = d < mn ? d : mn;
                mx = d > mx ? d : mx;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mn;
        red[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PB / 64; ++w) {
            mn = red[0][w] < mn ? red[0][w] : mn;
            mx = red[1][w] > mx ? red[1][w] : mx;
        }
        rows[2 * blockIdx.x] = mn;
        rows[2 * blockIdx.x + 1] = mx;
    }
}

__global__ void __launch_bounds__(64) minmax_fold_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ range) {
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (int i = threadIdx.x; i < nrows; i += 64) {
        mn = rows[2 * i] < mn ? rows[2 * i] : mn;
        mx = rows[2 * i + 1] > mx ? rows[2 * i + 1] : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (threadIdx.x == 0) {
        range[0] = mn;
        range[1] = mx;
    }
}

int stream_blocks(int64_t n, int elem) {
    const int64_t nv = n / (16 / elem);
    const int64_t b = ceil_div64(nv, PB);
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

__global__ void __launch_bounds__(PB) otsu_kernel(const long long* __restrict__ h, int bins, Range rg,
                                                  double* __restrict__ threshold, long long* __restrict__ index) {
    __shared__ long long wsum[PB / 64];
    __shared__ double bestv[PB];
    __shared__ int bestk[PB];
    const int per = (bins + PB - 1) / PB;
    const int k0 = threadIdx.x * per, k1 = min(k0 + per, bins);
    long long w = 0, s = 0;
    for (int k = k0; k < k1; ++k) {
        w += h[k];
        s += (long long)k * h[k];
    }
    long long N, S;
    long long w1 = block_exclusive_scan<long long>(w, wsum, N);
    long long s1 = block_exclusive_scan<long long>(s, wsum, S);
    double best = -1.0;                         // every variance is >= 0: the first candidate always enters
    int bk = 0;
    for (int k = k0; k < k1 && k <= bins - 2; ++k) {
        w1 += h[k];
        s1 += (long long)k * h[k];
        double var = 0.0;
        if (w1 != 0 && w1 != N) {
            const long long w2 = N - w1;
            const double m1 = (double)s1 / (double)w1, m2 = (double)(S - s1) / (double)w2;
            const double d = m1 - m2;
            const double ww = (double)w1 * (double)w2, dd = d * d;
            var = ww * dd;
        }
        if (var > best) {
            best = var;
            bk = k;
        }
    }
    bestv[threadIdx.x] = best;
    bestk[threadIdx.x] = bk;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < PB; ++t)            // thread order is bin order: a strict > keeps the first maximum
            if (bestv[t] > best) {
                best = bestv[t];
                bk = bestk[t];
            }
        double lo, hi;
        resolve(rg, lo, hi);
        const double width = (hi - lo) / (double)bins;
        const double off = ((double)bk + 0.5) * width;
        *threshold = lo + off;
        if (index) *index = bk;
    }
}

// ------------------------------------------------------------------------------------------------ binarize
struct InRange {
    double lo, hi;
    template <class V> __device__ __forceinline__ bool operator()(V v) const {
        const double d = (double)v;
        return d > lo && d <= hi;
    }
};

struct Bound {
    const double* dev;                          // DEVICE [1], or NULL: v below
    double v;
};

template <class T>
__global__ void __launch_bounds__(PB) binarize_kernel(const T* __restrict__ in, int64_t n, Bound lower, Bound upper,
                                                      uint8_t* __restrict__ out) {
    InRange pred;
    pred.lo = lower.dev ? *lower.dev : lower.v;
    pred.hi = upper.dev ? *upper.dev : upper.v;
    // chunk 0: the bytes in front of the output's first 16-byte boundary; chunk j >= 1: 16 bytes on the grid
    int64_t first = (int64_t)((16 - ((uintptr_t)out & 15)) & 15);
    if (first > n) first = n;
    const int64_t nchunks = 1 + (n - first + 15) / 16;
    for (int64_t j = (int64_t)blockIdx.x * PB + threadIdx.x; j < nchunks; j += (int64_t)gridDim.x * PB) {
        const int64_t a = j == 0 ? 0 : first + 16 * (j - 1);
        const int64_t b = j == 0 ? first : (a + 16 < n ? a + 16 : n);
        const int nv = (int)(b - a);
        if (nv <= 0) continue;
        ctu_vox::store_mask16(out + a, nv, ctu_vox::mask16(in + a, nv, pred));
    }
}

bool dtype_ok(int dtype) { return dtype == CTU_F32 || dtype == CTU_I16 || dtype == CTU_U8; }
int elem_size(int dtype) { return dtype == CTU_F32 ? 4 : (dtype == CTU_I16 ? 2 : 1); }
constexpr int64_t MAX_ELEMS = (int64_t)1 << 38;  // a block's LDS counts are 32-bit: 2^38 / 2048 blocks stays far below

}  // namespace

#define PP_DISPATCH(dtype, ...)                                   \
    do {                                                          \
        if ((dtype) == CTU_F32) { typedef float T; __VA_ARGS__; } \
        else if ((dtype) == CTU_I16) { typedef int16_t T; __VA_ARGS__; } \
        else { typedef uint8_t T; __VA_ARGS__; }                  \
    } while (0)

extern "C" size_t ctu_gaussian_ws_bytes(int64_t N, int D, int H, int W, int rz) {
    if (N < 1 || !ctu_vox::sides_ok(D, H, W) || rz < 1) return 0;
    const int64_t tplane = ((int64_t)H * W + 3) / 4 * 4;
    return align256((size_t)(N < MAX_BATCH ? N : MAX_BATCH) * D * tplane * sizeof(float));
}

extern "C" int ctu_gaussian_filter(const void* in, int dtype, int64_t N, int D, int H, int W, const int* radius,
                                   const float* weights, int mode, float cval, float* out, void* ws, void* stream) {
    CTU_REQUIRE(in && out && radius && weights, "gaussian_filter: null pointer");
    CTU_REQUIRE(dtype_ok(dtype), "gaussian_filter: unsupported dtype %d (float32, int16 or uint8)", dtype);
    CTU_REQUIRE(mode >= NEAREST && mode <= CONSTANT, "gaussian_filter: unknown mode %d", mode);
    CTU_REQUIRE(N > 0 && ctu_vox::sides_ok(D, H, W) && (int64_t)D * H * W < ((int64_t)1 << 31),
                "gaussian_filter: bad shape N=%lld %dx%dx%d (every side in 1..%d, D*H*W < 2^31)", (long long)N, D, H, W,
                ctu_vox::MAX_SIDE);
    for (int a = 0; a < 3; ++a)
        CTU_REQUIRE(radius[a] >= 0 && radius[a] <= MAX_R, "gaussian_filter: radius %d of axis %d outside 0..%d", radius[a], a,
                    MAX_R);
    CTU_REQUIRE(radius[0] == 0 || ws, "gaussian_filter: the z pass needs the workspace of ctu_gaussian_ws_bytes");
    CTU_REQUIRE(((uintptr_t)ws & 15) == 0, "gaussian_filter: the workspace must be 16-byte aligned");
    GaussArgs a;
    a.D = D; a.H = H; a.W = W;
    a.rz = radius[0]; a.ry = radius[1]; a.rx = radius[2];
    a.mode = mode;
    a.cval = cval;
    const float* w = weights;
    for (int k = 0; k <= MAX_R; ++k) a.wz[k] = k <= a.rz ? w[k] : 0.f;
    w += a.rz + 1;
    for (int k = 0; k <= MAX_R; ++k) a.wy[k] = k <= a.ry ? w[k] : 0.f;
    w += a.ry + 1;
    for (int k = 0; k <= MAX_R; ++k) a.wx[k] = k <= a.rx ? w[k] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    PP_DISPATCH(dtype, return launch_gauss<T>(a, in, N, out, (float*)ws, st));
    return CTU_OK;
}

extern "C" size_t ctu_minmax_ws_bytes(int64_t n) { return n < 1 ? 0 : align256((size_t)MAX_BLOCKS * 2 * sizeof(double)); }

extern "C" int ctu_finite_minmax(const void* in, int dtype, int64_t n, double* range, void* ws, void* stream) {
    CTU_REQUIRE(in && range && ws, "finite_minmax: null pointer");
    CTU_REQUIRE(dtype_ok(dtype), "finite_minmax: unsupported dtype %d (float32, int16 or uint8)", dtype);
    CTU_REQUIRE(n > 0 && n < MAX_ELEMS, "finite_minmax: %lld elements (1 .. 2^38 - 1)", (long long)n);
    hipStream_t st = (hipStream_t)stream;
    const int nb = stream_blocks(n, elem_size(dtype));
    PP_DISPATCH(dtype, minmax_kernel<T><<<nb, PB, 0, st>>>((const T*)in, n, (double*)ws));
    CTU_CHECK_LAUNCH("finite_minmax");
    minmax_fold_kernel<<<1, 64, 0, st>>>((const double*)ws, nb, range);
    CTU_CHECK_LAUNCH("finite_minmax (fold)");
    return CTU_OK;
}

extern "C" int ctu_histogram(const void* in, int dtype, int64_t n, int bins, const double* range, double lo, double hi,
                             int64_t* hist, void* stream) {
    CTU_REQUIRE(in && hist, "histogram: null pointer");
    CTU_REQUIRE(dtype_ok(dtype), "histogram: unsupported dtype %d (float32, int16 or uint8)", dtype);
    CTU_REQUIRE(n > 0 && n < MAX_ELEMS, "histogram: %lld elements (1 .. 2^38 - 1)", (long long)n);
    CTU_REQUIRE(bins >= 2 && bins <= CTU_HISTOGRAM_MAX_BINS, "histogram: bins must lie in 2..%d, got %d", CTU_HISTOGRAM_MAX_BINS,
                bins);
    CTU_REQUIRE(range || (lo <= hi && hi - hi == 0.0 && lo - lo == 0.0), "histogram: range (%g, %g) must be finite, lo <= hi",
                lo, hi);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)bins * sizeof(int64_t), st) != hipSuccess) {
        ctu_set_error("histogram: cannot clear the counts");
        return CTU_ELAUNCH;
    }
    const Range rg = {range, lo, hi};
    const int nb = stream_blocks(n, elem_size(dtype));
    PP_DISPATCH(dtype, histogram_kernel<T><<<nb, PB, (size_t)bins * sizeof(uint32_t), st>>>((const T*)in, n, bins, rg,
                                                                                         (unsigned long long*)hist));
    CTU_CHECK_LAUNCH("histogram");
    return CTU_OK;
}

extern "C" int ctu_threshold_otsu(const int64_t* hist, int bins, const double* range, double lo, double hi,
                                  double* threshold, int64_t* index, void* stream) {
    CTU_REQUIRE(hist && threshold, "threshold_otsu: null pointer");
    CTU_REQUIRE(bins >= 2 && bins <= CTU_HISTOGRAM_MAX_BINS, "threshold_otsu: bins must lie in 2..%d, got %d",
                CTU_HISTOGRAM_MAX_BINS, bins);
    CTU_REQUIRE(range || (lo <= hi && hi - hi == 0.0 && lo - lo == 0.0), "threshold_otsu: range (%g, %g) must be finite, lo <= hi",
                lo, hi);
    const Range rg = {range, lo, hi};
    otsu_kernel<<<1, PB, 0, (hipStream_t)stream>>>((const long long*)hist, bins, rg, threshold, (long long*)index);
    CTU_CHECK_LAUNCH("threshold_otsu");
    return CTU_OK;
}

extern "C" int ctu_binarize(const void* in, int dtype, int64_t n, const double* lower_dev, double lower,
                            const double* upper_dev, double upper, uint8_t* out, void* stream) {
    CTU_REQUIRE(in && out, "binarize: null pointer");
    CTU_REQUIRE(dtype_ok(dtype), "binarize: unsupported dtype %d (float32, int16 or uint8)", dtype);
    CTU_REQUIRE(n > 0, "binarize: %lld elements", (long long)n);
    const Bound lb = {lower_dev, lower}, ub = {upper_dev, upper};
    const int64_t b = ceil_div64(n / 16 + 2, PB);
    const int nb = (int)(b > MAX_BLOCKS ? MAX_BLOCKS : b);
    PP_DISPATCH(dtype, binarize_kernel<T><<<nb, PB, 0, (hipStream_t)stream>>>((const T*)in, n, lb, ub, out));
    CTU_CHECK_LAUNCH("binarize");
    return CTU_OK;
}
