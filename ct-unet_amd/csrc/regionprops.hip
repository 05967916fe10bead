// Region properties of label maps, gfx950: exact integer moments, bounding boxes and the float64 quantities derived from
// them (centroid, covariance, principal axes), per region of a label map (rule: ctunet_amd/postprocess.py, "Region
// properties"; tests/regionprops_ref.py restates it in numpy).
//
// Region r (1..R) of item n is the set of voxels whose label is r; 0 is background; any other value belongs to no region
// and is counted in overflow[n].  moments[n][r-1] = (count, Sz, Sy, Sx, Szz, Szy, Szx, Syy, Syx, Sxx) over the voxel
// indices, int64.  Every side is <= ctu_vox::MAX_SIDE = 1024 and an item has fewer than 2^31 voxels, so every sum is below
// 2^31 * 2^20 = 2^51 < 2^53 and converts to float64 exactly.
//
// ctu_region_moments, one pass over the map (it is read once, nothing else of its size is touched):
//   0. memsets: moments, overflow and the box accumulators (workspace) to 0.
//   1. moments: persistent blocks of 256 lanes over tiles of 256 lane-units; a lane-unit is 16 x-consecutive voxels of one
//      row, read with 16-byte loads (each16 of voxel_rows.h: one for uint8, four for int32, eight for int64).  Labels change
//      rarely along x: the usual lane holds one run of equal labels or two (a boundary), found without a branch as the
//      lengths of its first and last label, and their sums are closed forms of (start, length).  A lane with three runs
//      or more takes a voxel-by-voxel scan (a wave enters it only if one of its lanes needs it).  Every run but the lane's
//      last goes to the block's table at once; the last is first summed across the wave among the lanes that hold the
//      same label (32-bit shuffles: a lane's ten sums are below 2^24), so a wave
//      inside one region makes one table update instead of 64.  The table is a 128-slot LDS hash keyed by label: ten 64-bit
//      LDS integer adds and six 32-bit LDS maxima per update.  A label that finds no slot within 8 probes goes straight to
//      the global accumulators (slow, correct: every accumulator is a commutative integer operation).  The block flushes
//      its occupied slots with 64-bit global integer atomics when more than half the table is in use after a tile, and
//      once at its end: with few labels the number of flushes is the grid's size, whatever the volume's.
//      Box corners are kept as maxima over zero-initialised words: BIAS - lower corner and upper corner + 1.
//   2. boxes: one lane per region decodes the accumulators into (z0, y0, x0, z1, y1, x1), half open; six zeros when empty.
// Integer adds and maxima commute: the result is a function of the input alone and two calls are bit-equal.  No float
// atomic anywhere, no host synchronisation, nothing allocated: capture-safe.
//
// ctu_region_derive, one lane per region, float64, every operation rounded on its own (contraction is off for the file):
//   n = count, m_a = S_a / n, centroid_a = origin_a + sampling_a * m_a, c_ab = S_ab / n - m_a * m_b,
//   covariance_ab = (c_ab * sampling_min(a,b)) * sampling_max(a,b); then 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2) with +, -, *, /
//   and sqrt only, the eigenvalues sorted in descending order (stable), the sign rule and the cross product of the docstring.
//
// Replaces: nothing in the reference; users would copy the label map to the host for scipy.ndimage.
#include "common.h"
#include "voxel_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int LV = 16;                          // voxels of a lane-unit
constexpr int TB = 256;                         // lanes of a block = lane-units of a tile
constexpr int NM = 10;                          // moments
constexpr int SLOTS = 128;                      // LDS table (a power of two)
constexpr int SLOT_BITS = 7;
constexpr int PROBES = 8;                       // then the label spills to the global accumulators
constexpr int FLUSH_AT = SLOTS / 2;
constexpr int WAVE_MIN = 8;                     // lanes that share a label before the wave sums for them
constexpr int MAX_R = 65536;                    // CTU_REGION_MAX
constexpr int BIAS = ctu_vox::MAX_SIDE;         // lower corners are kept as BIAS - x: every box word is a maximum over 0
constexpr int GRID_CAP = 256 * 8;               // 8 resident blocks on each of 256 CUs (14 KB of LDS each)
constexpr int SWEEPS = 8;                       // CTU_REGION_SWEEPS
constexpr int MAXG = 64;                        // items per derive launch: their frames travel in the kernel arguments

typedef unsigned long long u64;

struct Table {
    u64 sum[SLOTS][NM];
    int box[SLOTS][6];
    int key[SLOTS];                             // 0: free
    int used;
    u64 ovf;
};

// the global accumulators of one item
struct Acc {
    u64* mom;                                   // [R][NM]
    int* box;                                   // [R][6]
};

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ void gadd(u64* p, u64 v) {
    if (v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gmax(int* p, int v) {
    if (v) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of a label (1..R) in the block's table, or -1 when PROBES slots from its hash are taken by other labels
__device__ __forceinline__ int slot_of(Table& t, int code) {
    int h = (int)(((uint32_t)code * 2654435761u) >> (32 - SLOT_BITS));
#pragma unroll 1
    for (int i = 0; i < PROBES; ++i) {
        int k = lds_load(t.key + h);
        if (k == 0) {
            k = atomicCAS(t.key + h, 0, code);
            if (k == 0) {
                atomicAdd(&t.used, 1);
                return h;
            }
        }
        if (k == code) return h;
        h = (h + 1) & (SLOTS - 1);
    }
    return -1;
}

// one update: ten sums and the six box words of `code`
__device__ __forceinline__ void add(Table& t, const Acc& g, int code, const uint32_t v[NM], const int b[6]) {
    const int s = slot_of(t, code);
    if (s >= 0) {
#pragma unroll
        for (int k = 0; k < NM; ++k)
            if (v[k]) atomicAdd(&t.sum[s][k], (u64)v[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicMax(&t.box[s][k], b[k]);
    } else {
        u64* m = g.mom + (int64_t)(code - 1) * NM;
        int* bx = g.box + (int64_t)(code - 1) * 6;
#pragma unroll
        for (int k = 0; k < NM; ++k) gadd(m + k, (u64)v[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) gmax(bx + k, b[k]);
    }
}

// a run of one row: cnt voxels at x0..x1 with sum sx and sum of squares sxx of their x.  Every entry is below 2^24
__device__ __forceinline__ void run_sums(int z, int y, int cnt, int sx, int sxx, int x0, int x1, uint32_t v[NM], int b[6]) {
    v[0] = cnt; v[1] = z * cnt; v[2] = y * cnt; v[3] = sx;
    v[4] = z * z * cnt; v[5] = z * y * cnt; v[6] = z * sx;
    v[7] = y * y * cnt; v[8] = y * sx; v[9] = sxx;
    b[0] = BIAS - z; b[1] = BIAS - y; b[2] = BIAS - x0;
    b[3] = z + 1; b[4] = y + 1; b[5] = x1 + 1;
}

// a run that ends inside a lane: rare, and kept out of line so that the unrolled scan of the 16 labels stays small
__device__ __noinline__ void add_inner_run(Table& t, Acc g, int code, int z, int y, int cnt, int sx, int sxx, int x0, int x1) {
    uint32_t v[NM];
    int b[6];
    run_sums(z, y, cnt, sx, sxx, x0, x1, v, b);
    add(t, g, code, v, b);
}

// 0 background, 1..R a region, -1 no region
template <class T>
__device__ __forceinline__ int code_of(T v, int R) {
    if constexpr (sizeof(T) == 1) {
        return v == 0 ? 0 : ((int)v <= R ? (int)v : -1);
    } else {
        return v == 0 ? 0 : ((v >= 1 && v <= (T)R) ? (int)v : -1);
    }
}

// the occupied slots go to the global accumulators and the table is cleared.  Called by the whole block behind a barrier
__device__ __forceinline__ void flush(Table& t, const Acc& g) {
    for (int i = threadIdx.x; i < SLOTS * 16; i += TB) {
        const int s = i >> 4, k = i & 15;
        const int code = t.key[s];
        if (!code) continue;
        if (k < NM) gadd(g.mom + (int64_t)(code - 1) * NM + k, t.sum[s][k]);
        else gmax(g.box + (int64_t)(code - 1) * 6 + (k - NM), t.box[s][k - NM]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS * 16; i += TB) {
        const int s = i >> 4, k = i & 15;
        if (k < NM) t.sum[s][k] = 0;
        else t.box[s][k - NM] = 0;
        if (k == 0) t.key[s] = 0;
    }
    if (threadIdx.x == 0) t.used = 0;
    __syncthreads();
}

template <class T>
__global__ void __launch_bounds__(TB) rp_moments_kernel(const T* __restrict__ labels, int64_t V, int D, int H, int W, int R,
                                                        int nxc, int ntiles, u64* __restrict__ mom,
                                                        int* __restrict__ boxacc, u64* __restrict__ overflow) {
    __shared__ Table t;
    const int n = blockIdx.y;
    const Acc g{mom + (int64_t)n * R * NM, boxacc + (int64_t)n * R * 6};
    for (int i = threadIdx.x; i < SLOTS * 16; i += TB) {
        const int s = i >> 4, k = i & 15;
        if (k < NM) t.sum[s][k] = 0;
        else t.box[s][k - NM] = 0;
        if (k == 0) t.key[s] = 0;
    }
    if (threadIdx.x == 0) {
        t.used = 0;
        t.ovf = 0;
    }
    __syncthreads();
    const T* src = labels + n * V;
    const int lane = threadIdx.x & 63;
    // this lane's unit (row z * H + y, chunk xc of the row) and the step from one of the block's tiles to the next: the
    // divisions are made once, then the position advances with carries
    int z, y, xc;
    {
        const int unit = blockIdx.x * TB + threadIdx.x;
        const int row = unit / nxc;
        xc = unit - row * nxc;
        z = row / H;
        y = row - z * H;
    }
    const int step = gridDim.x * TB, srow = step / nxc;
    const int dxc = step - srow * nxc, dz = srow / H, dy = srow - dz * H;
    uint32_t ovf = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int cur = 0, cnt = 0, sx = 0, sxx = 0, x0 = 0, x1 = 0;
        const bool live = z < D;                                 // the lane-units behind the last row
        const int x = xc * LV;
        int c[LV];
#pragma unroll
        for (int u = 0; u < LV; ++u) c[u] = 0;
        if (live)
            ctu_vox::each16(src + ((int64_t)z * H + y) * W + x, min(W - x, LV), [&](int u, T v) { c[u] = code_of<T>(v, R); });
        // the usual lane holds one run, or two (a boundary): lf voxels of its first label, lt of its last
        const int cf = c[0], cl = c[LV - 1];
        int lf = 1, lt = 1;
        bool af = true, at = true;
#pragma unroll
        for (int u = 1; u < LV; ++u) {
            af = af && c[u] == cf;
            at = at && c[LV - 1 - u] == cl;
            lf += af;
            lt += at;
        }
        const bool many = lf + lt < LV;                          // three runs or more
        if (!many) {
            const bool two = lf < LV;
            if (two && cf > 0) {
                const int l = lf;
                add_inner_run(t, g, cf, z, y, l, l * x + l * (l - 1) / 2,
                              l * x * x + x * l * (l - 1) + (l - 1) * l * (2 * l - 1) / 6, x, x + l - 1);
            }
            ovf += (cf < 0 ? lf : 0) + (two && cl < 0 ? lt : 0);
            const int l = two ? lt : lf, s = x + LV - l;          // the lane's last run: s .. s + l - 1
            cur = cl;
            cnt = l;
            sx = l * s + l * (l - 1) / 2;
            sxx = l * s * s + s * l * (l - 1) + (l - 1) * l * (2 * l - 1) / 6;
            x0 = s;
            x1 = s + l - 1;
        }
        if (__any(many)) {
            if (many) {
#pragma unroll
                for (int u = 0; u < LV; ++u) {
                    if (c[u] != cur) {
                        if (cur > 0) add_inner_run(t, g, cur, z, y, cnt, sx, sxx, x0, x1);
                        cur = c[u];
                        cnt = 0; sx = 0; sxx = 0;
                        x0 = x + u;
                    }
                    if (c[u] > 0) {
                        ++cnt;
                        sx += x + u;
                        sxx += (x + u) * (x + u);
                        x1 = x + u;
                    }
                    ovf += c[u] < 0;
                }
            }
        }
        // the run each lane ends with: summed across the wave for the labels that many lanes share
        uint32_t v[NM];
        int b[6];
        run_sums(z, y, cnt, sx, sxx, x0, x1, v, b);
        if (cur < 0) cur = 0;
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const u64 act = __ballot(cur > 0);
            if (!act) break;
            const int lead = __ffsll((long long)act) - 1;
            const int c0 = __shfl(cur, lead);
            const bool mine = cur == c0;
            if (__popcll(__ballot(mine)) < WAVE_MIN) break;
            uint32_t w[NM];
            int wb[6];
#pragma unroll
            for (int k = 0; k < NM; ++k) {
                w[k] = mine ? v[k] : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) w[k] += __shfl_xor(w[k], o);       // < 64 * 2^24
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                wb[k] = mine ? b[k] : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) wb[k] = max(wb[k], __shfl_xor(wb[k], o));
            }
            if (lane == lead) add(t, g, c0, w, wb);
            if (mine) cur = 0;
        }
        if (cur > 0) add(t, g, cur, v, b);
        // block-uniform whatever each lane saw of `used`: the table only fills faster or slower
        if (__syncthreads_or(lds_load(&t.used) > FLUSH_AT)) flush(t, g);
        xc += dxc;
        const int carry = xc >= nxc;
        xc -= carry ? nxc : 0;
        y += dy + carry;
        const int over = y >= H;
        y -= over ? H : 0;
        z += dz + over;
    }
    if (ovf) atomicAdd(&t.ovf, (u64)ovf);
    __syncthreads();
    flush(t, g);
    if (threadIdx.x == 0) gadd(overflow + n, t.ovf);
}

__global__ void __launch_bounds__(TB) rp_boxes_kernel(const long long* __restrict__ mom, const int* __restrict__ boxacc,
                                                      int64_t NR, int* __restrict__ boxes) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= NR) return;
    const bool some = mom[i * NM] != 0;
    const int* a = boxacc + i * 6;
    int* o = boxes + i * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[k] = some ? BIAS - a[k] : 0;
        o[3 + k] = some ? a[3 + k] : 0;
    }
}

// ------------------------------------------------------------------------------------------------ derived float64 fields
struct DeriveArgs {
    double frame[MAXG][6];                      // sampling z, y, x and origin z, y, x of each item of the launch
};

// one Jacobi rotation that annihilates a[p][q]; r is the third index
__device__ __forceinline__ void rotate(double a[3][3], double e[3][3], int p, int q, int r) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    a[p][p] = a[p][p] - t * apq;
    a[q][q] = a[q][q] + t * apq;
    a[p][q] = a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double ekp = e[k][p], ekq = e[k][q];
        e[k][p] = c * ekp - s * ekq;
        e[k][q] = s * ekp + c * ekq;
    }
}

__global__ void __launch_bounds__(TB) rp_derive_kernel(DeriveArgs fa, const long long* __restrict__ mom, int R, int n0,
                                                       double* __restrict__ centroid, double* __restrict__ covariance,
                                                       double* __restrict__ extent, double* __restrict__ axes) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r >= R) return;
    const int g = blockIdx.y;
    const int64_t i = (int64_t)(n0 + g) * R + r;
    const long long* m = mom + i * NM;
    const double nan = __builtin_nan("");
    double* oc = centroid + i * 3;
    double* ov = covariance + i * 9;
    double* oe = extent + i * 3;
    double* oa = axes + i * 9;
    const long long cnt = m[0];
    if (cnt == 0) {
        for (int k = 0; k < 3; ++k) oc[k] = oe[k] = nan;
        for (int k = 0; k < 9; ++k) ov[k] = oa[k] = nan;
        return;
    }
    const double n = (double)cnt;
    const double* sp = fa.frame[g];
    const double* org = fa.frame[g] + 3;
    double mean[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mean[a] = (double)m[1 + a] / n;
        oc[a] = org[a] + sp[a] * mean[a];
    }
    // Szz Szy Szx Syy Syx Sxx
    const double s2[3][3] = {{(double)m[4], (double)m[5], (double)m[6]},
                             {(double)m[5], (double)m[7], (double)m[8]},
                             {(double)m[6], (double)m[8], (double)m[9]}};
    double a[3][3], e[3][3];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int lo = p < q ? p : q, hi = p < q ? q : p;               // the product m_lo * m_hi: symmetric bit for bit
            const double c = s2[p][q] / n - mean[lo] * mean[hi];
            a[p][q] = (c * sp[lo]) * sp[hi];
            ov[p * 3 + q] = a[p][q];
            e[p][q] = p == q ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        rotate(a, e, 0, 1, 2);
        rotate(a, e, 0, 2, 1);
        rotate(a, e, 1, 2, 0);
    }
    // descending, stable: rank of k = number of entries that come before it
    const double w[3] = {a[0][0], a[1][1], a[2][2]};
    double ev[3], ax[3][3];                                                 // ax[j] = the j-th axis
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) rank += (w[j] > w[k]) || (w[j] == w[k] && j < k);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (rank == j) {
                ev[j] = w[k];
                ax[j][0] = e[0][k]; ax[j][1] = e[1][k]; ax[j][2] = e[2][k];
            }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int big = 0;
        double mag = ax[j][0] < 0.0 ? -ax[j][0] : ax[j][0];
#pragma unroll
        for (int k = 1; k < 3; ++k) {
            const double ak = ax[j][k] < 0.0 ? -ax[j][k] : ax[j][k];
            if (ak > mag) { mag = ak; big = k; }
        }
        const double lead = big == 0 ? ax[j][0] : (big == 1 ? ax[j][1] : ax[j][2]);
        if (lead < 0.0) {
            ax[j][0] = -ax[j][0]; ax[j][1] = -ax[j][1]; ax[j][2] = -ax[j][2];
        }
    }
    ax[2][0] = ax[0][1] * ax[1][2] - ax[0][2] * ax[1][1];
    ax[2][1] = ax[0][2] * ax[1][0] - ax[0][0] * ax[1][2];
    ax[2][2] = ax[0][0] * ax[1][1] - ax[0][1] * ax[1][0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        oe[j] = ev[j];
#pragma unroll
        for (int k = 0; k < 3; ++k) oa[k * 3 + j] = cnt < 2 ? nan : ax[j][k];   // the axes are the columns
    }
}

bool regions_ok(int N, int R) { return N > 0 && N <= 65535 && R >= 1 && R <= MAX_R; }

template <class T>
int run_moments(const void* labels, int N, int D, int H, int W, int R, u64* mom, int* boxacc, u64* overflow, hipStream_t st) {
    const int nxc = ceil_div(W, LV);
    const int units = D * H * nxc;                              // <= D*H*W < 2^31
    const int ntiles = ceil_div(units, TB);
    const Grid gr = persist_grid(ntiles, GRID_CAP / (N < GRID_CAP ? N : GRID_CAP));
    rp_moments_kernel<T><<<dim3((unsigned)gr.gx, (unsigned)N), TB, 0, st>>>((const T*)labels, (int64_t)D * H * W, D, H, W, R, nxc,
                                                                            ntiles, mom, boxacc, overflow);
    CTU_CHECK_LAUNCH("region_moments");
    return CTU_OK;
}

}  // namespace

extern "C" size_t ctu_region_moments_ws_bytes(int N, int R) {
    if (!regions_ok(N, R)) return 0;
    return align256((size_t)N * R * 6 * sizeof(int));
}

extern "C" int ctu_region_moments(const void* labels, int dtype, int N, int D, int H, int W, int R, int64_t* moments,
                                  int32_t* boxes, int64_t* overflow, void* ws, void* stream) {
    CTU_REQUIRE(labels && moments && boxes && overflow && ws, "region_moments: null pointer");
    CTU_REQUIRE(dtype == CTU_U8 || dtype == CTU_I32 || dtype == CTU_I64, "region_moments: unsupported dtype %d (uint8, int32 or int64)",
                dtype);
    CTU_REQUIRE(geometry_ok(N, D, H, W) && ctu_vox::sides_ok(D, H, W),
                "region_moments: bad shape N=%d D=%d H=%d W=%d (N in 1..65535, every side in 1..%d, D*H*W < 2^31)", N, D, H, W,
                ctu_vox::MAX_SIDE);
    // a lane-unit holds up to 16 voxels, so the last tile's lane-unit indices stay below D*H*W + 256
    CTU_REQUIRE((int64_t)D * H * ceil_div(W, LV) + TB < ((int64_t)1 << 31), "region_moments: too many rows");
    CTU_REQUIRE(R >= 1 && R <= MAX_R, "region_moments: num_regions must lie in 1..%d, got %d", MAX_R, R);
    hipStream_t st = (hipStream_t)stream;
    const size_t NR = (size_t)N * R;
    if (hipMemsetAsync(moments, 0, NR * NM * 8, st) != hipSuccess || hipMemsetAsync(overflow, 0, (size_t)N * 8, st) != hipSuccess ||
        hipMemsetAsync(ws, 0, NR * 6 * 4, st) != hipSuccess) {
        ctu_set_error("region_moments: memset failed");
        return CTU_ELAUNCH;
    }
    u64* mom = (u64*)moments;
    u64* ovf = (u64*)overflow;
    int* boxacc = (int*)ws;
    const int rc = dtype == CTU_U8    ? run_moments<uint8_t>(labels, N, D, H, W, R, mom, boxacc, ovf, st)
                   : dtype == CTU_I32 ? run_moments<int>(labels, N, D, H, W, R, mom, boxacc, ovf, st)
                                      : run_moments<long long>(labels, N, D, H, W, R, mom, boxacc, ovf, st);
    if (rc != CTU_OK) return rc;
    rp_boxes_kernel<<<(unsigned)ceil_div64((int64_t)NR, TB), TB, 0, st>>>((const long long*)moments, boxacc, (int64_t)NR, boxes);
    CTU_CHECK_LAUNCH("region_moments boxes");
    return CTU_OK;
}

extern "C" int ctu_region_derive(const int64_t* moments, int N, int R, const double* frame, double* centroid,
                                 double* covariance, double* extent, double* axes, void* stream) {
    CTU_REQUIRE(moments && centroid && covariance && extent && axes, "region_derive: null pointer");
    CTU_REQUIRE(regions_ok(N, R), "region_derive: N must lie in 1..65535 and num_regions in 1..%d, got %d and %d", MAX_R, N, R);
    if (frame)
        for (int i = 0; i < N; ++i) {
            CTU_REQUIRE(steps_ok(frame + 6 * (size_t)i), "region_derive: sampling must be positive and finite");
            CTU_REQUIRE(finite_n(frame + 6 * (size_t)i + 3, 3), "region_derive: origin must be finite");
        }
    hipStream_t st = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += MAXG) {
        const int np = N - n0 < MAXG ? N - n0 : MAXG;
        DeriveArgs fa;
        for (int i = 0; i < MAXG; ++i)
            for (int k = 0; k < 6; ++k) fa.frame[i][k] = (frame && i < np) ? frame[6 * (size_t)(n0 + i) + k] : (k < 3 ? 1.0 : 0.0);
        rp_derive_kernel<<<dim3((unsigned)ceil_div(R, TB), (unsigned)np), TB, 0, st>>>(fa, (const long long*)moments, R, n0, centroid,
                                                                                      covariance, extent, axes);
        CTU_CHECK_LAUNCH("region_derive");
    }
    return CTU_OK;
}
