// Surface-distance metrics of segmentations, gfx950: HD, HD_p (percentile Hausdorff), ASSD, surface Dice (NSD) and hard
// Dice with voxel spacing, from label maps or one-hot tensors (definitions: ctunet_amd/metrics.py).
//
// One (item, class) pair = two planes (side 0 = prediction P, side 1 = target G).  Per group of pairs:
//   1. edge_x:  one wave per image row reads both sides' memberships (16 x-consecutive voxels per lane, vector loads),
//               forms the surface mask & ~erode(mask) (6-neighbourhood, background outside), writes one edge byte per
//               voxel and the 1-D squared distance to the nearest edge voxel of the row (ballot-free: per-lane 16-bit
//               masks + two wave scans), and counts surface voxels, |P|, |G|, |P & G| (integer atomics).
//   2. line y, line z: exact squared EDT along the other two axes, one lane per line, lanes at consecutive x (coalesced):
//               linear-time lower envelope of parabolas (Felzenszwalb-Huttenlocher), the stack in LDS, in place.
//               Unit spacing: int32 squared distances (exact); otherwise fp32 physical squared distances sum (k_i s_i)^2.
//   3. reduce:  per directed plane (surface of one side, distance map of the other): max key, fp64 sum of distances and
//               count within tolerance, one slab entry per block (fixed grid: deterministic, no float atomics).
//   4. select (with a percentile): 4 radix passes of 8 bits over the uint32 keys of the surface voxels give the two
//               bracketing order statistics exactly (integer histograms).
//   5. final:   sqrt, interpolation, the empty-surface rules, the symmetric / directed combinations.
// No host synchronisation, allocation or copy: the whole sequence can be captured into a graph.
//
// ctu_hausdorff, the metric of the inference tail, is a composition on top: argmax of the prediction into a
// float label map (ctu_hard_segm), these metrics against the one-hot target, and the HD row copied out.
//
// Replaces: hausdorff (monai compute_hausdorff_distance on one_hot(argmax(pred)))  ctunet/utilities.py:62-70, the
//           reference's only distance metric; for the others evaluation users would call monai / scipy on the CPU.
#include "common.h"
#include "edt_line.h"

namespace {

using namespace ctu_edt;             // INF_I, LINE_LDS, DistT, is_inf, dist_inf, line_lanes, row_nearest, store16, edt_line
using namespace ctu_vox;             // InClass, mask16, store_mask16, sides_ok, MAX_SIDE

constexpr int EB = 256;                 // edge_x block: 4 waves, one row per wave
constexpr int RT = 256;                 // reduce / histogram block
constexpr int RB_MAX = 256;             // reduce blocks per directed plane
constexpr int MAXG = 64;                // pairs per group (kernel-argument spacing table)
constexpr int MAXC = 16;

struct Side {
    const void* p;
    int dtype;                          // CTU_U8, CTU_I64 or CTU_F32
    int onehot;                         // 1: mask = p[n][c] != 0; 0: label map, mask = p[n] == c
};

struct GroupArgs {
    Side a, b;                          // prediction, target
    int Ct, cls0, Cs, D, H, W;          // one-hot channel count, first scored class, scored classes, volume
    int pair0, np;                      // first global pair of the group and its size
    int has_tau, pairs;                 // pairs = N * Cs (row stride of out)
    double pct;                         // percentile in [0, 100], < 0: none
    double tau[MAXC];
    float sp[MAXG][3];                  // (z, y, x) spacing of each pair of the group
};

struct SlabEntry {
    uint32_t mx;                        // max key (uint32 bits of a non-negative int or float)
    uint32_t cnt;                       // distances <= tau
    double sum;                         // sum of distances
};

struct SelState {
    uint32_t prefix[2];
    uint32_t k[2];
};

// 16-bit membership mask of class c in nv (<= 16) x-consecutive voxels starting at element `off` of side s
__device__ __forceinline__ uint32_t row_bits(const Side& s, int64_t off, int nv, int c) {
    const InClass in{s.onehot, c};
    if (s.dtype == CTU_U8) return mask16((const uint8_t*)s.p + off, nv, in);
    if (s.dtype == CTU_F32) return mask16((const float*)s.p + off, nv, in);
    return mask16((const long long*)s.p + off, nv, in);
}

// ------------------------------------------------------------------------------------------------ 1. edges + x pass
template <bool FLT>
__global__ void __launch_bounds__(EB) surf_edge_x_kernel(GroupArgs g, int64_t Vp, uint8_t* __restrict__ edges,
                                                         void* __restrict__ dist, unsigned long long* __restrict__ counts) {
    typedef typename DistT<FLT>::T T;
    const int lane = threadIdx.x & 63;
    const int il = blockIdx.y;
    const int pair = g.pair0 + il;
    const int n = pair / g.Cs, c = pair % g.Cs + g.cls0;
    const int D = g.D, H = g.H, W = g.W;
    const int64_t HW = (int64_t)H * W, V = (int64_t)D * HW;
    const int64_t base[2] = {g.a.onehot ? ((int64_t)n * g.Ct + c) * V : (int64_t)n * V,
                             g.b.onehot ? ((int64_t)n * g.Ct + c) * V : (int64_t)n * V};
    const float sx2 = g.sp[il][2] * g.sp[il][2];
    const int x0 = lane * 16;
    const int nv = min(max(W - x0, 0), 16);
    uint32_t cnt[5] = {0, 0, 0, 0, 0};       // |dP|, |dG|, |P & G|, |P|, |G|
    const int nrows = D * H;
    const int nwaves = gridDim.x * (EB / 64);
    for (int r = blockIdx.x * (EB / 64) + (threadIdx.x >> 6); r < nrows; r += nwaves) {    // wave-uniform
        const int z = r / H, y = r - (r / H) * H;
        const int64_t vrow = (int64_t)z * HW + (int64_t)y * W + x0;
        uint32_t m[2], e[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const Side& sd = s ? g.b : g.a;
            const int64_t o = base[s] + vrow;
            uint32_t mm = 0, inner = 0;
            if (nv) {
                mm = row_bits(sd, o, nv, c);
                inner = mm;
                if (inner) inner &= (y > 0) ? row_bits(sd, o - W, nv, c) : 0u;
                if (inner) inner &= (y < H - 1) ? row_bits(sd, o + W, nv, c) : 0u;
                if (inner) inner &= (z > 0) ? row_bits(sd, o - HW, nv, c) : 0u;
                if (inner) inner &= (z < D - 1) ? row_bits(sd, o + HW, nv, c) : 0u;
            }
            // x neighbours: bit 15 of the lane on the left, bit 0 of the lane on the right (0 outside the row)
            const uint32_t up = __shfl_up(mm, 1), dn = __shfl_down(mm, 1);
            const uint32_t lin = lane > 0 ? (up >> 15) & 1u : 0u, rin = lane < 63 ? dn & 1u : 0u;
            inner &= ((mm << 1) | lin) & ((mm >> 1) | (rin << 15));
            m[s] = mm;
            e[s] = mm & ~inner & 0xffffu;
        }
        cnt[0] += __popc(e[0]); cnt[1] += __popc(e[1]);
        cnt[2] += __popc(m[0] & m[1]); cnt[3] += __popc(m[0]); cnt[4] += __popc(m[1]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t es = e[s];
            T val[16];
            row_nearest<FLT, false>(es, x0, lane, sx2, val, nullptr);
            if (!nv) continue;
            const int64_t vo = (int64_t)(2 * il + s) * Vp + vrow;
            store16((T*)dist + vo, nv, val);
            store_mask16(edges + vo, nv, es);
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t v = cnt[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0 && v) atomicAdd(&counts[(size_t)pair * 5 + k], (unsigned long long)v);   // integer: order-free
    }
}

// ------------------------------------------------------------------------------------------------ 2. y / z passes
// One lane per line of length L (element stride lstride), lanes at consecutive x; blockIdx.x = o * nbx + x block, the
// line of lane x starts at o * ostride + x.  f(q) = min_k src(k) + s2 (q - k)^2 over the finite src(k), in place.
// Stack of the lower envelope: positions (uint16) and values in LDS, [entry][lane] (the routine: edt_line.h).
template <bool FLT>
__global__ void surf_line_kernel(GroupArgs g, int64_t Vp, void* __restrict__ dist, int L, int64_t lstride,
                                 int64_t ostride, int nbx, int axis) {
    typedef typename DistT<FLT>::T T;
    extern __shared__ uint8_t smem[];
    const int NL = blockDim.x, lane = threadIdx.x;
    T* Fs = reinterpret_cast<T*>(smem);
    uint16_t* Vs = reinterpret_cast<uint16_t*>(Fs + (size_t)L * NL);
    const int plane = blockIdx.y;
    const int xb = blockIdx.x % nbx, o = blockIdx.x / nbx;
    const int x = xb * NL + lane;
    if (x >= g.W) return;                 // no barriers below: every lane owns its line and its LDS column
    const float sp = g.sp[plane >> 1][axis];
    const T s2 = FLT ? (T)(sp * sp) : (T)1;
    T* d = (T*)dist + (int64_t)plane * Vp + (int64_t)o * ostride + x;

    edt_line<FLT, false>(d, L, lstride, s2, Fs, Vs, NL, lane, nullptr);
}

// ------------------------------------------------------------------------------------------------ 3. reduction
__device__ __forceinline__ double key_dist(uint32_t key, bool flt) {
    return flt ? sqrt((double)__uint_as_float(key)) : sqrt((double)(int)key);
}

// directed plane dp = 2 il + s: the surface of side s, the distance map of side s ^ 1
template <bool FLT>
__global__ void __launch_bounds__(RT) surf_reduce_kernel(GroupArgs g, int64_t V, int64_t Vp, const uint8_t* __restrict__ edges,
                                                         const uint32_t* __restrict__ dist, SlabEntry* __restrict__ slab, int RB) {
    __shared__ uint32_t smx[RT / 64], scnt[RT / 64];
    __shared__ double ssum[RT / 64];
    const int dp = blockIdx.y;
    const int pair = g.pair0 + (dp >> 1);
    const double tau = g.has_tau ? g.tau[pair % g.Cs] : -1.0;
    const uint4* e4 = reinterpret_cast<const uint4*>(edges + (int64_t)dp * Vp);
    const uint32_t* dk = dist + (int64_t)(dp ^ 1) * Vp;
    uint32_t mx = 0, cnt = 0;
    double sum = 0.0;
    const int64_t nvec = Vp / 16;
    for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < nvec; i += (int64_t)RB * RT) {
        const uint4 e = e4[i];
        if (!(e.x | e.y | e.z | e.w)) continue;
        const uint32_t w[4] = {e.x, e.y, e.z, e.w};
        for (int b = 0; b < 16; ++b) {
            const int64_t v = i * 16 + b;
            if (((w[b >> 2] >> (8 * (b & 3))) & 255u) == 0 || v >= V) continue;
            const uint32_t key = dk[v];
            mx = max(mx, key);
            const double dd = key_dist(key, FLT);
            sum += dd;
            cnt += (dd <= tau) ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        cnt += (uint32_t)__shfl_xor((int)cnt, o);
        sum += __shfl_xor(sum, o);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smx[wv] = mx; scnt[wv] = cnt; ssum[wv] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        SlabEntry r = {smx[0], scnt[0], ssum[0]};
        for (int k = 1; k < RT / 64; ++k) { r.mx = max(r.mx, smx[k]); r.cnt += scnt[k]; r.sum += ssum[k]; }
        slab[((int64_t)g.pair0 * 2 + dp) * RB + blockIdx.x] = r;
    }
}

// ------------------------------------------------------------------------------------------------ 4. order statistics
// numpy's default ("linear") percentile: virtual index h = n q + (1 - q) - 1, q = p / 100, lo = floor(h)
__device__ __forceinline__ void pct_index(uint64_t n, double pct, uint32_t* lo, uint32_t* hi, double* gamma) {
    const double q = pct / 100.0;
    const double h = (double)n * q + (1.0 - q) - 1.0;
    double fl = floor(h);
    if (fl < 0.0) fl = 0.0;
    if (fl > (double)(n - 1)) fl = (double)(n - 1);
    *lo = (uint32_t)fl;
    *hi = (uint32_t)min((uint64_t)fl + 1, n - 1);
    *gamma = h - fl;
}

__global__ void surf_select_init_kernel(GroupArgs g, const unsigned long long* __restrict__ counts, SelState* __restrict__ sel) {
    const int dp = blockIdx.x * blockDim.x + threadIdx.x;
    if (dp >= 2 * g.np) return;
    const int pair = g.pair0 + (dp >> 1);
    const uint64_t n = counts[(size_t)pair * 5 + (dp & 1)];
    SelState s = {{0u, 0u}, {0u, 0u}};
    if (n > 0) {
        double gm;
        pct_index(n, g.pct, &s.k[0], &s.k[1], &gm);
    }
    sel[(size_t)g.pair0 * 2 + dp] = s;
}

__global__ void __launch_bounds__(RT) surf_hist_kernel(GroupArgs g, int64_t V, int64_t Vp, const uint8_t* __restrict__ edges,
                                                       const uint32_t* __restrict__ dist, const SelState* __restrict__ sel,
                                                       uint32_t* __restrict__ hist, int RB, int shift) {
    __shared__ uint32_t h[2][256];
    const int dp = blockIdx.y;
    const int64_t gdp = (int64_t)g.pair0 * 2 + dp;
    const uint32_t mask_hi = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    const SelState s = sel[gdp];
    for (int i = threadIdx.x; i < 512; i += RT) (&h[0][0])[i] = 0;
    __syncthreads();
    const uint4* e4 = reinterpret_cast<const uint4*>(edges + (int64_t)dp * Vp);
    const uint32_t* dk = dist + (int64_t)(dp ^ 1) * Vp;
    const int64_t nvec = Vp / 16;
    for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < nvec; i += (int64_t)RB * RT) {
        const uint4 e = e4[i];
        if (!(e.x | e.y | e.z | e.w)) continue;
        const uint32_t w[4] = {e.x, e.y, e.z, e.w};
        for (int b = 0; b < 16; ++b) {
            const int64_t v = i * 16 + b;
            if (((w[b >> 2] >> (8 * (b & 3))) & 255u) == 0 || v >= V) continue;
            const uint32_t key = dk[v];
            const uint32_t dg = (key >> shift) & 255u;
            if ((key & mask_hi) == s.prefix[0]) atomicAdd(&h[0][dg], 1u);
            if ((key & mask_hi) == s.prefix[1]) atomicAdd(&h[1][dg], 1u);
        }
    }
    __syncthreads();
    uint32_t* gh = hist + gdp * 512;
    for (int i = threadIdx.x; i < 512; i += RT) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&gh[i], c);          // integer: order-free
    }
}

__global__ void surf_select_kernel(GroupArgs g, SelState* __restrict__ sel, uint32_t* __restrict__ hist, int shift) {
    const int dp = blockIdx.x * blockDim.x + threadIdx.x;
    if (dp >= 2 * g.np) return;
    const int64_t gdp = (int64_t)g.pair0 * 2 + dp;
    SelState s = sel[gdp];
    uint32_t* gh = hist + gdp * 512;
    for (int t = 0; t < 2; ++t) {
        uint32_t cum = 0, digit = 255;
        for (int b = 0; b < 256; ++b) {
            const uint32_t c = gh[t * 256 + b];
            if (cum + c > s.k[t]) { digit = b; break; }
            cum += c;
        }
        s.prefix[t] |= digit << shift;
        s.k[t] -= cum;
        for (int b = 0; b < 256; ++b) gh[t * 256 + b] = 0;   // ready for the next pass / call
    }
    sel[gdp] = s;
}

// ------------------------------------------------------------------------------------------------ 5. final
// out rows (each [pairs]): 0 dice, 1 hd, 2 hd directed, 3 hd_p, 4 hd_p directed, 5 assd, 6 asd directed, 7 nsd
template <bool FLT>
__global__ void surf_final_kernel(GroupArgs g, const unsigned long long* __restrict__ counts, const SlabEntry* __restrict__ slab,
                                  const SelState* __restrict__ sel, int RB, float* __restrict__ out) {
    const int il = blockIdx.x * blockDim.x + threadIdx.x;
    if (il >= g.np) return;
    const int pair = g.pair0 + il;
    const unsigned long long* cn = counts + (size_t)pair * 5;
    const uint64_t nP = cn[0], nG = cn[1], inter = cn[2], tot = cn[3] + cn[4];
    const float nan = __builtin_nanf("");
    const int P = g.pairs;
    out[0 * P + pair] = tot ? (float)(2.0 * (double)inter / (double)tot) : 1.f;
    uint32_t mx[2];
    uint64_t cnt[2];
    double sum[2], qd[2];
    for (int s = 0; s < 2; ++s) {
        const SlabEntry* se = slab + ((int64_t)pair * 2 + s) * RB;
        uint32_t m = 0;
        uint64_t c = 0;
        double sm = 0.0;
        for (int b = 0; b < RB; ++b) { m = max(m, se[b].mx); c += se[b].cnt; sm += se[b].sum; }
        mx[s] = m; cnt[s] = c; sum[s] = sm;
        qd[s] = 0.0;
        const uint64_t ns = s ? nG : nP;
        if (g.pct >= 0.0 && ns > 0) {
            uint32_t lo, hi;
            double gm;
            pct_index(ns, g.pct, &lo, &hi, &gm);
            const SelState st = sel[(int64_t)pair * 2 + s];
            const double a = key_dist(st.prefix[0], FLT), b = key_dist(st.prefix[1], FLT);
            const double diff = b - a;
            qd[s] = gm >= 0.5 ? b - diff * (1.0 - gm) : a + diff * gm;      // numpy's _lerp
        }
    }
    const bool both = nP > 0 && nG > 0;
    const double d0 = key_dist(mx[0], FLT), d1 = key_dist(mx[1], FLT);
    out[1 * P + pair] = both ? (float)fmax(d0, d1) : nan;
    out[2 * P + pair] = both ? (float)d0 : nan;
    out[3 * P + pair] = (both && g.pct >= 0.0) ? (float)fmax(qd[0], qd[1]) : nan;
    out[4 * P + pair] = (both && g.pct >= 0.0) ? (float)qd[0] : nan;
    out[5 * P + pair] = both ? (float)((sum[0] + sum[1]) / (double)(nP + nG)) : nan;
    out[6 * P + pair] = both ? (float)(sum[0] / (double)nP) : nan;
    float nsd = nan;
    if (g.has_tau && nP + nG > 0) nsd = both ? (float)((double)(cnt[0] + cnt[1]) / (double)(nP + nG)) : 0.f;
    out[7 * P + pair] = nsd;
}

// ------------------------------------------------------------------------------------------------ host side
int64_t pad16(int64_t v) { return (v + 15) & ~(int64_t)15; }

int group_pairs(int pairs, int64_t Vp) {
    const int64_t per_pair = 2 * Vp * 5;                              // two planes: edge byte + 4-byte distance
    const int64_t cap = std::max<int64_t>(1, ((int64_t)4 << 30) / per_pair);
    return (int)std::min<int64_t>(std::min<int64_t>(pairs, MAXG), cap);
}

int reduce_blocks(int64_t Vp) { return (int)std::min<int64_t>(ceil_div64(Vp / 16, RT), RB_MAX); }

struct Layout {
    size_t maps, counts, slab, sel, hist, total;
    int gp, RB;
    int64_t Vp;
};

Layout layout(int N, int Cs, int D, int H, int W) {
    Layout l;
    const int pairs = N * Cs;
    l.Vp = pad16((int64_t)D * H * W);
    l.gp = group_pairs(pairs, l.Vp);
    l.RB = reduce_blocks(l.Vp);
    size_t off = 0;
    l.maps = off;   off = align256(off + (size_t)2 * l.gp * l.Vp * 5);
    l.counts = off; off = align256(off + (size_t)pairs * 5 * sizeof(unsigned long long));
    l.hist = off;   off = align256(off + (size_t)pairs * 2 * 512 * sizeof(uint32_t));
    l.sel = off;    off = align256(off + (size_t)pairs * 2 * sizeof(SelState));
    l.slab = off;   off = align256(off + (size_t)pairs * 2 * l.RB * sizeof(SlabEntry));
    l.total = off;
    return l;
}

template <bool FLT>
int run_group(const GroupArgs& g, const Layout& lay, uint8_t* ws, float* out, hipStream_t st) {
    const int D = g.D, H = g.H, W = g.W;
    const int64_t V = (int64_t)D * H * W, Vp = lay.Vp;
    uint8_t* edges = ws + lay.maps;
    uint32_t* dist = reinterpret_cast<uint32_t*>(edges + (size_t)2 * lay.gp * Vp);
    auto* counts = reinterpret_cast<unsigned long long*>(ws + lay.counts);
    auto* hist = reinterpret_cast<uint32_t*>(ws + lay.hist);
    auto* sel = reinterpret_cast<SelState*>(ws + lay.sel);
    auto* slab = reinterpret_cast<SlabEntry*>(ws + lay.slab);
    const int planes = 2 * g.np;

    const unsigned ge = (unsigned)std::min<int64_t>(ceil_div64((int64_t)D * H, EB / 64), 2048);
    surf_edge_x_kernel<FLT><<<dim3(ge, g.np), EB, 0, st>>>(g, Vp, edges, dist, counts);
    CTU_CHECK_LAUNCH("surface edges");
    const int ly = line_lanes(H), lz = line_lanes(D);
    const int nby = ceil_div(W, ly), nbz = ceil_div(W, lz);
    surf_line_kernel<FLT><<<dim3((unsigned)(D * nby), planes), ly, (size_t)6 * H * ly, st>>>(
        g, Vp, dist, H, (int64_t)W, (int64_t)H * W, nby, 1);
    CTU_CHECK_LAUNCH("surface edt y");
    surf_line_kernel<FLT><<<dim3((unsigned)(H * nbz), planes), lz, (size_t)6 * D * lz, st>>>(
        g, Vp, dist, D, (int64_t)H * W, (int64_t)W, nbz, 0);
    CTU_CHECK_LAUNCH("surface edt z");
    surf_reduce_kernel<FLT><<<dim3(lay.RB, planes), RT, 0, st>>>(g, V, Vp, edges, dist, slab, lay.RB);
    CTU_CHECK_LAUNCH("surface reduce");
    if (g.pct >= 0.0) {
        const unsigned gs = (unsigned)ceil_div(planes, 64);
        surf_select_init_kernel<<<gs, 64, 0, st>>>(g, counts, sel);
        CTU_CHECK_LAUNCH("surface select init");
        for (int shift = 24; shift >= 0; shift -= 8) {
            surf_hist_kernel<<<dim3(lay.RB, planes), RT, 0, st>>>(g, V, Vp, edges, dist, sel, hist, lay.RB, shift);
            CTU_CHECK_LAUNCH("surface histogram");
            surf_select_kernel<<<gs, 64, 0, st>>>(g, sel, hist, shift);
            CTU_CHECK_LAUNCH("surface select");
        }
    }
    surf_final_kernel<FLT><<<(unsigned)ceil_div(g.np, 64), 64, 0, st>>>(g, counts, slab, sel, lay.RB, out);
    CTU_CHECK_LAUNCH("surface final");
    return CTU_OK;
}

bool dtype_ok(int t) { return t == CTU_U8 || t == CTU_I64 || t == CTU_F32; }

}  // namespace

extern "C" size_t ctu_surface_ws_bytes(int N, int Cs, int D, int H, int W) {
    if (N <= 0 || Cs <= 0 || Cs > MAXC || D <= 0 || H <= 0 || W <= 0) return 0;
    return layout(N, Cs, D, H, W).total;
}

extern "C" int ctu_surface_metrics(const void* pred, int pred_dtype, int pred_onehot, const void* target, int target_dtype,
                                   int target_onehot, int N, int C, int cls0, int Cs, int D, int H, int W,
                                   const float* spacing, const double* tau, double percentile, float* out, void* ws,
                                   void* stream) {
    CTU_REQUIRE(pred && target && out && ws, "surface_metrics: null pointer");
    CTU_REQUIRE(dtype_ok(pred_dtype) && dtype_ok(target_dtype), "surface_metrics: unsupported dtype");
    CTU_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "surface_metrics: bad shape");
    CTU_REQUIRE(sides_ok(D, H, W), "surface_metrics: volume side above %d", MAX_SIDE);
    CTU_REQUIRE(Cs >= 1 && Cs <= MAXC && (cls0 == 0 || cls0 == 1) && cls0 + Cs <= C && C <= MAXC + 1,
                "surface_metrics: bad classes C=%d cls0=%d Cs=%d", C, cls0, Cs);
    CTU_REQUIRE((int64_t)N * Cs <= (1 << 20), "surface_metrics: too many (item, class) pairs");
    CTU_REQUIRE(percentile < 0.0 || percentile <= 100.0, "surface_metrics: percentile above 100");
    bool unit = true;
    if (spacing) {
        for (int i = 0; i < 3 * N; ++i) {
            CTU_REQUIRE(spacing[i] > 0.f && spacing[i] < __builtin_inff(), "surface_metrics: spacing must be positive and finite");
            unit = unit && spacing[i] == 1.f;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const Layout lay = layout(N, Cs, D, H, W);
    uint8_t* w = (uint8_t*)ws;
    const int pairs = N * Cs;
    // counters and histograms are accumulated into: zeroed once per call (the select pass re-zeroes its histograms)
    if (hipMemsetAsync(w + lay.counts, 0, lay.sel - lay.counts, st) != hipSuccess) {
        ctu_set_error("surface_metrics: memset failed");
        return CTU_ELAUNCH;
    }
    GroupArgs g;
    g.a = Side{pred, pred_dtype, pred_onehot ? 1 : 0};
    g.b = Side{target, target_dtype, target_onehot ? 1 : 0};
    g.Ct = C; g.cls0 = cls0; g.Cs = Cs; g.D = D; g.H = H; g.W = W;
    g.has_tau = tau != nullptr;
    g.pairs = pairs;
    g.pct = percentile < 0.0 ? -1.0 : percentile;
    for (int k = 0; k < MAXC; ++k) g.tau[k] = (tau && k < Cs) ? tau[k] : 0.0;
    for (int p0 = 0; p0 < pairs; p0 += lay.gp) {
        g.pair0 = p0;
        g.np = std::min(lay.gp, pairs - p0);
        for (int i = 0; i < MAXG; ++i) {
            const int n = (p0 + std::min(i, g.np - 1)) / Cs;
            for (int a = 0; a < 3; ++a) g.sp[i][a] = spacing ? spacing[3 * n + a] : 1.f;
        }
        const int rc = unit ? run_group<false>(g, lay, w, out, st) : run_group<true>(g, lay, w, out, st);
        if (rc != CTU_OK) return rc;
    }
    return CTU_OK;
}

// ------------------------------------------------------------------------------------------------ Hausdorff
namespace {
// workspace: the float label map of the prediction, the 8 rows of ctu_surface_metrics, its workspace
size_t hd_seg_bytes(int N, int D, int H, int W) { return align256((size_t)N * D * H * W * sizeof(float)); }
size_t hd_rows_bytes(int N, int C) { return align256((size_t)8 * N * (C - 1) * sizeof(float)); }
}  // namespace

extern "C" size_t ctu_hausdorff_ws_bytes(int N, int C, int D, int H, int W) {
    if (N <= 0 || C < 2 || D <= 0 || H <= 0 || W <= 0) return 0;
    return hd_seg_bytes(N, D, H, W) + hd_rows_bytes(N, C) + align256(ctu_surface_ws_bytes(N, C - 1, D, H, W));
}

extern "C" int ctu_hausdorff(const float* pred, const float* target, int N, int C, int D, int H, int W, float* out, void* ws,
                             void* stream) {
    CTU_REQUIRE(pred && target && out && ws, "hausdorff: null pointer");
    CTU_REQUIRE(N > 0 && C >= 2 && C <= 8 && D > 0 && H > 0 && W > 0, "hausdorff: bad shape N=%d C=%d", N, C);
    CTU_REQUIRE(sides_ok(D, H, W), "hausdorff: volume side above %d", MAX_SIDE);
    CTU_REQUIRE(N * (C - 1) * 2 <= 65535, "hausdorff: too many (item, class) planes");
    float* seg = (float*)ws;
    float* rows = (float*)((uint8_t*)ws + hd_seg_bytes(N, D, H, W));
    int rc = ctu_hard_segm(pred, N, C, (int64_t)D * H * W, seg, stream);
    if (rc != CTU_OK) return rc;
    rc = ctu_surface_metrics(seg, CTU_F32, 0, target, CTU_F32, 1, N, C, 1, C - 1, D, H, W, nullptr, nullptr, -1.0, rows,
                             (uint8_t*)rows + hd_rows_bytes(N, C), stream);
    if (rc != CTU_OK) return rc;
    const size_t pairs = (size_t)N * (C - 1);                         // row 1 of the block: hd
    if (hipMemcpyAsync(out, rows + pairs, pairs * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
        ctu_set_error("hausdorff: copy failed");
        return CTU_ELAUNCH;
    }
    return CTU_OK;
}
