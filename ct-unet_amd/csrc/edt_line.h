// The exact squared Euclidean distance transform shared by surface.hip (surface metrics, Hausdorff) and distance.hip
// (public distance transform): the x pass of one row from a wave's site masks (row_nearest), then one line of the y / z
// passes, the linear-time lower envelope of parabolas (Felzenszwalb-Huttenlocher, edt_line).
//
// edt_line:
// One lane owns one line of length L (element stride lstride) and one column [entry][lane] of the block's LDS stack:
// values Fs (T) and positions Vs (uint16), 6 bytes per entry, so a block of NL lanes needs 6 L NL bytes and a line may be
// at most 64 KB / (6 x 8 lanes) = 1365 elements long (line_lanes picks NL; the callers cap every side at 1024).
//   f(q) = min_k src(k) + s2 (q - k)^2 over the finite src(k), written in place.
// The intersection of parabolas a < b lies at num / den with num = (f_b - f_a) + s2 (b - a)(b + a), den = 2 (b - a) > 0
// (s2 cancels from the comparison).  Unit spacing: int32 squared distances, 64-bit products, exact; otherwise fp32.
// TRACK: also record the k that attains the minimum (int16, -1 on a line without a finite entry) at sel[q * lstride]; on
// a tie the later k wins.  Without TRACK the code is what surface.hip always ran.
#pragma once
#include "common.h"
#include "voxel_rows.h"

namespace ctu_edt {

using ctu_vox::NONE_POS;

constexpr int INF_I = 0x3fffffff;       // "no site on this line" in the int32 maps (3 * 1023^2 << INF_I)
constexpr int LINE_LDS = 64 * 1024;     // LDS budget of one line-pass block

template <bool FLT> struct DistT;
template <> struct DistT<false> { typedef int T; typedef long long A; };
template <> struct DistT<true> { typedef float T; typedef float A; };

__device__ __forceinline__ bool is_inf(int v) { return v == INF_I; }
__device__ __forceinline__ bool is_inf(float v) { return v == __builtin_inff(); }
template <bool FLT> __device__ __forceinline__ typename DistT<FLT>::T dist_inf();
template <> __device__ __forceinline__ int dist_inf<false>() { return INF_I; }
template <> __device__ __forceinline__ float dist_inf<true>() { return __builtin_inff(); }

// lanes per block of a line pass over lines of length L: as many of 64 as the LDS budget admits, at least 8
inline int line_lanes(int L) {
    int nl = 64;
    while (nl > 8 && (size_t)6 * L * nl > (size_t)LINE_LDS) nl >>= 1;
    return nl;
}

// The x pass of one image row, one wave per row: lane `lane` owns the 16 voxels x0 = 16 lane .. x0 + 15 and brings the
// 16-bit mask `es` of the sites among them (0 for a lane past the row's end).  val[u] = sx2 (x - k)^2 for the nearest site
// k of the row, dist_inf on a row without sites; with TRACK pos[u] = that k (-1: none; on a tie the site on the left).
// Per-lane bit scans find the sites inside the lane, two wave scans (prefix max of the lanes' last site, suffix min of
// their first) the nearest ones outside it.  Every lane of the wave must call.
template <bool FLT, bool TRACK>
__device__ __forceinline__ void row_nearest(uint32_t es, int x0, int lane, float sx2, typename DistT<FLT>::T val[16],
                                            int16_t pos[16]) {
    typedef typename DistT<FLT>::T T;
    int last = es ? x0 + 31 - __clz(es) : -1;
    int first = es ? x0 + __ffs(es) - 1 : NONE_POS;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int tl = __shfl_up(last, o), tf = __shfl_down(first, o);
        if (lane >= o) last = max(last, tl);
        if (lane + o < 64) first = min(first, tf);
    }
    int prev_last = __shfl_up(last, 1), next_first = __shfl_down(first, 1);
    if (lane == 0) prev_last = -1;
    if (lane == 63) next_first = NONE_POS;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int x = x0 + u;
        const uint32_t le = es & ((2u << u) - 1u), re = es >> u;
        const int lp = le ? x0 + 31 - __clz(le) : prev_last;
        const int rp = re ? x + __ffs(re) - 1 : next_first;
        int dmin = NONE_POS, at = -1;
        if (lp >= 0) { dmin = x - lp; at = lp; }
        if (rp < NONE_POS) {
            if (TRACK && rp - x < dmin) at = rp;
            dmin = min(dmin, rp - x);
        }
        if (dmin == NONE_POS) val[u] = dist_inf<FLT>();
        else if (FLT) val[u] = (T)(sx2 * (float)(dmin * dmin));
        else val[u] = (T)(dmin * dmin);
        if (TRACK) pos[u] = (int16_t)at;
    }
}

// the first nv (<= 16) of a lane's 16 values (distances: 4 bytes, positions: 2) to p: 16-byte stores where all 16 go to
// an aligned p
template <class T>
__device__ __forceinline__ void store16(T* p, int nv, const T v[16]) {
    constexpr int PER = 16 / (int)sizeof(T);        // values of one 16-byte store
    typedef T Vec __attribute__((ext_vector_type(PER)));
    if (nv == 16 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 16 / PER; ++q) {
            Vec w;
#pragma unroll
            for (int u = 0; u < PER; ++u) w[u] = v[q * PER + u];
            reinterpret_cast<Vec*>(p)[q] = w;
        }
    } else {
        for (int u = 0; u < nv; ++u) p[u] = v[u];
    }
}

// no barriers: every lane owns its line and its LDS column
template <bool FLT, bool TRACK>
__device__ __forceinline__ void edt_line(typename DistT<FLT>::T* d, int L, int64_t lstride, typename DistT<FLT>::T s2,
                                         typename DistT<FLT>::T* Fs, uint16_t* Vs, int NL, int lane, int16_t* sel) {
    typedef typename DistT<FLT>::T T;
    typedef typename DistT<FLT>::A A;
    int n = 0, vtop = 0;
    T ftop = 0;
    A zn = 0, zd = 1;                      // intersection of the two top entries (valid when n >= 2)
    for (int q0 = 0; q0 < L; q0 += 8) {
        T buf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) buf[u] = (q0 + u < L) ? d[(int64_t)(q0 + u) * lstride] : dist_inf<FLT>();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int q = q0 + u;
            const T fq = buf[u];
            if (q >= L || is_inf(fq)) continue;
            A num = 0, den = 1;
            while (n > 0) {
                num = (A)(fq - ftop) + (A)s2 * (A)((q - vtop) * (q + vtop));
                den = (A)(2 * (q - vtop));
                if (n >= 2 && num * zd <= zn * den) {
                    --n;
                    vtop = Vs[(n - 1) * NL + lane];
                    ftop = Fs[(n - 1) * NL + lane];
                    if (n >= 2) {
                        const int va = Vs[(n - 2) * NL + lane];
                        const T fa = Fs[(n - 2) * NL + lane];
                        zn = (A)(ftop - fa) + (A)s2 * (A)((vtop - va) * (vtop + va));
                        zd = (A)(2 * (vtop - va));
                    }
                } else {
                    break;
                }
            }
            if (n > 0) { zn = num; zd = den; }
            Fs[n * NL + lane] = fq;
            Vs[n * NL + lane] = (uint16_t)q;
            ++n;
            vtop = q;
            ftop = fq;
        }
    }
    if (n == 0) {
        for (int q = 0; q < L; ++q) {
            d[(int64_t)q * lstride] = dist_inf<FLT>();
            if (TRACK) sel[(int64_t)q * lstride] = (int16_t)-1;
        }
        return;
    }
    int j = 0, vj = Vs[lane], vn = 0;
    T fj = Fs[lane], fn = 0;
    if (n > 1) { vn = Vs[NL + lane]; fn = Fs[NL + lane]; }
    for (int q = 0; q < L; ++q) {
        T ej = fj + s2 * (T)((q - vj) * (q - vj));
        while (j + 1 < n) {
            const T en = fn + s2 * (T)((q - vn) * (q - vn));
            if (en > ej) break;
            ++j; vj = vn; fj = fn; ej = en;
            if (j + 1 < n) { vn = Vs[(j + 1) * NL + lane]; fn = Fs[(j + 1) * NL + lane]; }
        }
        d[(int64_t)q * lstride] = ej;
        if (TRACK) sel[(int64_t)q * lstride] = (int16_t)vj;
    }
}

}  // namespace ctu_edt
