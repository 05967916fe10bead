// One line of an exact squared Euclidean distance transform: the linear-time lower envelope of parabolas
// (Felzenszwalb-Huttenlocher), shared by surface.hip (surface metrics) and distance.hip (public distance transform).
//
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

namespace ctu_edt {

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
