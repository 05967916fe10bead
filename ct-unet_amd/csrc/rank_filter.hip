// Rank filters on the device, gfx950: median, percentile, minimum and maximum over a box of up to 7 x 7 x 7 voxels (rule:
// ctunet_amd/preprocess.py; tests/rank_ref.py restates it).  One launch per 65535 items, no workspace, no atomics, no host
// synchronisation; the output has the input's dtype and carries the selected element's own bits.
//
// Every element becomes an unsigned KEY that preserves the order and is a bijection on its bits (uint8: the value; int16:
// value + 32768; float32: ~b for a set sign bit, else b | 0x80000000), 16 bits wide for uint8 / int16 and 32 for float32.
// A block of 256 threads owns a tile of TZ = 8 planes x TY = 4 rows x TX = 64 voxels.
//   stage       the one loader of all three kernels: the tile's box with its halo goes into LDS AS KEYS.  A thread takes 16
//               bytes of a row on the row's own 16-byte grid; a chunk that lies inside the volume is one 16-byte load, the
//               chunks at the clipped ends and everything outside the volume are read voxel by voxel through the border rule
//               (per axis: clamp, scipy's reflect, the constant's key), so every global read sits behind a mapped index and
//               the selection code knows no border.  `flip` (all ones) stages ~key: rank r of the flipped keys is rank
//               n - 1 - r of the keys, which halves the ranks the 3 x 3 x 3 kernel is instantiated for and makes the maximum
//               the minimum's kernel.
//   fast3       3 x 3 x 3, ranks 1..25.  A thread owns one (y, x) column of the tile and walks z.  Each plane's 3 x 3
//               neighbourhood is read once (9 LDS reads) and sorted by a 9-input network; two consecutive planes are merged
//               once into a sorted 18 that serves two outputs; an output picks its rank from a sorted 9 and that 18 by one
//               more merge network of which only the wanted output is kept.  Element i of a sorted list of m that is merged
//               with n others lands on a rank in [i, i + n], so the lists are cut to the elements that can hold the rank
//               before they are merged; the rest of the pruning is the compiler's dead-code elimination (the networks are
//               Batcher's odd-even merges, expanded at compile time; pads are the constant all-ones key, which min / max
//               fold away).  Everything is min / max on 32-bit registers: no local array survives, scratch is 0.
//   separable   rank 0 and rank n - 1 at any size: a running minimum of the (flipped) keys along x, then y, then z, in place
//               in the staged box.  x: a wave owns a row and reads before it writes; y and z: a thread owns a column and
//               walks it upwards, so what it overwrites is never read again.  Bit-equal to the rule: the key order is total.
//   generic     every other size and rank: a most-significant-bit-first search on the key.  With res the bits found so far,
//               cand = res | bit, and the bit stays iff fewer than rank + 1 window keys lie below cand: 16 or 32 passes
//               over the n keys of the window in LDS, exact, nothing allocated.  The x side of the window is a template
//               argument (a row's reads go out together) and a thread searches two x-neighbours at once on shared reads.
//   store       results are keys in LDS; a thread turns 16 bytes of an output row on that row's 16-byte grid back into
//               elements and stores them at once; the chunks cut by the tile's or the row's end go voxel by voxel.
// CTU_RANK_PATH=generic in the environment sends every call down the generic kernel (the A/B of profiles/rank.md).
// Measured: profiles/rank.md.
//
// No reference counterpart: the reference's datasets load volumes that were filtered beforehand.
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "common.h"
#include "voxel_rows.h"

namespace {

constexpr int RB = 256;
constexpr int TX = CTU_RANK_TILE_X, TY = CTU_RANK_TILE_Y, TZ = CTU_RANK_TILE_Z;
constexpr int MAX_SIZE = CTU_RANK_MAX_SIZE;
constexpr int MAX_BATCH = 65535;                // grid.y
constexpr int NEAREST = CTU_GAUSS_NEAREST, REFLECT = CTU_GAUSS_REFLECT, CONSTANT = CTU_GAUSS_CONSTANT;
static_assert(TX == 64 && TY == 4 && TY * 64 == RB && TZ % 2 == 0, "a wave owns a row of the tile; fast3 forms two planes a step");

// ------------------------------------------------------------------------------------------------ keys
template <class T> struct Key;
template <> struct Key<uint8_t> {
    typedef uint16_t K;
    static __host__ __device__ __forceinline__ uint32_t to(uint8_t v) { return v; }
    static __device__ __forceinline__ uint8_t from(uint32_t k) { return (uint8_t)k; }
};
template <> struct Key<int16_t> {
    typedef uint16_t K;
    static __host__ __device__ __forceinline__ uint32_t to(int16_t v) { return (uint16_t)v ^ 0x8000u; }
    static __device__ __forceinline__ int16_t from(uint32_t k) { return (int16_t)(uint16_t)(k ^ 0x8000u); }
};
template <> struct Key<float> {
    typedef uint32_t K;
    static __host__ __device__ __forceinline__ uint32_t to(float v) {
        uint32_t b;
        memcpy(&b, &v, 4);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    static __device__ __forceinline__ float from(uint32_t k) {
        const uint32_t b = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
        return __uint_as_float(b);
    }
};

struct RankArgs {
    int D, H, W;
    int sz, sy, sx;
    int rank;
    int mode;
    uint32_t ckey;                              // the constant's key, flipped like every staged key
    uint32_t flip;                              // 0, or all ones of the key's width
    int ntx, nty;
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

struct Origin { int X0, Y0, Z0; };
__device__ __forceinline__ Origin origin(const RankArgs& a) {
    int bi = blockIdx.x;
    const int tx = bi % a.ntx;
    bi /= a.ntx;
    return {tx * TX, bi % a.nty * TY, bi / a.nty * TZ};
}

// ------------------------------------------------------------------------------------------------ the loader
// box[SZ][SY][SX] (SZ = TZ + sz - 1, ...) = the flipped keys of the voxels [Z0 - rz, ..) x [Y0 - ry, ..) x [X0 - rx, ..)
template <class T>
__device__ __forceinline__ void stage(const RankArgs& a, const T* __restrict__ item, const Origin& t,
                                      typename Key<T>::K* __restrict__ box) {
    typedef typename Key<T>::K K;
    constexpr int PER = 16 / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(PER)));
    const int SX = TX + a.sx - 1, SY = TY + a.sy - 1, SZ = TZ + a.sz - 1;
    const int lo = t.X0 - (a.sx >> 1), hi = lo + SX;            // the staged positions of a row
    const int va = max(lo, 0), vb = min(hi, a.W);               // ... and those of them inside the volume
    const int nch = (SX + PER - 1) / PER + 1;                   // 16-byte chunks that can touch [lo, hi) on any grid
    for (int it = threadIdx.x; it < SZ * SY * nch; it += RB) {
        const int c = it % nch, row = it / nch;
        const int z = border(t.Z0 - (a.sz >> 1) + row / SY, a.D, a.mode);
        const int y = border(t.Y0 - (a.sy >> 1) + row % SY, a.H, a.mode);
        K* dst = box + row * SX - lo;                           // dst[x]: position x of the row
        const bool outside = z < 0 || y < 0;
        const T* grow = item + ((int64_t)(outside ? 0 : z) * a.H + (outside ? 0 : y)) * a.W;
        // the grid of the row: position lo sits e elements behind a 16-byte boundary (an address is not formed for lo < 0)
        const int e = (int)(((int64_t)((uintptr_t)grow / sizeof(T)) + lo) & (PER - 1));
        const int cs = lo - e + c * PER;
        if (!outside && cs >= va && cs + PER <= vb) {
            const Vec v = *reinterpret_cast<const Vec*>(grow + cs);
#pragma unroll
            for (int u = 0; u < PER; ++u) dst[cs + u] = (K)(Key<T>::to(v[u]) ^ a.flip);
        } else {
            for (int x = max(cs, lo); x < min(cs + PER, hi); ++x) {
                const int xi = outside ? -1 : border(x, a.W, a.mode);
                dst[x] = xi < 0 ? (K)a.ckey : (K)(Key<T>::to(grow[xi]) ^ a.flip);
            }
        }
    }
}

// res: the tile's result keys, voxel (z, y, x) of the tile at res[z * plane + y * row + x]
template <class T>
__device__ __forceinline__ void store_tile(const RankArgs& a, T* __restrict__ oitem, const Origin& t,
                                           const typename Key<T>::K* __restrict__ res, int row, int plane) {
    constexpr int PER = 16 / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(PER)));
    constexpr int NCH = TX / PER + 1;
    const int xe = min(t.X0 + TX, a.W);
    for (int it = threadIdx.x; it < TZ * TY * NCH; it += RB) {
        const int c = it % NCH, r = it / NCH;
        const int y = t.Y0 + r % TY, z = t.Z0 + r / TY;
        if (z >= a.D || y >= a.H) continue;
        T* orow = oitem + ((int64_t)z * a.H + y) * a.W;
        const int e = (int)(((uintptr_t)orow / sizeof(T) + t.X0) & (PER - 1));
        const int cs = t.X0 - e + c * PER;
        const int xa = max(cs, t.X0), xb = min(cs + PER, xe);
        if (xa >= xb) continue;
        const typename Key<T>::K* src = res + (r / TY) * plane + (r % TY) * row - t.X0;
        if (xb - xa == PER) {
            Vec v;
#pragma unroll
            for (int u = 0; u < PER; ++u) v[u] = Key<T>::from(src[cs + u] ^ a.flip);
            *reinterpret_cast<Vec*>(orow + cs) = v;
        } else {
            for (int x = xa; x < xb; ++x) orow[x] = Key<T>::from(src[x] ^ a.flip);
        }
    }
}

// ------------------------------------------------------------------------------------------------ networks
// The compare-exchanges of the stages p = p0, 2 p0, .. < n of Batcher's odd-even merge sort on n inputs: p0 = 1 sorts,
// p0 = n / 2 merges two sorted halves.
struct CeList {
    int n;
    unsigned char a[96], b[96];
};
constexpr CeList batcher(int n, int p0) {
    CeList l{};
    for (int p = p0; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= n - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < n - j - k - 1 ? k - 1 : n - j - k - 1); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        l.a[l.n] = (unsigned char)(i + j);
                        l.b[l.n] = (unsigned char)(i + j + k);
                        ++l.n;
                    }
    return l;
}
constexpr CeList SORT9 = batcher(9, 1), MERGE32 = batcher(32, 16);
constexpr uint32_t PAD = 0xffffffffu;           // not below any key: a pad never moves down, min / max with it fold away

template <int A, int B> __device__ __forceinline__ void ce(uint32_t* w) {
    const uint32_t lo = w[A] < w[B] ? w[A] : w[B], hi = w[A] < w[B] ? w[B] : w[A];
    w[A] = lo;
    w[B] = hi;
}
template <size_t... I> __device__ __forceinline__ void sort9(uint32_t* w, std::index_sequence<I...>) {
    (ce<SORT9.a[I], SORT9.b[I]>(w), ...);
}
template <size_t... I> __device__ __forceinline__ void merge32(uint32_t* w, std::index_sequence<I...>) {
    (ce<MERGE32.a[I], MERGE32.b[I]>(w), ...);
}

// w[0 ..] = the sorted union of the sorted a[0 .. NA) and b[0 .. NB), NA, NB <= 16
template <int NA, int NB> __device__ __forceinline__ void merge(const uint32_t* a, const uint32_t* b, uint32_t* w) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        w[i] = i < NA ? a[i] : PAD;
        w[16 + i] = i < NB ? b[i] : PAD;
    }
    merge32(w, std::make_index_sequence<MERGE32.n>());
}

// the sorted keys of the 3 x 3 neighbourhood whose corner is p
template <class K> __device__ __forceinline__ void plane9(const K* p, int SX, uint32_t* s) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) s[3 * j + i] = p[j * SX + i];
    sort9(s, std::make_index_sequence<SORT9.n>());
}

// the key of rank RANK (<= 13) among a sorted 9 and a sorted 18: only one[0 .. RANK] and pair[RANK - 9 .. RANK] can hold it
template <int RANK> __device__ __forceinline__ uint32_t select27(const uint32_t* one, const uint32_t* pair) {
    constexpr int N1 = RANK + 1 < 9 ? RANK + 1 : 9;
    constexpr int P0 = RANK > 9 ? RANK - 9 : 0, NP = RANK + 1 - P0;
    static_assert(RANK >= 1 && RANK <= 13 && NP <= 16, "ranks above 13 are taken on flipped keys");
    uint32_t w[32];
    merge<N1, NP>(one, pair + P0, w);
    return w[RANK - P0];                        // the P0 elements cut from below all lie below the rank
}

template <class T, int RANK>
__global__ void __launch_bounds__(RB) rank_fast3_kernel(RankArgs a, const T* __restrict__ in, T* __restrict__ out) {
    typedef typename Key<T>::K K;
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int SX = TX + 2, SY = TY + 2, SZ = TZ + 2;
    K* box = reinterpret_cast<K*>(smem);
    K* res = box + SZ * SY * SX;
    const Origin t = origin(a);
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    stage<T>(a, in + (int64_t)blockIdx.y * vox, t, box);
    __syncthreads();
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    if (t.X0 + x < a.W && t.Y0 + y < a.H) {
        const K* col = box + y * SX + x;
        K* o = res + y * TX + x;
        uint32_t A[9], B[9];
        plane9(col, SX, A);
        plane9(col + SY * SX, SX, B);
#pragma unroll 1
        for (int i = 0; i < TZ / 2; ++i) {      // A, B: planes 2 i and 2 i + 1 of the box; outputs 2 i and 2 i + 1
            uint32_t Cn[9], En[9], M[32];
            plane9(col + (2 * i + 2) * SY * SX, SX, Cn);
            merge<9, 9>(B, Cn, M);
            o[(2 * i) * TY * TX] = (K)select27<RANK>(A, M);
            plane9(col + (2 * i + 3) * SY * SX, SX, En);
            o[(2 * i + 1) * TY * TX] = (K)select27<RANK>(En, M);
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                A[q] = Cn[q];
                B[q] = En[q];
            }
        }
    }
    __syncthreads();
    store_tile<T>(a, out + (int64_t)blockIdx.y * vox, t, res, TX, TY * TX);
}

template <class T>
__global__ void __launch_bounds__(RB) rank_separable_kernel(RankArgs a, const T* __restrict__ in, T* __restrict__ out) {
    typedef typename Key<T>::K K;
    extern __shared__ __align__(16) unsigned char smem[];
    K* box = reinterpret_cast<K*>(smem);
    const int SX = TX + a.sx - 1, SY = TY + a.sy - 1, SZ = TZ + a.sz - 1;
    const Origin t = origin(a);
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    stage<T>(a, in + (int64_t)blockIdx.y * vox, t, box);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // x: every lane of the wave has read its window before any of them writes
    for (int r = wv; r < SZ * SY; r += RB / 64) {
        K* p = box + r * SX + lane;
        K m = p[0];
        for (int k = 1; k < a.sx; ++k) m = p[k] < m ? p[k] : m;
        p[0] = m;
    }
    __syncthreads();
    // y, then z: a thread walks its column upwards; the element it overwrites is below every window still to come
    for (int c = threadIdx.x; c < SZ * TX; c += RB) {
        K* p = box + (c / TX) * SY * SX + c % TX;
        for (int yo = 0; yo < TY; ++yo) {
            K m = p[yo * SX];
            for (int k = 1; k < a.sy; ++k) m = p[(yo + k) * SX] < m ? p[(yo + k) * SX] : m;
            p[yo * SX] = m;
        }
    }
    __syncthreads();
    {
        K* p = box + wv * SX + lane;
        for (int zo = 0; zo < TZ; ++zo) {
            K m = p[zo * SY * SX];
            for (int k = 1; k < a.sz; ++k) m = p[(zo + k) * SY * SX] < m ? p[(zo + k) * SY * SX] : m;
            p[zo * SY * SX] = m;
        }
    }
    __syncthreads();
    store_tile<T>(a, out + (int64_t)blockIdx.y * vox, t, box, SX, SY * SX);
}

// WX = the window's x side, a compile-time constant.  A thread searches the keys of two x-neighbours side by side: their
// windows share all but one key of a row, the row's WX + 1 keys start on an even position (aligned 4- or 8-byte LDS
// reads: 16-bit keys come two to a dword), and the two searches are independent chains.
template <class T, int WX>
__global__ void __launch_bounds__(RB) rank_generic_kernel(RankArgs a, const T* __restrict__ in, T* __restrict__ out) {
    typedef typename Key<T>::K K;
    constexpr int BITS = 8 * (int)sizeof(K);
    extern __shared__ __align__(16) unsigned char smem[];
    K* box = reinterpret_cast<K*>(smem);
    constexpr int SX = TX + WX - 1;
    static_assert(SX % 2 == 0 && TX % 2 == 0, "a pair's row starts on an even key");
    const int SY = TY + a.sy - 1, SZ = TZ + a.sz - 1;
    K* res = box + SZ * SY * SX;
    const Origin t = origin(a);
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    stage<T>(a, in + (int64_t)blockIdx.y * vox, t, box);
    __syncthreads();
    const int x = 2 * (threadIdx.x & 31), y = (threadIdx.x >> 5) & (TY - 1), z0 = (threadIdx.x >> 7) * (TZ / 2);
    if (t.X0 + x < a.W && t.Y0 + y < a.H) {
        for (int z = z0; z < z0 + TZ / 2 && t.Z0 + z < a.D; ++z) {
            const K* win = box + (z * SY + y) * SX + x;
            uint32_t r0 = 0, r1 = 0;
            for (int b = BITS - 1; b >= 0; --b) {
                const uint32_t c0 = r0 | (1u << b), c1 = r1 | (1u << b);
                int n0 = 0, n1 = 0;
                for (int dz = 0; dz < a.sz; ++dz)
                    for (int dy = 0; dy < a.sy; ++dy) {
                        const K* p = win + (dz * SY + dy) * SX;
                        uint32_t k[WX + 1];
                        if constexpr (sizeof(K) == 2) {
                            const uint32_t* p2 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                            for (int j = 0; j < (WX + 1) / 2; ++j) {
                                const uint32_t w = p2[j];
                                k[2 * j] = w & 0xffffu;
                                k[2 * j + 1] = w >> 16;
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j <= WX; ++j) k[j] = p[j];
                        }
#pragma unroll
                        for (int dx = 0; dx < WX; ++dx) {
                            n0 += k[dx] < c0;
                            n1 += k[dx + 1] < c1;
                        }
                    }
                if (n0 <= a.rank) r0 = c0;      // the key of rank `rank` is the largest v with at most `rank` keys below it
                if (n1 <= a.rank) r1 = c1;
            }
            K* o = res + (z * TY + y) * TX + x;
            o[0] = (K)r0;
            o[1] = (K)r1;                       // the neighbour may lie past the row's end: its box is staged, its key dropped
        }
    }
    __syncthreads();
    store_tile<T>(a, out + (int64_t)blockIdx.y * vox, t, res, TX, TY * TX);
}

enum Path { FAST3, SEPARABLE, GENERIC };

template <class T>
int launch_rank(RankArgs a, Path path, const void* in, int64_t N, void* out, double cval, hipStream_t st) {
    typedef typename Key<T>::K K;
    const int64_t vox = (int64_t)a.D * a.H * a.W;
    const int n = a.sz * a.sy * a.sx;
    const uint32_t ones = sizeof(K) == 2 ? 0xffffu : 0xffffffffu;
    a.flip = 0;
    if (path == SEPARABLE && a.rank != 0) a.flip = ones;        // the maximum: the minimum of the flipped keys
    if (path == FAST3 && a.rank > 13) {
        a.flip = ones;
        a.rank = n - 1 - a.rank;
    }
    a.ckey = (Key<T>::to((T)cval) ^ a.flip) & ones;
    a.ntx = ceil_div(a.W, TX);
    a.nty = ceil_div(a.H, TY);
    const size_t keys = (size_t)(TZ + a.sz - 1) * (TY + a.sy - 1) * (TX + a.sx - 1) + (path == SEPARABLE ? 0 : TZ * TY * TX);
    const size_t lds = keys * sizeof(K);                        // at most 47392 bytes: below the 64 KB every kernel may ask for
    for (int64_t n0 = 0; n0 < N; n0 += MAX_BATCH) {
        const dim3 g((unsigned)(a.ntx * a.nty * ceil_div(a.D, TZ)), (unsigned)(N - n0 < MAX_BATCH ? N - n0 : MAX_BATCH));
        const T* i = (const T*)in + n0 * vox;
        T* o = (T*)out + n0 * vox;
        if (path == SEPARABLE) {
            rank_separable_kernel<T><<<g, RB, lds, st>>>(a, i, o);
        } else if (path == GENERIC) {
            if (a.sx == 1) rank_generic_kernel<T, 1><<<g, RB, lds, st>>>(a, i, o);
            else if (a.sx == 3) rank_generic_kernel<T, 3><<<g, RB, lds, st>>>(a, i, o);
            else if (a.sx == 5) rank_generic_kernel<T, 5><<<g, RB, lds, st>>>(a, i, o);
            else rank_generic_kernel<T, 7><<<g, RB, lds, st>>>(a, i, o);
        } else {
            switch (a.rank) {
#define CTU_RANK_CASE(R) case R: rank_fast3_kernel<T, R><<<g, RB, lds, st>>>(a, i, o); break;
                CTU_RANK_CASE(1) CTU_RANK_CASE(2) CTU_RANK_CASE(3) CTU_RANK_CASE(4) CTU_RANK_CASE(5) CTU_RANK_CASE(6)
                CTU_RANK_CASE(7) CTU_RANK_CASE(8) CTU_RANK_CASE(9) CTU_RANK_CASE(10) CTU_RANK_CASE(11) CTU_RANK_CASE(12)
                CTU_RANK_CASE(13)
#undef CTU_RANK_CASE
                default: ctu_set_error("rank_filter: no 3 x 3 x 3 kernel of rank %d", a.rank); return CTU_EINVAL;
            }
        }
        CTU_CHECK_LAUNCH("rank_filter");
    }
    return CTU_OK;
}

bool cval_ok(int dtype, double c) {
    if (dtype == CTU_F32) return (double)(float)c - (double)(float)c == 0.0;    // finite once it is a float32
    const double lo = dtype == CTU_I16 ? -32768.0 : 0.0, hi = dtype == CTU_I16 ? 32767.0 : 255.0;
    return c >= lo && c <= hi && c == (double)(long long)c;
}

}  // namespace

extern "C" size_t ctu_rank_filter_ws_bytes(int64_t N, int D, int H, int W, const int* size) {
    (void)N; (void)D; (void)H; (void)W; (void)size;
    return 0;                                   // every path works in LDS
}

extern "C" int ctu_rank_filter(const void* in, int dtype, int64_t N, int D, int H, int W, const int* size, int rank,
                               int mode, double cval, void* out, void* ws, void* stream) {
    (void)ws;
    CTU_REQUIRE(in && out && size, "rank_filter: null pointer");
    CTU_REQUIRE(dtype == CTU_F32 || dtype == CTU_I16 || dtype == CTU_U8,
                "rank_filter: unsupported dtype %d (float32, int16 or uint8)", dtype);
    CTU_REQUIRE(mode >= NEAREST && mode <= CONSTANT, "rank_filter: unknown mode %d", mode);
    CTU_REQUIRE(N > 0 && ctu_vox::sides_ok(D, H, W), "rank_filter: bad shape N=%lld %dx%dx%d (every side in 1..%d)",
                (long long)N, D, H, W, ctu_vox::MAX_SIDE);
    for (int a = 0; a < 3; ++a)
        CTU_REQUIRE(size[a] >= 1 && size[a] <= MAX_SIZE && (size[a] & 1), "rank_filter: size %d of axis %d must be odd, 1..%d",
                    size[a], a, MAX_SIZE);
    const int n = size[0] * size[1] * size[2];
    CTU_REQUIRE(rank >= 0 && rank < n, "rank_filter: rank %d outside 0..%d", rank, n - 1);
    CTU_REQUIRE(cval_ok(dtype, cval), "rank_filter: cval %g is not representable in dtype %d", cval, dtype);
    RankArgs a;
    a.D = D; a.H = H; a.W = W;
    a.sz = size[0]; a.sy = size[1]; a.sx = size[2];
    a.rank = rank;
    a.mode = mode;
    const char* force = getenv("CTU_RANK_PATH");                // development A/B: "generic" for every call
    Path path = GENERIC;
    if (!(force && !strcmp(force, "generic"))) {
        if (rank == 0 || rank == n - 1) path = SEPARABLE;
        else if (a.sz == 3 && a.sy == 3 && a.sx == 3) path = FAST3;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == CTU_F32) return launch_rank<float>(a, path, in, N, out, cval, st);
    if (dtype == CTU_I16) return launch_rank<int16_t>(a, path, in, N, out, cval, st);
    return launch_rank<uint8_t>(a, path, in, N, out, cval, st);
}
