// On-device class-balanced random patch sampling for training, gfx950: a stated share of the patches of a batch is centred on
// a voxel of a chosen label class, the rest start anywhere.  Three entry points, no atomics and no host syncs, so index ->
// draw -> crop replays inside a captured graph and is bitwise reproducible:
//   ctu_patch_index  voxels of each of K classes per (item, chunk of CTU_PATCH_CHUNK voxels in C order); one read of the labels
//   ctu_patch_draw   one block per patch: class, k-th class voxel and jitter from Philox4x32-10 (philox.h) -> patch origin
//   ctu_patch_crop   typed, batched window gather on the 16-byte output tiling of chunk_tile.h
// The rules (RNG words, clamping, record layout) are pinned in ctunet_amd/sampling.py and include/ctunet_hip.h.
//
// Replaces: nothing in the reference: its datasets feed whole pre-resized volumes (ctunet/pytorch/datasets.py:89-112,195-235).
#include <string.h>

#include "chunk_tile.h"
#include "common.h"
#include "philox.h"

namespace {

using namespace ctu_rng;
using namespace ctu_tile;

constexpr int PB = 256;
constexpr int KMAX = CTU_PATCH_MAX_CLASSES;
constexpr int REC = CTU_PATCH_RECORD;
constexpr int SEG = 1024;                          // chunks per thread segment of the draw at most: V < 2^31
constexpr int ROUNDS = CTU_PATCH_CHUNK / PB;       // ballots per wave of the draw's rescan
static_assert(ROUNDS == 32 && ROUNDS * PB == CTU_PATCH_CHUNK, "one hit bit per round in a 32-bit word");

// lo + floor(r span / 2^32): uniform integer in [lo, lo + span) (augment.hip's rule)
__device__ __forceinline__ int64_t draw_int(uint32_t r, int64_t lo, uint64_t span) {
    return lo + (int64_t)(((uint64_t)r * span) >> 32);
}

// the K predicates: byte != 0 (any = 1, K = 1), or byte == cls[i]
struct Classes { int K, any; uint32_t cls[KMAX]; };

__device__ __forceinline__ bool in_class(const Classes& k, int i, uint32_t byte) {
    return k.any ? byte != 0 : byte == k.cls[i];
}

// nonzero bytes of a word: bit 7 of every byte that has any bit set, counted
__device__ __forceinline__ int nonzero_bytes(uint32_t x) {
    return __popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// the sum of s over the threads before this one and over the whole block; wtot: PB / 64 shared words, free on entry
__device__ __forceinline__ int64_t block_exclusive(int64_t s, int64_t* wtot, int64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = s;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int64_t before = 0;
    total = 0;
    for (int w = 0; w < PB / 64; ++w) {
        if (w < wave) before += wtot[w];
        total += wtot[w];
    }
    return before + inc - s;
}

// --------------------------------------------------------------------------------------------------------------- index
// grid (nchunks, M): block (c, n) counts, for every class, the voxels of flat indices [c CH, min(V, (c+1) CH)) of item n.
// An item with odd V starts at any byte, so the chunk is split at the 16-byte grid of its own address: up to 15 head bytes,
// whole 16-byte loads, up to 15 tail bytes.  One load feeds all K counters.
__global__ void __launch_bounds__(PB) patch_index_kernel(const uint8_t* __restrict__ labels, int64_t V, int nchunks,
                                                         Classes k, int32_t* __restrict__ counts) {
    const int c = blockIdx.x, n = blockIdx.y;
    const int64_t s0 = (int64_t)c * CTU_PATCH_CHUNK;
    const int len = (int)(min(V, s0 + CTU_PATCH_CHUNK) - s0);
    const uint8_t* p = labels + (int64_t)n * V + s0;
    const int head = min((int)((16 - ((uintptr_t)p & 15)) & 15), len);
    const int nvec = (len - head) >> 4;
    const int tail0 = head + (nvec << 4);
    int cnt[KMAX] = {0, 0, 0, 0};
    uint32_t pat[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) pat[i] = k.any ? 0u : k.cls[i] * 0x01010101u;
    for (int v = threadIdx.x; v < nvec; v += PB) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + head + (v << 4));
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
            if (i >= k.K) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt[i] += k.any ? nonzero_bytes(w[j]) : 4 - nonzero_bytes(w[j] ^ pat[i]);
        }
    }
    // the bytes either side of the 16-byte body: at most 30, one per thread
    const int edge = head + (len - tail0);
    if ((int)threadIdx.x < edge) {
        const int at = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
        const uint32_t b = p[at];
#pragma unroll
        for (int i = 0; i < KMAX; ++i)
            if (i < k.K) cnt[i] += in_class(k, i, b);
    }
    __shared__ int wsum[KMAX][PB / 64];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
        int t = cnt[i];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if ((threadIdx.x & 63) == 0) wsum[i][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < k.K) {
        int t = 0;
        for (int w = 0; w < PB / 64; ++w) t += wsum[threadIdx.x][w];
        counts[((int64_t)n * k.K + threadIdx.x) * nchunks + c] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- draw
struct DrawArgs {
    const uint8_t* labels;
    const int32_t* counts;
    const int32_t* items;
    const int64_t* counter;
    int M, P, nchunks;
    int n[3], p[3], jit[3];
    Classes k;
    double cum[KMAX];
    uint32_t k0, k1;
    int32_t* coords;
    int32_t* records;
};

// one block per patch j (record layout: ctunet_hip.h).  The counter is only read here; patch_advance_kernel adds P after
// this launch has finished, in stream order.
__global__ void __launch_bounds__(PB) patch_draw_kernel(DrawArgs a) {
    const int j = blockIdx.x;
    int32_t* rec = a.records + (int64_t)j * REC;
    int32_t* co = a.coords + (int64_t)j * 4;
    const int item = a.items[j];
    if (item < 0 || item >= a.M) {                    // block-uniform: nothing of the labels or the index is read
        if (threadIdx.x == 0) {
            for (int f = 0; f < REC; ++f) rec[f] = 0;
            rec[0] = rec[4] = rec[8] = rec[9] = rec[10] = -1;
            co[0] = -1;
            co[1] = co[2] = co[3] = 0;
        }
        return;
    }
    const int64_t V = (int64_t)a.n[0] * a.n[1] * a.n[2];
    const int64_t seq = a.counter[0] + j;
    const uint4 r = philox_seq(0, 0, seq, a.k0, a.k1);        // (r_class, r_k, -, -)
    const uint4 r2 = philox_seq(1, 0, seq, a.k0, a.k1);       // (r_z, r_y, r_x, -)
    const double u = unif_f64(r.x);
    int cls = -1;
    for (int i = a.k.K - 1; i >= 0; --i)
        if (u < a.cum[i]) cls = i;                    // the first i with u < cum_i: cum_{i-1} <= u < cum_i
    __shared__ int64_t wtot[PB / 64];
    __shared__ int wcnt[PB / 64];
    __shared__ int64_t sh_kloc, sh_idx;
    __shared__ int sh_seg, sh_chunk;
    int64_t total = 0, k = 0;                         // the same in every thread
    if (cls >= 0) {                                   // block-uniform, as is every branch around a barrier below
        const int32_t* cn = a.counts + ((int64_t)item * a.k.K + cls) * a.nchunks;
        const int per = (a.nchunks + PB - 1) / PB;    // chunks per thread segment, <= SEG
        const int c0 = min(a.nchunks, (int)threadIdx.x * per), c1 = min(a.nchunks, c0 + per);
        int64_t s = 0;
        for (int c = c0; c < c1; ++c) s += cn[c];
        if (threadIdx.x == 0) { sh_seg = sh_chunk = -1; sh_kloc = 0; sh_idx = -1; }
        const int64_t ex = block_exclusive(s, wtot, total);
        if (total > 0) {                              // the thread segment that holds the k-th class voxel
            k = draw_int(r.y, 0, (uint64_t)total);
            if (ex <= k && k < ex + s) { sh_seg = threadIdx.x; sh_kloc = k - ex; }
        }
        __syncthreads();
        if (sh_seg >= 0) {                            // ... and the chunk of the segment: up to SEG / PB chunks per thread
            const int q = (per + PB - 1) / PB;
            const int i0 = min(per, (int)threadIdx.x * q), i1 = min(per, i0 + q);
            const int64_t kseg = sh_kloc;
            int64_t s2 = 0;
            for (int i = i0; i < i1; ++i) s2 += sh_seg * per + i < a.nchunks ? cn[sh_seg * per + i] : 0;
            int64_t tot2;
            const int64_t ex2 = block_exclusive(s2, wtot, tot2);      // its barriers: every thread has read sh_kloc
            if (ex2 <= kseg && kseg < ex2 + s2) {
                int64_t kl = kseg - ex2;
                for (int i = i0; i < i1 && sh_seg * per + i < a.nchunks; ++i) {
                    const int64_t n = cn[sh_seg * per + i];
                    if (kl < n) { sh_chunk = sh_seg * per + i; sh_kloc = kl; break; }
                    kl -= n;
                }
            }
            __syncthreads();
            if (sh_chunk >= 0) {                      // ballot rescan of the chunk: a quarter per wave, 64 voxels per ballot
                const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
                const int64_t e = min(V, ((int64_t)sh_chunk + 1) * CTU_PATCH_CHUNK);
                const int64_t b0 = (int64_t)sh_chunk * CTU_PATCH_CHUNK + wave * (ROUNDS * 64);
                const uint8_t* lab = a.labels + (int64_t)item * V;
                uint32_t hits = 0;                    // bit `it`: voxel b0 + 64 it + lane is of the class
#pragma unroll
                for (int it = 0; it < ROUNDS; ++it) {
                    const int64_t i = b0 + it * 64 + lane;
                    if (i < e && in_class(a.k, cls, lab[i])) hits |= 1u << it;
                }
                int cnt = 0;
#pragma unroll
                for (int it = 0; it < ROUNDS; ++it) cnt += __popcll(__ballot((hits >> it) & 1u));
                if (lane == 0) wcnt[wave] = cnt;
                __syncthreads();
                int64_t kl = sh_kloc;
                for (int w = 0; w < wave; ++w) kl -= wcnt[w];
                if (kl >= 0 && kl < cnt) {            // wave-uniform: this quarter holds it
                    for (int it = 0; it < ROUNDS; ++it) {
                        const bool hit = (hits >> it) & 1u;
                        const uint64_t m = __ballot(hit);
                        const int pc = __popcll(m);
                        if (kl < pc) {
                            if (hit && __popcll(m & ((1ull << lane) - 1ull)) == kl) sh_idx = b0 + it * 64 + lane;
                            break;
                        }
                        kl -= pc;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int64_t idx = cls >= 0 ? sh_idx : -1;
    const int64_t hw = (int64_t)a.n[1] * a.n[2];
    const int ctr[3] = {idx < 0 ? -1 : (int)(idx / hw), idx < 0 ? -1 : (int)((idx / a.n[2]) % a.n[1]),
                        idx < 0 ? -1 : (int)(idx % a.n[2])};
    const uint32_t ra[3] = {r2.x, r2.y, r2.z};
    rec[0] = co[0] = item;
    for (int ax = 0; ax < 3; ++ax) {
        const int hi = max(0, a.n[ax] - a.p[ax]);
        int64_t s;
        if (idx < 0) {
            s = draw_int(ra[ax], 0, (uint64_t)hi + 1);
        } else {
            const int64_t jt = draw_int(ra[ax], -(int64_t)a.jit[ax], 2 * (uint64_t)a.jit[ax] + 1);
            s = min(max((int64_t)ctr[ax] - a.p[ax] / 2 + jt, (int64_t)0), (int64_t)hi);
        }
        rec[1 + ax] = co[1 + ax] = (int32_t)s;
        rec[8 + ax] = ctr[ax];
    }
    rec[4] = cls;
    rec[5] = cls >= 0 && total == 0;
    rec[6] = (int32_t)total;
    rec[7] = (int32_t)k;
    rec[11] = 0;
}

__global__ void patch_advance_kernel(int64_t* counter, int P) { counter[0] += P; }

// ---------------------------------------------------------------------------------------------------------------- crop
struct CropArgs {
    const void* src;
    const int32_t* coords;
    void* out;
    int64_t items;                                    // P * C output channels to write
    int Ms, C, D, H, W, pd, ph, pw, Ctot, oc, ntx, nty;
    double fill;
};

// grid (tiles of one [pd][ph][pw] channel, min(P C, 65535)): a block walks the output channels blockIdx.y, + gridDim.y, ...
// and writes its tile of each; a thread owns one 16-byte chunk of one output row, which is one span of one source row.
template <class S, class O>
__global__ void __launch_bounds__(SB) patch_crop_kernel(CropArgs a) {
    constexpr int VX = 16 / (int)sizeof(O);
    const Origin t = origin<O>(a.ntx, a.nty);
    int yy, zz;
    row_of(t, yy, zz);
    if (yy >= a.ph || zz >= a.pd) return;
    const O fill = (O)a.fill;
    const int64_t pv = (int64_t)a.pd * a.ph * a.pw;
    const int64_t rowoff = ((int64_t)zz * a.ph + yy) * a.pw;
    for (int64_t it = blockIdx.y; it < a.items; it += gridDim.y) {
        const int64_t p = it / a.C;
        const int c = (int)(it % a.C);
        O* orow = static_cast<O*>(a.out) + (p * a.Ctot + a.oc + c) * pv + rowoff;
        const Span s = chunk_of(orow, t.X0, a.pw);
        if (s.xa >= s.xb) continue;
        const int32_t* co = a.coords + p * 4;
        const int item = co[0];
        const int64_t z = (int64_t)co[1] + zz, y = (int64_t)co[2] + yy, x = (int64_t)co[3] + s.cx;
        const bool live = item >= 0 && (a.Ms == 1 || item < a.Ms) && z >= 0 && z < a.D && y >= 0 && y < a.H;
        Chunk<O> res;
#pragma unroll
        for (int v = 0; v < VX; ++v) res.v[v] = fill;
        if (live) {
            const int64_t m = a.Ms == 1 ? 0 : item;
            const S* srow = static_cast<const S*>(a.src) + (((m * a.C + c) * a.D + z) * a.H + y) * a.W;
            if (x >= 0 && x + VX <= a.W) {            // the whole chunk lies inside the source row: one load
                S tmp[VX];
                memcpy(tmp, srow + x, sizeof(tmp));
#pragma unroll
                for (int v = 0; v < VX; ++v) res.v[v] = (O)tmp[v];
            } else {
#pragma unroll
                for (int v = 0; v < VX; ++v)
                    if (x + v >= 0 && x + v < a.W) res.v[v] = (O)srow[x + v];
            }
        }
        store(orow, s, res, true);
    }
}

template <class S, class O>
int launch_crop(CropArgs a, hipStream_t stream) {
    const int64_t pv = (int64_t)a.pd * a.ph * a.pw;
    const Tiles tl = tiles(a.pd, a.ph, a.pw, static_cast<O*>(a.out) + (int64_t)a.oc * pv, sizeof(O));
    a.ntx = tl.ntx;
    a.nty = tl.nty;
    const unsigned gy = (unsigned)std::min<int64_t>(a.items, 65535);
    patch_crop_kernel<S, O><<<dim3(tl.blocks, gy), SB, 0, stream>>>(a);
    CTU_CHECK_LAUNCH("patch_crop");
    return CTU_OK;
}

int classes_of(int K, const int* classes, Classes* k, const char* who) {
    CTU_REQUIRE(K >= 1 && K <= KMAX, "%s: %d classes (1..%d)", who, K, KMAX);
    CTU_REQUIRE(classes || K == 1, "%s: the nonzero predicate (classes = NULL) is one class, got K = %d", who, K);
    k->K = K;
    k->any = classes ? 0 : 1;
    for (int i = 0; i < KMAX; ++i) k->cls[i] = 0;
    for (int i = 0; classes && i < K; ++i) {
        CTU_REQUIRE(classes[i] >= 0 && classes[i] <= 255, "%s: class %d outside 0..255", who, classes[i]);
        k->cls[i] = (uint32_t)classes[i];
    }
    return CTU_OK;
}

}  // namespace

extern "C" int ctu_patch_index(const uint8_t* labels, int M, int64_t V, int K, const int* classes, int32_t* counts,
                               void* stream) {
    CTU_REQUIRE(labels && counts, "patch_index: null pointer");
    CTU_REQUIRE(M > 0 && M <= 65535 && V > 0 && V < ((int64_t)1 << 31), "patch_index: bad shape M=%d V=%lld", M, (long long)V);
    Classes k;
    if (int e = classes_of(K, classes, &k, "patch_index")) return e;
    const int nchunks = (int)ceil_div64(V, CTU_PATCH_CHUNK);
    patch_index_kernel<<<dim3(nchunks, M), PB, 0, (hipStream_t)stream>>>(labels, V, nchunks, k, counts);
    CTU_CHECK_LAUNCH("patch_index");
    return CTU_OK;
}

extern "C" int ctu_patch_draw(const uint8_t* labels, const int32_t* counts, int M, int D, int H, int W, int K,
                              const int* classes, const int32_t* items, int P, int64_t* counter, uint64_t seed,
                              const int* patch, const int* jitter, const double* cum, int32_t* coords, int32_t* records,
                              void* stream) {
    CTU_REQUIRE(labels && counts && items && counter && patch && jitter && cum && coords && records, "patch_draw: null pointer");
    CTU_REQUIRE(M > 0 && M <= 65535 && grid_ok(D, H, W), "patch_draw: bad shape M=%d %dx%dx%d", M, D, H, W);
    CTU_REQUIRE(P > 0, "patch_draw: %d patches", P);
    DrawArgs a;
    if (int e = classes_of(K, classes, &a.k, "patch_draw")) return e;
    double prev = 0.0;
    for (int i = 0; i < KMAX; ++i) {
        a.cum[i] = i < K ? cum[i] : 0.0;
        if (i < K) {
            CTU_REQUIRE(cum[i] >= prev && cum[i] <= 1.0, "patch_draw: cumulative probabilities must rise within [0, 1]");
            prev = cum[i];
        }
    }
    a.n[0] = D; a.n[1] = H; a.n[2] = W;
    for (int ax = 0; ax < 3; ++ax) {
        CTU_REQUIRE(patch[ax] >= 1, "patch_draw: patch side %d", patch[ax]);
        CTU_REQUIRE(jitter[ax] >= 0 && jitter[ax] <= (patch[ax] - 1) / 2, "patch_draw: jitter %d outside [0, (%d - 1) / 2]",
                    jitter[ax], patch[ax]);
        a.p[ax] = patch[ax];
        a.jit[ax] = jitter[ax];
    }
    a.labels = labels; a.counts = counts; a.items = items; a.counter = counter;
    a.M = M; a.P = P;
    a.nchunks = (int)ceil_div64((int64_t)D * H * W, CTU_PATCH_CHUNK);
    CTU_REQUIRE(ceil_div(a.nchunks, PB) <= SEG, "patch_draw: %d chunks", a.nchunks);
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.coords = coords; a.records = records;
    patch_draw_kernel<<<P, PB, 0, (hipStream_t)stream>>>(a);
    CTU_CHECK_LAUNCH("patch_draw");
    patch_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(counter, P);
    CTU_CHECK_LAUNCH("patch_draw (counter)");
    return CTU_OK;
}

extern "C" int ctu_patch_crop(const void* src, int src_dtype, int Ms, int C, int D, int H, int W, const int32_t* coords,
                              int P, int pd, int ph, int pw, double fill, void* out, int out_dtype, int Ctot,
                              int out_channel, void* stream) {
    CTU_REQUIRE(src && coords && out, "patch_crop: null pointer");
    CTU_REQUIRE(Ms > 0 && C > 0 && D > 0 && H > 0 && W > 0, "patch_crop: bad source shape %dx%dx%dx%dx%d", Ms, C, D, H, W);
    CTU_REQUIRE(P > 0 && pd > 0 && ph > 0 && pw > 0 && (int64_t)pd * ph * pw < ((int64_t)1 << 31),
                "patch_crop: bad patch shape %dx%dx%dx%d", P, pd, ph, pw);
    CTU_REQUIRE(out_channel >= 0 && out_channel + C <= Ctot, "patch_crop: channels [%d, %d) of %d", out_channel,
                out_channel + C, Ctot);
    CTU_REQUIRE(out_dtype == src_dtype || out_dtype == CTU_F32, "patch_crop: the output is the source's dtype or float32");
    const bool whole = fill == (double)(int64_t)fill;
    CTU_REQUIRE(out_dtype != CTU_U8 || (whole && fill >= 0 && fill <= 255), "patch_crop: fill is not a uint8");
    CTU_REQUIRE(out_dtype != CTU_I16 || (whole && fill >= -32768 && fill <= 32767), "patch_crop: fill is not an int16");
    CTU_REQUIRE(out_dtype != CTU_F32 || (double)(float)fill == fill, "patch_crop: fill is not a float32");
    CropArgs a;
    a.src = src; a.coords = coords; a.out = out;
    a.items = (int64_t)P * C;
    a.Ms = Ms; a.C = C; a.D = D; a.H = H; a.W = W;
    a.pd = pd; a.ph = ph; a.pw = pw; a.Ctot = Ctot; a.oc = out_channel;
    a.ntx = a.nty = 0;
    a.fill = fill;
    hipStream_t st = (hipStream_t)stream;
    if (src_dtype == CTU_U8) return out_dtype == CTU_U8 ? launch_crop<uint8_t, uint8_t>(a, st) : launch_crop<uint8_t, float>(a, st);
    if (src_dtype == CTU_I16) return out_dtype == CTU_I16 ? launch_crop<int16_t, int16_t>(a, st) : launch_crop<int16_t, float>(a, st);
    CTU_REQUIRE(src_dtype == CTU_F32, "patch_crop: dtype %d (uint8, int16 or float32)", src_dtype);
    return launch_crop<float, float>(a, st);
}
