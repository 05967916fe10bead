// Exclusive scans in a fixed order, shared by the kernels that number things: the block-wide scan (components.hip: roots per
// chunk; mesh.hip: vertices and faces per cell row; mesh_distance.hip: faces per cell) and, on top of it, the chunked scan
// of a whole device array in three launches (mesh_smooth.hip: adjacency cursors and offsets; mesh_decimate.hip: occupied
// cells, face buckets, used clusters, surviving faces).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

// Exclusive prefix of x over the block's threads in thread order, `total` = the block's sum.  `lds` holds one T per wave
// (blockDim.x / 64 entries) and fixes the type of the sums; every thread of the block must call it (two barriers).
template <class T, class X>
__device__ __forceinline__ T block_exclusive_scan(X x_, T* lds, T& total) {
    const T x = (T)x_;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T s = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(s, o);
        if (lane >= o) s += y;
    }
    if (lane == 63) lds[wid] = s;
    __syncthreads();
    T wo = 0;
    total = 0;
    for (int i = 0; i < nw; ++i) {
        if (i < wid) wo += lds[i];
        total += lds[i];
    }
    __syncthreads();
    return wo + s - x;
}

// ---- chunked scan: y[i] = x[0] + ... + x[i-1] over n items of int32 or uint8, in three launches: the sum of every chunk of
// CSCAN_CHUNK = 1024 threads x 4 items, one block that scans the chunk sums in order (a thread owns ceil(chunks / 1024)
// consecutive chunks beyond 1024 chunks; int64), and the chunks again with their bases.  x is a 256-byte aligned array.
constexpr int CSCAN_BLOCK = 1024;
constexpr int CSCAN_ITEMS = 4;
constexpr int CSCAN_CHUNK = CSCAN_BLOCK * CSCAN_ITEMS;

__device__ __forceinline__ void cscan_load(const int* __restrict__ x, int64_t i0, int64_t n, int (&w)[CSCAN_ITEMS]) {
    if (i0 + CSCAN_ITEMS <= n) {
        const int4 q = *reinterpret_cast<const int4*>(x + i0);     // i0 % 4 == 0
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
        for (int u = 0; u < CSCAN_ITEMS; ++u) w[u] = i0 + u < n ? x[i0 + u] : 0;
    }
}
__device__ __forceinline__ void cscan_load(const uint8_t* __restrict__ x, int64_t i0, int64_t n, int (&w)[CSCAN_ITEMS]) {
    if (i0 + CSCAN_ITEMS <= n) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(x + i0);
        w[0] = q & 255u; w[1] = (q >> 8) & 255u; w[2] = (q >> 16) & 255u; w[3] = q >> 24;
    } else {
#pragma unroll
        for (int u = 0; u < CSCAN_ITEMS; ++u) w[u] = i0 + u < n ? x[i0 + u] : 0;
    }
}

template <class X>
__global__ void __launch_bounds__(CSCAN_BLOCK) cscan_sums_kernel(const X* __restrict__ x, int64_t n, long long* __restrict__ bsum) {
    __shared__ long long lds[CSCAN_BLOCK / 64];
    int w[CSCAN_ITEMS];
    cscan_load(x, (int64_t)blockIdx.x * CSCAN_CHUNK + (int64_t)threadIdx.x * CSCAN_ITEMS, n, w);
    long long total;
    block_exclusive_scan((long long)w[0] + w[1] + w[2] + w[3], lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// exclusive scan of the chunk sums in place; the total goes to *total and, as an int32, to *end if given
static __global__ void __launch_bounds__(CSCAN_BLOCK) cscan_chunks_kernel(long long* __restrict__ bsum, int nb, long long* total,
                                                                          int* end) {
    __shared__ long long lds[CSCAN_BLOCK / 64];
    const int per = (nb + CSCAN_BLOCK - 1) / CSCAN_BLOCK;
    const int r0 = min((int)threadIdx.x * per, nb), r1 = min(r0 + per, nb);
    long long s = 0;
    for (int r = r0; r < r1; ++r) s += bsum[r];
    long long t;
    long long o = block_exclusive_scan(s, lds, t);
    for (int r = r0; r < r1; ++r) {
        const long long b = bsum[r];
        bsum[r] = o;
        o += b;
    }
    if (threadIdx.x == 0) {
        *total = t;
        if (end) *end = (int)t;                                    // the caller keeps the total below 2^31
    }
}

template <class X>
__global__ void __launch_bounds__(CSCAN_BLOCK) cscan_apply_kernel(const X* __restrict__ x, int64_t n, const long long* __restrict__ bsum,
                                                                  int* __restrict__ y) {
    __shared__ long long lds[CSCAN_BLOCK / 64];
    int w[CSCAN_ITEMS];
    const int64_t i0 = (int64_t)blockIdx.x * CSCAN_CHUNK + (int64_t)threadIdx.x * CSCAN_ITEMS;
    cscan_load(x, i0, n, w);
    long long total;
    long long o = bsum[blockIdx.x] + block_exclusive_scan((long long)w[0] + w[1] + w[2] + w[3], lds, total);
#pragma unroll
    for (int u = 0; u < CSCAN_ITEMS; ++u) {
        if (i0 + u < n) y[i0 + u] = (int)o;
        o += w[u];
    }
}

// n >= 1 items, n <= 2^31; bsum: ceil(n / CSCAN_CHUNK) int64; y may not alias x.  `what` names the caller in a launch error.
template <class X>
int chunked_exclusive_scan(const X* x, int64_t n, long long* bsum, int* y, long long* total, int* end, hipStream_t st,
                           const char* what) {
    const int nb = (int)ceil_div64(n, CSCAN_CHUNK);
    cscan_sums_kernel<X><<<nb, CSCAN_BLOCK, 0, st>>>(x, n, bsum);
    CTU_CHECK_LAUNCH(what);
    cscan_chunks_kernel<<<1, CSCAN_BLOCK, 0, st>>>(bsum, nb, total, end);
    CTU_CHECK_LAUNCH(what);
    cscan_apply_kernel<X><<<nb, CSCAN_BLOCK, 0, st>>>(x, n, bsum, y);
    CTU_CHECK_LAUNCH(what);
    return CTU_OK;
}
