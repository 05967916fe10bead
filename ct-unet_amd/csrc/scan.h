// Block-wide exclusive scan in a fixed order, shared by the kernels that number things in C order (components.hip: roots
// per chunk; mesh.hip: vertices and faces per cell row).
#pragma once
#include <hip/hip_runtime.h>

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
