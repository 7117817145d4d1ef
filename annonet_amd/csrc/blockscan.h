// blockscan.h — the workgroup-wide prefix sum of the kernels that rank things in raster order (kernels_blobs.hip, kernels_dataset.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace anh {

// block-wide exclusive prefix sum over THREADS values; *total = their sum.  Every thread of the block calls it.
// wave_sums: THREADS / 64 words of LDS.
template <int THREADS>
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* wave_sums, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(x, d, 64);
        if (lane >= d) x += up;
    }
    __syncthreads();   // a previous call's readers are done with wave_sums
    if (lane == 63) wave_sums[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) {
        const unsigned s = wave_sums[i];
        if (i < wave) before += s;
        all += s;
    }
    *total = all;
    return before + x - v;
}

}  // namespace anh
