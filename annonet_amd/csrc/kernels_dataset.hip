// kernels_dataset.hip — what a training crop is drawn FROM, built on the device from the resident label image of a dataset entry
// (annonet_train_main.cpp:414-502 the two filters, annonet.cpp:41-58 + annonet_train_main.cpp:121-131 the labelled-point lists):
//
//   relabel   labels equal to one of up to 64 class values become ANH_LABEL_IGNORE (ignore_classes_to_ignore)
//   extent    area and bounding box of every blob of kernels_blobs.hip's blob map: integer atomics, summed per wave and per workgroup
//             (an LDS table keyed by blob number) before they touch global memory
//   ignore    every pixel of a blob that is too large by area, width or height becomes ANH_LABEL_IGNORE (ignore_large_nonzero_regions)
//   count     per block of 1024 pixels in raster order, the number of pixels of every class value below 64, class-major [64][blocks]
//   scan      one workgroup per class: the class's exclusive prefix over the blocks, in place, and its total
//   pick      one wave per pick: "the k-th pixel of class c in raster order" = binary search of c's block prefix, then a walk over the
//             block in 64-pixel steps by ballot / popcount; random_rect_containing_point around it, written into the crop's CropSource
//
// No labelled-point list exists anywhere: the index of an image is 4 bytes per present class and 1024 pixels.
#include <hip/hip_runtime.h>

#include <climits>

#include "blockscan.h"
#include "common.h"
#include "kernels.h"

namespace anh {
namespace {

constexpr int kIndexPixels = kDatasetIndexPixels;   // pixels per block of the index (256 threads x 4)
constexpr int kExtentPixels = 4096;                 // pixels per block of the extent launch (256 threads x 16)
constexpr int kExtentSlots = 128;                   // its LDS table
constexpr uint16_t kIgnore = ANH_LABEL_IGNORE;

// the sum of `mine` over the wave goes to *counter by one atomic of lane 0 (none when the sum is 0)
__device__ __forceinline__ void wave_add(unsigned mine, unsigned long long* counter) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += (unsigned)__shfl_xor((int)mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counter, (unsigned long long)mine);
}

__global__ __launch_bounds__(256) void dataset_relabel_kernel(uint16_t* labels, int64_t pixels, DatasetIgnoreList list, unsigned long long* changed) {
    const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + j * 256;
        if (p >= pixels) break;
        const uint16_t l = labels[p];
        bool hit = false;
        for (int i = 0; i < list.n; ++i) hit |= l == list.values[i];
        if (hit && l != kIgnore) { labels[p] = kIgnore; ++mine; }
    }
    wave_add(mine, changed);
}

struct ExtentSlots {
    unsigned key[kExtentSlots], area[kExtentSlots];
    int left[kExtentSlots], top[kExtentSlots], right[kExtentSlots], bottom[kExtentSlots];
};

__device__ __forceinline__ void extent_to_global(anh_region* table, unsigned b, unsigned area, int left, int top, int right, int bottom) {
    anh_region* row = table + (b - 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->area), (unsigned long long)area);
    atomicMin(&row->left, left);
    atomicMin(&row->top, top);
    atomicMax(&row->right, right);
    atomicMax(&row->bottom, bottom);
}

__device__ __forceinline__ void extent_to_lds(ExtentSlots& s, anh_region* table, unsigned b, unsigned area, int left, int top, int right, int bottom) {
    unsigned slot = (b * 2654435761u) >> 25;   // 7 bits
#pragma unroll 1
    for (int probe = 0; probe < 8; ++probe, slot = (slot + 1) & (kExtentSlots - 1)) {
        const unsigned k = atomicCAS(&s.key[slot], 0u, b);
        if (k != 0 && k != b) continue;
        atomicAdd(&s.area[slot], area);
        atomicMin(&s.left[slot], left);
        atomicMin(&s.top[slot], top);
        atomicMax(&s.right[slot], right);
        atomicMax(&s.bottom[slot], bottom);
        return;
    }
    extent_to_global(table, b, area, left, top, right, bottom);   // a crowded table: more blobs in this block than it holds
}

// the rows come initialised from blob_number_kernel (area 0, an empty box)
__global__ __launch_bounds__(256) void dataset_extent_kernel(const uint32_t* blobs, anh_region* table, int64_t pixels, int w) {
    __shared__ ExtentSlots s;
    for (int i = threadIdx.x; i < kExtentSlots; i += 256) {
        s.key[i] = 0; s.area[i] = 0;
        s.left[i] = INT_MAX; s.top[i] = INT_MAX; s.right[i] = -1; s.bottom[i] = -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * kExtentPixels;
#pragma unroll 1
    for (int it = 0; it < kExtentPixels / 256; ++it) {
        const int64_t p = base + it * 256 + threadIdx.x;
        unsigned b = 0;
        int x = 0, y = 0;
        if (p < pixels) b = blobs[p];
        if (b) { y = (int)(p / w); x = (int)(p - (int64_t)y * w); }
        const unsigned long long active = __ballot(b != 0);
        if (active == 0) continue;
        const int first = __ffsll((long long)active) - 1;
        const unsigned b0 = (unsigned)__shfl((int)b, first, 64);
        if (__ballot(b != 0 && b != b0) == 0) {   // one blob in the whole wave (the inside of a large region): ONE lane carries the wave's sums
            int left = b ? x : INT_MAX, top = b ? y : INT_MAX, right = b ? x : -1, bottom = b ? y : -1;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                left = min(left, __shfl_xor(left, d, 64));
                top = min(top, __shfl_xor(top, d, 64));
                right = max(right, __shfl_xor(right, d, 64));
                bottom = max(bottom, __shfl_xor(bottom, d, 64));
            }
            if (lane == first) extent_to_lds(s, table, b0, (unsigned)__popcll(active), left, top, right, bottom);
        } else if (b)
            extent_to_lds(s, table, b, 1u, x, y, x, y);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kExtentSlots; i += 256)
        if (s.key[i]) extent_to_global(table, s.key[i], s.area[i], s.left[i], s.top[i], s.right[i], s.bottom[i]);
}

// the three tests of hostlogic.cpp: ignore_large_nonzero_regions, strict, in double; an infinite limit never fires
__global__ __launch_bounds__(256) void dataset_ignore_large_kernel(uint16_t* labels, const uint32_t* blobs, const anh_region* table, int64_t pixels, double max_points,
                                                                   double max_width, double max_height, unsigned long long* changed) {
    const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + j * 256;
        if (p >= pixels) break;
        const uint32_t b = blobs[p];
        if (b == 0) continue;
        const anh_region* row = table + (b - 1);
        const bool too_large = (double)row->area > max_points || (double)(row->right - row->left + 1) > max_width || (double)(row->bottom - row->top + 1) > max_height;
        if (!too_large) continue;
        if (labels[p] != kIgnore) { labels[p] = kIgnore; ++mine; }   // a blob of the ignore label stays what it is and is not counted
    }
    wave_add(mine, changed);
}

// counts[c][block] = pixels of class c < 64 among the block's 1024; any other label but the ignore label raises *bad
__global__ __launch_bounds__(256) void dataset_count_kernel(const uint16_t* labels, int64_t pixels, unsigned blocks, unsigned* counts, int* bad) {
    __shared__ unsigned hist[kCropMaxClasses];
    if (threadIdx.x < kCropMaxClasses) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kIndexPixels + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + j * 256;
        if (p >= pixels) break;
        const uint16_t l = labels[p];
        if (l < kCropMaxClasses) atomicAdd(&hist[l], 1u);
        else if (l != kIgnore) *bad = 1;
    }
    __syncthreads();
    if (threadIdx.x < kCropMaxClasses) counts[(size_t)threadIdx.x * blocks + blockIdx.x] = hist[threadIdx.x];
}

// one workgroup per class; an image may have more than 1024 blocks, so the scan walks the row in strides of 1024 with a carry
__global__ __launch_bounds__(1024) void dataset_scan_kernel(unsigned* counts, int blocks, unsigned long long* totals) {
    __shared__ unsigned wave_sums[16];
    counts += (size_t)blockIdx.x * blocks;
    unsigned carry = 0;
    for (int base = 0; base < blocks; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < blocks ? counts[i] : 0u;
        unsigned total;
        const unsigned before = block_exclusive_scan<1024>(v, wave_sums, &total);
        if (i < blocks) counts[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void dataset_pick_kernel(const DatasetPickJob* jobs, int n, CropSource* specs, DatasetPick* picks, int* failed) {
    const int pick = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pick >= n) return;
    const DatasetPickJob job = jobs[pick];
    int lo = 0, hi = job.blocks - 1;   // the last block whose prefix is <= k holds the k-th pixel
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (job.prefix[mid] <= job.k) lo = mid;
        else hi = mid - 1;
    }
    unsigned rest = job.k - job.prefix[lo];
    int64_t found = -1;
#pragma unroll 1
    for (int step = 0; step < kIndexPixels / 64; ++step) {
        const int64_t p = (int64_t)lo * kIndexPixels + step * 64 + lane;
        const bool match = p < job.pixels && job.labels[p] == job.label;
        const unsigned long long mask = __ballot(match);
        const unsigned here = (unsigned)__popcll(mask);
        if (rest < here) {
            const bool mine = match && (unsigned)__popcll(mask & ((1ull << lane) - 1ull)) == rest;
            const unsigned long long winner = __ballot(mine);
            found = (int64_t)lo * kIndexPixels + step * 64 + (__ffsll((long long)winner) - 1);
            break;
        }
        rest -= here;
    }
    if (lane != 0) return;
    DatasetPick out{0, 0, 0, 0};
    if (found < 0) *failed = 1;   // the index does not describe these labels
    else {
        out.y = (int)(found / job.width); out.x = (int)(found - (int64_t)out.y * job.width);
        // random_rect_containing_point (hostlogic.cpp) for a square of side src_dim: the centre is drawn from src_dim positions
        const long long side = job.src_dim;
        const long long cx = out.x - (side - 1) / 2 + (long long)(job.draw_x % (unsigned)job.src_dim);
        const long long cy = out.y - (side - 1) / 2 + (long long)(job.draw_y % (unsigned)job.src_dim);
        out.left = (int)(cx - side / 2); out.top = (int)(cy - side / 2);
    }
    specs[pick].left = out.left; specs[pick].top = out.top;
    picks[pick] = out;
}

unsigned blocks_of(int64_t pixels, int per_block) { return (unsigned)((pixels + per_block - 1) / per_block); }

}  // namespace

size_t dataset_index_blocks(int64_t pixels) { return (size_t)blocks_of(pixels, kIndexPixels); }

void launch_dataset_relabel(uint16_t* d_labels, int64_t pixels, const DatasetIgnoreList& list, unsigned long long* d_changed, hipStream_t s) {
    hipLaunchKernelGGL(dataset_relabel_kernel, dim3(blocks_of(pixels, 1024)), dim3(256), 0, s, d_labels, pixels, list, d_changed);
    HIP_CHECK(hipGetLastError());
}

void launch_dataset_ignore_large(uint16_t* d_labels, const uint32_t* d_blobs, anh_region* d_table, uint32_t rows, int h, int w, double max_points, double max_width,
                                 double max_height, unsigned long long* d_changed, hipStream_t s) {
    if (rows == 0) return;
    const int64_t pixels = (int64_t)h * w;
    hipLaunchKernelGGL(dataset_extent_kernel, dim3(blocks_of(pixels, kExtentPixels)), dim3(256), 0, s, d_blobs, d_table, pixels, w);
    hipLaunchKernelGGL(dataset_ignore_large_kernel, dim3(blocks_of(pixels, 1024)), dim3(256), 0, s, d_labels, d_blobs, d_table, pixels, max_points, max_width, max_height,
                       d_changed);
    HIP_CHECK(hipGetLastError());
}

void launch_dataset_index(const uint16_t* d_labels, int64_t pixels, unsigned* d_counts, unsigned long long* d_totals, int* d_bad, hipStream_t s) {
    const unsigned blocks = blocks_of(pixels, kIndexPixels);
    hipLaunchKernelGGL(dataset_count_kernel, dim3(blocks), dim3(256), 0, s, d_labels, pixels, blocks, d_counts, d_bad);
    hipLaunchKernelGGL(dataset_scan_kernel, dim3(kCropMaxClasses), dim3(1024), 0, s, d_counts, (int)blocks, d_totals);
    HIP_CHECK(hipGetLastError());
}

void launch_dataset_pick(const DatasetPickJob* d_jobs, int n, CropSource* d_specs, DatasetPick* d_picks, int* d_failed, hipStream_t s) {
    hipLaunchKernelGGL(dataset_pick_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, d_jobs, n, d_specs, d_picks, d_failed);
    HIP_CHECK(hipGetLastError());
}

}  // namespace anh
