// kernels_blobs.hip — connected blobs of a u16 label map on the device (annonet_infer.cpp:194-223: connected_blobs, detection_seeds):
// block-based union-find labelling, dlib's numbering, and a per-blob region table.
//
// A blob = an 8-connected set of pixels of EQUAL non-zero label; blobs are numbered 1, 2, ... in raster order of their first pixel
// (annonet_host.h: label_connected_blobs restates that numbering [UPSTREAM-UNVERIFIED]).
//
//   local    one workgroup per 32 x 32 tile: union-find in LDS; parent[p] = smallest linear index of p's in-tile component (-1: background)
//   seam     pixels on tile borders unite with their neighbours in adjacent tiles (the diagonal across a tile corner included).  A union
//            hangs the larger root under the smaller with an agent-scope atomic min, and every read of parent[] in that launch is an
//            agent-scope atomic load (a plain load may be served from a stale line of another XCD's L2).  Parents only ever decrease,
//            so every walk to a root ends.
//   flatten  every pixel walks to its root = the blob's minimum linear index = its first pixel in raster order; roots per 1024 pixels counted
//   scan     exclusive prefix sum of those counts by ONE workgroup, then every block ranks its own roots: plain launches, no workgroup
//            ever waits for another one of its launch — coherence comes from the kernel boundaries and the atomics above
//   number   blob[p] = rank(root(p)) + 1; the root's thread initialises the blob's table row
//   stats    area, bounding box, seed count, peak margin: integer atomics only (order-independent, bitwise reproducible), summed per
//            wave and per workgroup (an LDS table keyed by blob number) before they touch global memory
//
// Every step works on a stack of n maps of one size, [n][h][w], with a number of launches that does not depend on n; one map is a stack
// with n = 1.  The grid of every step covers n times the blocks of one map and no block straddles two images; parents, roots and blob
// numbers stay plane-local (the numbers restart at 1 in every image, the scan has one workgroup per image); image i's table rows begin
// at row_offsets[i], which the host sums from the counts.
#include <hip/hip_runtime.h>

#include <climits>

#include "blockscan.h"
#include "common.h"
#include "kernels.h"

namespace anh {
namespace {

constexpr int T = kBlobTile;
constexpr int kScanPixels = 1024;    // pixels per block of the flatten / rank launches (256 threads x 4)
constexpr int kStatPixels = 4096;    // pixels per block of the statistics launch (256 threads x 16)
constexpr int kStatSlots = 128;      // LDS table of the statistics launch
constexpr unsigned kPeakNone = 0x007FFFFFu;   // ordered_bits(-inf)

static_assert(sizeof(anh_region) == 56, "the table rows are written as 14 words");

// float -> unsigned whose order is the float order (-inf lowest); NaN never enters (callers test for it)
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

// ---- union-find in LDS (one tile) ----
__device__ __forceinline__ int lds_find(int* par, int a) {
    for (;;) {
        const int pa = __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (pa == a) return a;
        a = pa;
    }
}
__device__ __forceinline__ void lds_unite(int* par, int a, int b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // the larger root under the smaller
        if (old == a) return;
        a = old;   // a was no root any more: its parent (now min(old, b)) and b still have to meet
    }
}

// ---- union-find in global memory (the seams) ----
__device__ __forceinline__ int agent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int global_find(int* parent, int a) {
    const int start = a;
    int pa = agent_load(parent + a);
    if (pa == a) return a;
    for (;;) {
        a = pa;
        pa = agent_load(parent + a);
        if (pa == a) break;
    }
    __hip_atomic_fetch_min(parent + start, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // shorten the chain: a root is never above any ancestor
    return a;
}
__device__ __forceinline__ void global_unite(int* parent, int a, int b) {
    for (;;) {
        a = global_find(parent, a);
        b = global_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// Every kernel below cuts blockIdx.x ONCE into (image, block within the image) and moves its pointers to that image's plane; the addresses
// add image * plane in 64 bits.  Everything computed after that is plane-local (parent values are linear indices within the plane), so an
// image gets the same bits whatever stack it lies in, a stack of one included.  The grid of the two tile kernels covers n x tiles.
__global__ __launch_bounds__(256) void blob_local_kernel(const uint16_t* labels, int* parent, int h, int w, int tiles_x, unsigned tiles) {
    __shared__ uint16_t lab[T + 1][T + 2];   // a frame of zeros above, left and right: label 0 never joins a blob
    __shared__ int par[T * T];
    const unsigned image = blockIdx.x / tiles, tile = blockIdx.x - image * tiles;
    const size_t at = (size_t)image * ((size_t)h * w);
    labels += at; parent += at;
    const int tile_y = (int)(tile / (unsigned)tiles_x), tile_x = (int)(tile - (unsigned)tile_y * (unsigned)tiles_x);
    const int x0 = tile_x * T, y0 = tile_y * T;
    for (int i = threadIdx.x; i < (T + 1) * (T + 2); i += 256) (&lab[0][0])[i] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = threadIdx.x + 256 * q, ly = i / T, lx = i - ly * T, y = y0 + ly, x = x0 + lx;
        lab[ly + 1][lx + 1] = (y < h && x < w) ? labels[(size_t)y * w + x] : (uint16_t)0;
        par[i] = i;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = threadIdx.x + 256 * q, ly = i / T, lx = i - ly * T;
        const uint16_t l = lab[ly + 1][lx + 1];
        if (l == 0) continue;
        // the four neighbours that come earlier in raster order; a matching N already ties W, NW and NE to it through their own tests
        if (lab[ly][lx + 1] == l) lds_unite(par, i, i - T);
        else {
            if (lab[ly + 1][lx] == l) lds_unite(par, i, i - 1);
            else if (lab[ly][lx] == l) lds_unite(par, i, i - T - 1);
            if (lab[ly][lx + 2] == l) lds_unite(par, i, i - T + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = threadIdx.x + 256 * q, ly = i / T, lx = i - ly * T, y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        int out = -1;
        if (lab[ly + 1][lx + 1] != 0) {
            const int r = lds_find(par, i), ry = r / T, rx = r - ry * T;   // raster order inside the tile = raster order of the map
            out = (y0 + ry) * w + (x0 + rx);
        }
        parent[(size_t)y * w + x] = out;
    }
}

// Neighbours are tested against the sides of the plane (nx, ny), never through the linear index: a seam neither wraps from a row's last
// column to the next row's first nor, in a stack, runs from the last row of one image into the first row of the next.
__global__ __launch_bounds__(128) void blob_seam_kernel(const uint16_t* labels, int* parent, int h, int w, int tiles_x, unsigned tiles) {
    const unsigned image = blockIdx.x / tiles, tile = blockIdx.x - image * tiles;
    const size_t at = (size_t)image * ((size_t)h * w);
    labels += at; parent += at;
    const int tile_y = (int)(tile / (unsigned)tiles_x), tile_x = (int)(tile - (unsigned)tile_y * (unsigned)tiles_x);
    const int t = threadIdx.x;
    int ly, lx;
    if (t < T) { ly = 0; lx = t; }                                 // top row
    else if (t < 2 * T - 1) { ly = t - T + 1; lx = 0; }            // left column below it
    else if (t < 3 * T - 2) { ly = t - (2 * T - 1) + 1; lx = T - 1; }   // right column below it
    else return;
    const int y = tile_y * T + ly, x = tile_x * T + lx;
    if (y >= h || x >= w) return;
    const uint16_t l = labels[(size_t)y * w + x];
    if (l == 0) return;
    const int p = y * w + x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // W, NW, N, NE: every adjacent pair of the map is seen from its later pixel
        const int nx = x + (k == 3 ? 1 : k == 2 ? 0 : -1), ny = y - (k == 0 ? 0 : 1);
        if (nx < 0 || nx >= w || ny < 0) continue;
        if (nx / T == tile_x && ny / T == tile_y) continue;   // the local pass has joined these
        if (labels[(size_t)ny * w + nx] == l) global_unite(parent, p, ny * w + nx);
    }
}

// roots[p] = root(p) + 1 (0: background); sums[block] = number of roots among the block's 1024 pixels.
// `per_image` = ceil(pixels / 1024) blocks per image: no block straddles two images; sums is [n][per_image]
__global__ __launch_bounds__(256) void blob_flatten_kernel(const int* parent, uint32_t* roots, unsigned* sums, int64_t pixels, unsigned per_image) {
    __shared__ unsigned wave_sums[4];
    const unsigned image = blockIdx.x / per_image, block = blockIdx.x - image * per_image;
    const size_t at = (size_t)image * (size_t)pixels;
    parent += at; roots += at; sums += (size_t)image * per_image;
    const int64_t base = (int64_t)block * kScanPixels + threadIdx.x * 4;
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + j;
        if (p >= pixels) break;
        int a = parent[p];
        if (a < 0) { roots[p] = 0; continue; }
        if (a == (int)p) ++mine;
        for (int pa = parent[a]; pa != a; pa = parent[a]) a = pa;
        roots[p] = (uint32_t)a + 1u;
    }
    unsigned total;
    (void)block_exclusive_scan<256>(mine, wave_sums, &total);
    if (threadIdx.x == 0) sums[block] = total;
}

// one workgroup per image, so the prefix sum restarts at every image: sums[image][i] -> sum of sums[image][0 .. i);
// counts[image] = the image's total + 1 ("labels including the background one")
__global__ __launch_bounds__(1024) void blob_scan_sums_kernel(unsigned* sums, int per_image, unsigned* counts) {
    __shared__ unsigned wave_sums[16];
    sums += (size_t)blockIdx.x * per_image;
    unsigned carry = 0;
    for (int base = 0; base < per_image; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < per_image ? sums[i] : 0u;
        unsigned total;
        const unsigned before = block_exclusive_scan<1024>(v, wave_sums, &total);
        if (i < per_image) sums[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry + 1u;
}

// every root's slot of parent[] receives the blob's number: 1 + the number of roots before it in raster order OF ITS IMAGE
__global__ __launch_bounds__(256) void blob_rank_kernel(int* parent, const unsigned* sums, int64_t pixels, unsigned per_image) {
    __shared__ unsigned wave_sums[4];
    const unsigned image = blockIdx.x / per_image, block = blockIdx.x - image * per_image;
    parent += (size_t)image * (size_t)pixels; sums += (size_t)image * per_image;
    const int64_t base = (int64_t)block * kScanPixels + threadIdx.x * 4;
    bool root[4];
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + j;
        root[j] = p < pixels && parent[p] == (int)p;
        mine += root[j] ? 1u : 0u;
    }
    unsigned total;
    unsigned number = sums[block] + block_exclusive_scan<256>(mine, wave_sums, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (root[j]) parent[base + j] = (int)++number;
}

// blobs[p]: root(p) + 1 -> the blob's number.  table != nullptr: the root's thread writes the blob's row (14 words, padding included).
// row_offsets[image] = the number of rows of the images before it: image i's rows begin there (table == nullptr: never read)
__global__ __launch_bounds__(256) void blob_number_kernel(const int* numbers, uint32_t* blobs, const uint16_t* labels, anh_region* table,
                                                          const unsigned long long* row_offsets, int64_t pixels, int w, unsigned per_image) {
    const unsigned image = blockIdx.x / per_image, block = blockIdx.x - image * per_image;
    const size_t at = (size_t)image * (size_t)pixels;
    numbers += at; blobs += at; labels += at;
    if (table) table += row_offsets[image];
    const int64_t p = (int64_t)block * 256 + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t r = blobs[p];
    if (r == 0) return;
    const uint32_t b = (uint32_t)numbers[r - 1];
    blobs[p] = b;
    if (table && (int64_t)(r - 1) == p) {
        uint32_t* row = reinterpret_cast<uint32_t*>(table + (b - 1));
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        row[0] = b;
        row[1] = (uint32_t)labels[p];   // label, detected = 0
        row[2] = (uint32_t)INT_MAX; row[3] = (uint32_t)INT_MAX; row[4] = (uint32_t)-1; row[5] = (uint32_t)-1;   // left, top, right, bottom
        row[6] = (uint32_t)y; row[7] = (uint32_t)x;
        row[8] = row[9] = row[10] = row[11] = 0;   // area, seeds
        row[12] = kPeakNone;
        row[13] = 0;
    }
}

struct StatSlots {
    unsigned key[kStatSlots];
    unsigned area[kStatSlots], seeds[kStatSlots], peak[kStatSlots];
    int left[kStatSlots], top[kStatSlots], right[kStatSlots], bottom[kStatSlots];
};

__device__ __forceinline__ void stat_to_global(anh_region* table, unsigned b, unsigned area, unsigned seeds, int left, int top, int right, int bottom, unsigned peak) {
    anh_region* row = table + (b - 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&row->area), (unsigned long long)area);
    if (seeds) atomicAdd(reinterpret_cast<unsigned long long*>(&row->seeds), (unsigned long long)seeds);
    atomicMin(&row->left, left);
    atomicMin(&row->top, top);
    atomicMax(&row->right, right);
    atomicMax(&row->bottom, bottom);
    if (peak > kPeakNone) atomicMax(reinterpret_cast<unsigned*>(&row->peak), peak);
}

__device__ __forceinline__ void stat_to_lds(StatSlots& s, anh_region* table, unsigned b, unsigned area, unsigned seeds, int left, int top, int right, int bottom, unsigned peak) {
    unsigned slot = (b * 2654435761u) >> 25;   // 7 bits
#pragma unroll 1
    for (int probe = 0; probe < 8; ++probe, slot = (slot + 1) & (kStatSlots - 1)) {
        const unsigned k = atomicCAS(&s.key[slot], 0u, b);
        if (k != 0 && k != b) continue;
        atomicAdd(&s.area[slot], area);
        if (seeds) atomicAdd(&s.seeds[slot], seeds);
        atomicMin(&s.left[slot], left);
        atomicMin(&s.top[slot], top);
        atomicMax(&s.right[slot], right);
        atomicMax(&s.bottom[slot], bottom);
        atomicMax(&s.peak[slot], peak);
        return;
    }
    stat_to_global(table, b, area, seeds, left, top, right, bottom, peak);   // a crowded table: more blobs in this block than it holds
}

// the margin is computed in float exactly as det_seed_kernel computes `mine - clean`.
// ceil(pixels / 4096) blocks per image, so a workgroup's LDS table is keyed by the blob numbers of ONE image; blended is [n][k][h][w]
__global__ __launch_bounds__(256) void blob_stats_kernel(const uint32_t* blobs, const uint16_t* labels, const float* blended, int k, const uint8_t* flags,
                                                         anh_region* table, const unsigned long long* row_offsets, int64_t pixels, int w, unsigned per_image) {
    __shared__ StatSlots s;
    const unsigned image = blockIdx.x / per_image, block = blockIdx.x - image * per_image;
    const size_t at = (size_t)image * (size_t)pixels;
    blobs += at; labels += at; blended += at * (size_t)k; flags += at; table += row_offsets[image];
    for (int i = threadIdx.x; i < kStatSlots; i += 256) {
        s.key[i] = 0; s.area[i] = 0; s.seeds[i] = 0; s.peak[i] = 0;
        s.left[i] = INT_MAX; s.top[i] = INT_MAX; s.right[i] = -1; s.bottom[i] = -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)block * kStatPixels;
#pragma unroll 1
    for (int it = 0; it < kStatPixels / 256; ++it) {
        const int64_t p = base + it * 256 + threadIdx.x;
        unsigned b = 0, seed = 0, peak = 0;
        int x = 0, y = 0;
        if (p < pixels) b = blobs[p];
        if (b) {
            y = (int)(p / w); x = (int)(p - (int64_t)y * w);
            seed = flags[p] ? 1u : 0u;
            const uint16_t lab = labels[p];
            if (lab < k) {
                const float clean = blended[p], mine = blended[(size_t)lab * pixels + p];
                const float margin = mine - clean;
                if (margin == margin) peak = ordered_bits(margin);   // NaN never wins
            }
        }
        const unsigned long long active = __ballot(b != 0);
        if (active == 0) continue;
        const int first = __ffsll((long long)active) - 1;
        const unsigned b0 = (unsigned)__shfl((int)b, first, 64);
        if (__ballot(b != 0 && b != b0) == 0) {   // one blob in the whole wave (the inside of a large region): ONE lane carries the wave's sums
            const unsigned area = (unsigned)__popcll(active), seeds = (unsigned)__popcll(__ballot(seed != 0));
            int left = b ? x : INT_MAX, top = b ? y : INT_MAX, right = b ? x : -1, bottom = b ? y : -1;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                left = min(left, __shfl_xor(left, d, 64));
                top = min(top, __shfl_xor(top, d, 64));
                right = max(right, __shfl_xor(right, d, 64));
                bottom = max(bottom, __shfl_xor(bottom, d, 64));
                peak = max(peak, (unsigned)__shfl_xor((int)peak, d, 64));
            }
            if (lane == first) stat_to_lds(s, table, b0, area, seeds, left, top, right, bottom, peak);
        } else if (b)
            stat_to_lds(s, table, b, 1u, seed, x, y, x, y, peak);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kStatSlots; i += 256)
        if (s.key[i]) stat_to_global(table, s.key[i], s.area[i], s.seeds[i], s.left[i], s.top[i], s.right[i], s.bottom[i], s.peak[i]);
}

__global__ __launch_bounds__(256) void blob_finish_kernel(anh_region* table, uint32_t n, int filtering) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    anh_region* row = table + i;
    row->peak = from_ordered_bits(*reinterpret_cast<const unsigned*>(&row->peak));
    row->detected = (uint16_t)((!filtering || row->seeds > 0) ? 1 : 0);
}

__global__ __launch_bounds__(256) void blob_filter_kernel(uint16_t* labels, const uint32_t* blobs, const anh_region* table, const unsigned long long* row_offsets,
                                                          int64_t pixels, unsigned per_image) {
    const unsigned image = blockIdx.x / per_image;
    const int64_t p = (int64_t)(blockIdx.x - image * per_image) * 256 + threadIdx.x;
    if (p >= pixels) return;
    const size_t at = (size_t)image * (size_t)pixels + (size_t)p;
    const uint32_t b = blobs[at];
    if (b != 0 && table[row_offsets[image] + (b - 1)].seeds == 0) labels[at] = 0;
}

unsigned blocks_of(int64_t pixels, int per_block) { return (unsigned)((pixels + per_block - 1) / per_block); }

}  // namespace

size_t blob_scan_blocks(int64_t pixels) { return (size_t)blocks_of(pixels, kScanPixels); }

// The limit of one labelling: h * w < 2^31 for every plane, and for a stack of two or more maps the tile-padded n * h * w < 2^32 as well.
// (For n = 1 the first alone holds, and every grid below is the grid of that one map.)
bool blob_batch_fits(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return false;
    const int64_t tiles = (int64_t)((w + T - 1) / T) * ((h + T - 1) / T);
    return (int64_t)n * tiles * (T * T) < ((int64_t)1 << 32);   // the widest launch has one thread per pixel of the tile-padded stack
}
bool blob_stack_fits(int n, int h, int w) { return n == 1 ? h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31) : blob_batch_fits(n, h, w); }

void launch_blob_label(const uint16_t* d_labels, int n, int h, int w, int* d_parent, uint32_t* d_blobs, unsigned* d_sums, unsigned* d_counts, hipStream_t s) {
    ANH_REQUIRE(blob_stack_fits(n, h, w), "blob labelling of a stack: too many pixels for one launch");
    const int64_t pixels = (int64_t)h * w;
    const int tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
    const unsigned tiles = (unsigned)((int64_t)tiles_x * tiles_y), blocks = blocks_of(pixels, kScanPixels);
    hipLaunchKernelGGL(blob_local_kernel, dim3(tiles * (unsigned)n), dim3(256), 0, s, d_labels, d_parent, h, w, tiles_x, tiles);
    if (tiles > 1) hipLaunchKernelGGL(blob_seam_kernel, dim3(tiles * (unsigned)n), dim3(128), 0, s, d_labels, d_parent, h, w, tiles_x, tiles);
    hipLaunchKernelGGL(blob_flatten_kernel, dim3(blocks * (unsigned)n), dim3(256), 0, s, d_parent, d_blobs, d_sums, pixels, blocks);
    hipLaunchKernelGGL(blob_scan_sums_kernel, dim3((unsigned)n), dim3(1024), 0, s, d_sums, (int)blocks, d_counts);
    hipLaunchKernelGGL(blob_rank_kernel, dim3(blocks * (unsigned)n), dim3(256), 0, s, d_parent, d_sums, pixels, blocks);
    HIP_CHECK(hipGetLastError());
}

void launch_blob_number(const int* d_numbers, uint32_t* d_blobs, const uint16_t* d_labels, int n, int h, int w, anh_region* d_table,
                        const unsigned long long* d_row_offsets, hipStream_t s) {
    const int64_t pixels = (int64_t)h * w;
    const unsigned per_image = blocks_of(pixels, 256);
    hipLaunchKernelGGL(blob_number_kernel, dim3(per_image * (unsigned)n), dim3(256), 0, s, d_numbers, d_blobs, d_labels, d_table, d_row_offsets, pixels, w, per_image);
    HIP_CHECK(hipGetLastError());
}

void launch_blob_stats(const uint32_t* d_blobs, const uint16_t* d_labels, const float* d_blended, int k, int n, int h, int w, const uint8_t* d_flags,
                       anh_region* d_table, const unsigned long long* d_row_offsets, uint32_t total_regions, bool filtering, hipStream_t s) {
    if (total_regions == 0) return;
    const int64_t pixels = (int64_t)h * w;
    const unsigned per_image = blocks_of(pixels, kStatPixels);
    hipLaunchKernelGGL(blob_stats_kernel, dim3(per_image * (unsigned)n), dim3(256), 0, s, d_blobs, d_labels, d_blended, k, d_flags, d_table, d_row_offsets, pixels, w,
                       per_image);
    hipLaunchKernelGGL(blob_finish_kernel, dim3((total_regions + 255) / 256), dim3(256), 0, s, d_table, total_regions, filtering ? 1 : 0);   // the rows lie back to back
    HIP_CHECK(hipGetLastError());
}

void launch_blob_filter(uint16_t* d_labels, const uint32_t* d_blobs, const anh_region* d_table, const unsigned long long* d_row_offsets, int n, int64_t pixels,
                        hipStream_t s) {
    const unsigned per_image = blocks_of(pixels, 256);
    hipLaunchKernelGGL(blob_filter_kernel, dim3(per_image * (unsigned)n), dim3(256), 0, s, d_labels, d_blobs, d_table, d_row_offsets, pixels, per_image);
    HIP_CHECK(hipGetLastError());
}

}  // namespace anh
