// kernels_score.hip — scoring a result label map against its ground truth on the device (annonet_infer_main.cpp:482-491 and :202-272,
// annonet_host.h: RegionScorer): the per-pixel confusion counts and the two-way per-region votes.
//
// A pixel is LABELLED where truth < K.  A prediction >= K (65535: an all-NaN pixel) casts no vote.
//
//   per pixel    labelled = number of labelled pixels; pixel[t][p] = labelled pixels with truth == t and result == p < K
//   per region   for each map M of (truth, result): its regions are its blobs (kernels_blobs.hip) plus region 0 = the pixels where
//                M == 0.  Every region with labelled pixels votes once: t = the class most of them carry in the truth, p = the class most
//                of them carry in the result; where t != 0 the background predictions are disregarded unless the region's predictions
//                are background only.  Ties go to the smaller class.
//
// Within one of the two passes one side of the vote is constant over a region: every pixel of a truth blob carries the blob's truth
// value, every pixel of a result blob the blob's result value, and region 0 carries 0.  So a region keeps ONE histogram of K counters —
// of the result classes (truth map) or of the truth classes (result map) — and one word with its own value:
//
//   vote table   one row of K + 1 words per region, the regions of the 2n maps back to back ([truth maps ; result maps], each map's rows
//                begin at row_offsets[map]): row[c] = labelled pixels of the region whose OTHER map says c, row[K] = the region's value
//   tally        one pass over the pixels of [n][h][w]: labelled, pixel and the vote table, by integer atomics only (the same bits on
//                every run), summed per wave and per workgroup before they touch global memory, as blob_stats_body does
//   decide       one thread per row applies the rule and adds 1 to region[image][t][p]
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace anh {
namespace {

constexpr int kTallyPixels = 4096;     // pixels per block of the tally launch (256 threads x 16)
constexpr int kVoteSlots = 256;        // LDS table of the tally launch, keyed by the counter's index in the vote table
constexpr int kPixelCells = 1024;      // K * K up to here: the block's per-pixel counts stay in LDS

struct VoteSlots {
    unsigned long long key[kVoteSlots];   // index of the counter in the vote table + 1 (0: free)
    unsigned count[kVoteSlots];
};

// `value` is the region's own value; region 0 (blob == 0) has value 0, which the cleared table already says
__device__ __forceinline__ void vote_to_global(unsigned* votes, size_t row_at, int k, unsigned cls, unsigned blob, unsigned value, unsigned count) {
    atomicAdd(votes + row_at + cls, count);
    if (blob) votes[row_at + (size_t)k] = value;   // every writer of a row stores the same word
}

__device__ __forceinline__ void vote_to_lds(VoteSlots& s, unsigned* votes, size_t row_at, int k, unsigned cls, unsigned blob, unsigned value, unsigned count) {
    const unsigned long long key = (unsigned long long)(row_at + cls) + 1ull;
    unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 56);   // 8 bits
#pragma unroll 1
    for (int probe = 0; probe < 8; ++probe, slot = (slot + 1) & (kVoteSlots - 1)) {
        const unsigned long long held = atomicCAS(&s.key[slot], 0ull, key);
        if (held != 0 && held != key) continue;
        atomicAdd(&s.count[slot], count);
        if (held == 0 && blob) votes[row_at + (size_t)k] = value;
        return;
    }
    vote_to_global(votes, row_at, k, cls, blob, value, count);   // a crowded table: more (region, class) pairs in this block than it holds
}

// one block = up to 4096 pixels of ONE image; truth / result / the two blob maps point at that image's planes, row_t / row_r are the first
// rows of its truth map's and its result map's regions, labelled and pixel its outputs
__device__ __forceinline__ void score_tally_body(const uint16_t* truth, const uint16_t* result, const uint32_t* blobs_t, const uint32_t* blobs_r,
                                                 unsigned long long row_t, unsigned long long row_r, int k, unsigned* votes,
                                                 unsigned long long* labelled, unsigned long long* pixel, int64_t pixels, unsigned block) {
    __shared__ VoteSlots s;
    __shared__ unsigned cells[kPixelCells];
    __shared__ unsigned n_labelled;
    const bool cells_in_lds = (int64_t)k * k <= kPixelCells;
    const int n_cells = cells_in_lds ? k * k : 0;
    for (int i = threadIdx.x; i < kVoteSlots; i += 256) { s.key[i] = 0; s.count[i] = 0; }
    for (int i = threadIdx.x; i < n_cells; i += 256) cells[i] = 0;
    if (threadIdx.x == 0) n_labelled = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const size_t stride = (size_t)k + 1;
    const int64_t base = (int64_t)block * kTallyPixels;
#pragma unroll 1
    for (int it = 0; it < kTallyPixels / 256; ++it) {
        const int64_t p = base + it * 256 + threadIdx.x;
        unsigned t = 0, r = 0, bt = 0, br = 0;
        bool lab = false;
        if (p < pixels) {
            t = truth[p];
            lab = t < (unsigned)k;
            if (lab) { r = result[p]; bt = blobs_t[p]; br = blobs_r[p]; }
        }
        const unsigned long long active = __ballot(lab);
        if (active == 0) continue;
        const int first = __ffsll((long long)active) - 1;
        const unsigned t0 = (unsigned)__shfl((int)t, first, 64), r0 = (unsigned)__shfl((int)r, first, 64);
        const unsigned bt0 = (unsigned)__shfl((int)bt, first, 64), br0 = (unsigned)__shfl((int)br, first, 64);
        // the whole wave in one region of either map with one class pair (the inside of large regions): ONE lane carries the wave's count
        const bool uniform = __ballot(lab && (t != t0 || r != r0 || bt != bt0 || br != br0)) == 0;
        if (lane == first) atomicAdd(&n_labelled, (unsigned)__popcll(active));
        if (uniform ? lane == first : lab) {
            const unsigned count = uniform ? (unsigned)__popcll(active) : 1u;
            if (r < (unsigned)k) {
                const unsigned cell = t * (unsigned)k + r;   // K <= 65535: below 2^32
                if (cells_in_lds) atomicAdd(&cells[cell], count);
                else atomicAdd(pixel + cell, (unsigned long long)count);
                vote_to_lds(s, votes, (size_t)(row_t + bt) * stride, k, r, bt, t, count);
            }
            vote_to_lds(s, votes, (size_t)(row_r + br) * stride, k, t, br, r, count);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && n_labelled) atomicAdd(labelled, (unsigned long long)n_labelled);
    for (int i = threadIdx.x; i < n_cells; i += 256)
        if (cells[i]) atomicAdd(pixel + i, (unsigned long long)cells[i]);
    for (int i = threadIdx.x; i < kVoteSlots; i += 256)
        if (s.key[i]) atomicAdd(votes + (s.key[i] - 1ull), s.count[i]);
}

// ceil(pixels / 4096) blocks per image, so no workgroup spans two images; maps = [n truth maps ; n result maps], blobs likewise
__global__ __launch_bounds__(256) void score_tally_kernel(const uint16_t* maps, const uint32_t* blobs, int n, int k, const unsigned long long* row_offsets,
                                                          unsigned* votes, unsigned long long* labelled, unsigned long long* pixel, int64_t pixels,
                                                          unsigned per_image) {
    const unsigned image = blockIdx.x / per_image;
    const size_t at_t = (size_t)image * (size_t)pixels, at_r = ((size_t)n + image) * (size_t)pixels;
    score_tally_body(maps + at_t, maps + at_r, blobs + at_t, blobs + at_r, row_offsets[image], row_offsets[(size_t)n + image], k, votes, labelled + image,
                     pixel + (size_t)image * k * k, pixels, blockIdx.x - image * per_image);
}

// one thread per row of the vote table; row_offsets: the 2n maps' first rows, ascending
__global__ __launch_bounds__(256) void score_decide_kernel(const unsigned* votes, const unsigned long long* row_offsets, int n, int k, unsigned long long rows,
                                                           unsigned long long* region) {
    const unsigned long long row = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (row >= rows) return;
    int lo = 0, hi = 2 * n - 1;   // the last map whose first row is not behind this one (maps without a row of their own do not exist: region 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_offsets[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const bool truth_map = lo < n;
    const unsigned image = (unsigned)(truth_map ? lo : lo - n);
    const unsigned* c = votes + (size_t)row * ((size_t)k + 1);
    int best = -1, best_defect = -1;   // first index of the maximum over all classes / over the classes behind 0
    unsigned most = 0, most_defect = 0;
    for (int i = 0; i < k; ++i) {
        const unsigned v = c[i];
        if (v > most) { most = v; best = i; }
        if (i > 0 && v > most_defect) { most_defect = v; best_defect = i; }
    }
    if (best < 0) return;   // no labelled pixel, or none with a prediction below K
    const unsigned value = c[k];
    if (value >= (unsigned)k) return;   // a result blob of a value >= K predicts nothing (a truth blob of one has no labelled pixel)
    unsigned t, p;
    if (truth_map) {   // the row is the histogram of the predictions; the truth is the region's value
        t = value;
        p = (t != 0 && best_defect >= 0) ? (unsigned)best_defect : (unsigned)best;   // background votes count only where nothing else was predicted
    } else {           // the row is the histogram of the truth; the one prediction is the region's value
        t = (unsigned)best;
        p = value;
    }
    atomicAdd(region + ((size_t)image * k + t) * k + p, 1ull);
}

}  // namespace

void launch_score_tally(const uint16_t* d_maps, const uint32_t* d_blobs, int n, int k, int h, int w, const unsigned long long* d_row_offsets, unsigned* d_votes,
                        unsigned long long* d_labelled, unsigned long long* d_pixel, hipStream_t s) {
    ANH_REQUIRE(blob_batch_fits(2 * n, h, w), "scoring a stack: too many pixels for one launch");
    const int64_t pixels = (int64_t)h * w;
    const unsigned per_image = (unsigned)((pixels + kTallyPixels - 1) / kTallyPixels);
    hipLaunchKernelGGL(score_tally_kernel, dim3(per_image * (unsigned)n), dim3(256), 0, s, d_maps, d_blobs, n, k, d_row_offsets, d_votes, d_labelled, d_pixel, pixels,
                       per_image);
    HIP_CHECK(hipGetLastError());
}

void launch_score_decide(const unsigned* d_votes, const unsigned long long* d_row_offsets, int n, int k, uint32_t rows, unsigned long long* d_region, hipStream_t s) {
    if (rows == 0) return;
    hipLaunchKernelGGL(score_decide_kernel, dim3((unsigned)(((uint64_t)rows + 255) / 256)), dim3(256), 0, s, d_votes, d_row_offsets, n, k, (unsigned long long)rows, d_region);
    HIP_CHECK(hipGetLastError());
}

}  // namespace anh
