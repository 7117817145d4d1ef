// kernels_eval.hip — held-out evaluation on the device: ONE pass over the logits of `count` windows and their weighted labels gives, per
// window, the loss sums the trainer optimises (loss_kernel's arithmetic) and the confusion counts of the inference program's argmax
// (find_label's arithmetic).
//
// For every pixel with logits z[0..K):
//   predicted   the first class with the strictly largest (float)((double)z + gain), from -inf; 65535 when no class exceeds -inf (every
//               logit NaN or -inf).  Written to the predicted map, when one is given, for every pixel, labelled or not.
//   ignored     label == ANH_LABEL_IGNORE: nothing else happens.  Another label >= K sets the error flag.
//   counted     += 1 for a labelled pixel; if predicted == 65535: unclassified += 1 and nothing else; otherwise
//   confusion[truth][predicted] += 1, weight_sum += w, loss_sum += w * (-log max(softmax(z)[truth], 1e-10)): float max, expf, float sum in
//               class order, z / sum, logf, then the product and the accumulation in double — loss_kernel's term, without gains.
// So sum(confusion) + unclassified == counted by construction.  Pixels where some but not all logits are NaN are unspecified.
//
// Determinism.  The counts are integer atomics (LDS per workgroup, then u64 global).  A workgroup serves kEvalBlockPixels consecutive
// pixels of ONE image: which pixels depends on the plane size alone, not on the number of images or the image's place among them.  Which
// thread loads a pixel does depend on where the label map lies in memory (below), so the threads only leave the pixel's two floats
// (w, -log p) in LDS by the pixel's position; the workgroup then sums them in position order, and eval_finalize_kernel sums an image's
// partials in workgroup order.  Image i of any call therefore equals, bit for bit, the call on that image alone, wherever its maps lie.
//
// Shape (labels_from_logits_kernel, argmax_kernel).  The net's window is the label map here, so an image's planes are contiguous and a
// workgroup's pixels are one long row: item 0 is its head up to the first label on an 8-byte boundary (taken from the pointer), then
// spans of four — one 16-byte load per class plane (dword-aligned), one 8-byte label load, one 16-byte weight load — and a scalar tail;
// K > 8 runs scalar throughout, reading the planes once for the argmax and the maximum and once for the sum.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace anh {
namespace {

typedef float f32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned short u16x4a8 __attribute__((ext_vector_type(4), aligned(8)));

struct EvalArgs {
    const float* logits; const uint16_t* labels; const float* weights; const double* gains;
    int k; int64_t pixels; unsigned per_image;
    anh_eval_image* images; unsigned long long* confusion; uint16_t* predicted; double* partials; int* error_flag;
};

struct EvalShared {
    float w[kEvalBlockPixels], nl[kEvalBlockPixels];     // per pixel of the workgroup, by position: weight and -log p (0, 0: adds nothing)
    unsigned cells[kEvalMaxClasses * kEvalMaxClasses];   // 16 KB at K = 64
    double red[2][256];
    unsigned counted, unclassified;
};

struct EvalTerm { uint16_t predicted; float w, nl; };

// the votes of one pixel whose prediction is known; `softmax_term` computes -log max(p[truth], 1e-10) only where it is needed
template <class Term>
__device__ __forceinline__ EvalTerm eval_vote(EvalShared& s, int k, unsigned truth, uint16_t predicted, float weight, int* error_flag, unsigned& n_counted,
                                              unsigned& n_unclassified, Term&& softmax_term) {
    EvalTerm t{predicted, 0.f, 0.f};
    if (truth == ANH_LABEL_IGNORE) return t;
    if (truth >= (unsigned)k) { *error_flag = 1; return t; }   // every writer stores the same word
    ++n_counted;
    if (predicted == ANH_LABEL_IGNORE) { ++n_unclassified; return t; }
    atomicAdd(&s.cells[truth * (unsigned)k + predicted], 1u);
    t.w = weight;
    t.nl = softmax_term();
    return t;
}

// K <= 8: the pixel's logits in registers
__device__ __forceinline__ EvalTerm eval_pixel_regs(EvalShared& s, const float (&z)[8], const double (&g)[8], int k, unsigned truth, float weight, int* error_flag,
                                                    unsigned& n_counted, unsigned& n_unclassified) {
    uint16_t label = ANH_LABEL_IGNORE;
    float best = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < k) {
            const float value = (float)__dadd_rn((double)z[c], g[c]);
            if (value > best) { label = (uint16_t)c; best = value; }
        }
    return eval_vote(s, k, truth, label, weight, error_flag, n_counted, n_unclassified, [&] {
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < 8; ++c) if (c < k) m = fmaxf(m, z[c]);
        float sum = 0.f, mine = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < k) {
                const float e = expf(z[c] - m);
                sum += e;
                if ((unsigned)c == truth) mine = e;
            }
        return -logf(fmaxf(mine / sum, 1e-10f));
    });
}

// any K: the pixel's logits in memory, `plane` floats apart
__device__ __forceinline__ EvalTerm eval_pixel_mem(EvalShared& s, const float* z, size_t plane, const double* gains, int k, unsigned truth, float weight,
                                                   int* error_flag, unsigned& n_counted, unsigned& n_unclassified) {
    uint16_t label = ANH_LABEL_IGNORE;
    float best = -INFINITY, m = -INFINITY;
    for (int c = 0; c < k; ++c) {
        const float v = z[(size_t)c * plane];
        const float value = (float)__dadd_rn((double)v, gains ? gains[c] : 0.0);
        if (value > best) { label = (uint16_t)c; best = value; }
        m = fmaxf(m, v);
    }
    return eval_vote(s, k, truth, label, weight, error_flag, n_counted, n_unclassified, [&] {
        float sum = 0.f, mine = 0.f;
        for (int c = 0; c < k; ++c) {
            const float e = expf(z[(size_t)c * plane] - m);
            sum += e;
            if ((unsigned)c == truth) mine = e;
        }
        return -logf(fmaxf(mine / sum, 1e-10f));
    });
}

__global__ __launch_bounds__(256) void eval_tally_kernel(EvalArgs a) {
    __shared__ EvalShared s;
    const int k = a.k;
    const unsigned image = blockIdx.x / a.per_image, block = blockIdx.x - image * a.per_image;
    const int64_t p0 = (int64_t)block * kEvalBlockPixels;
    const int len = (int)min((int64_t)kEvalBlockPixels, a.pixels - p0);
    const size_t plane = (size_t)a.pixels, at = (size_t)image * plane + (size_t)p0;
    const float* logits = a.logits + (size_t)image * plane * (size_t)k + (size_t)p0;
    const uint16_t* labels = a.labels + at;
    const float* weights = a.weights ? a.weights + at : nullptr;
    uint16_t* predicted = a.predicted ? a.predicted + at : nullptr;
    for (int i = threadIdx.x; i < k * k; i += 256) s.cells[i] = 0;
    if (threadIdx.x == 0) { s.counted = 0; s.unclassified = 0; }
    __syncthreads();

    double g[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) g[c] = (a.gains && c < k) ? a.gains[c] : 0.0;
    unsigned n_counted = 0, n_unclassified = 0;
    const int head = min(len, (int)(((8 - (reinterpret_cast<uintptr_t>(labels) & 7)) & 7) >> 1));
    const int n_items = 1 + (len - head + 3) / 4;
    for (int it = threadIdx.x; it < n_items; it += 256) {
        const int xa = it == 0 ? 0 : head + 4 * (it - 1), xb = it == 0 ? head : min(len, xa + 4);
        if (xa >= xb) continue;
        if (k <= 8 && xb - xa == 4) {
            float v[4][8];
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (c < k) {
                    const f32x4a4 q = *reinterpret_cast<const f32x4a4*>(logits + (size_t)c * plane + xa);
                    v[0][c] = q[0]; v[1][c] = q[1]; v[2][c] = q[2]; v[3][c] = q[3];
                }
            const u16x4a8 y = *reinterpret_cast<const u16x4a8*>(labels + xa);
            f32x4a4 w = {1.f, 1.f, 1.f, 1.f};
            if (weights) w = *reinterpret_cast<const f32x4a4*>(weights + xa);
            uint16_t out[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const EvalTerm t = eval_pixel_regs(s, v[j], g, k, y[j], w[j], a.error_flag, n_counted, n_unclassified);
                s.w[xa + j] = t.w; s.nl[xa + j] = t.nl;
                out[j] = t.predicted;
            }
            if (predicted) {
                if ((reinterpret_cast<uintptr_t>(predicted + xa) & 7) == 0) {   // (the predicted map need not lie as the label map does)
                    u16x4a8 l;
                    l[0] = out[0]; l[1] = out[1]; l[2] = out[2]; l[3] = out[3];
                    *reinterpret_cast<u16x4a8*>(predicted + xa) = l;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) predicted[xa + j] = out[j];
                }
            }
            continue;
        }
        for (int x = xa; x < xb; ++x) {
            const unsigned y = labels[x];
            const float w = weights ? weights[x] : 1.f;
            EvalTerm t;
            if (k <= 8) {
                float z[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) z[c] = c < k ? logits[(size_t)c * plane + x] : 0.f;
                t = eval_pixel_regs(s, z, g, k, y, w, a.error_flag, n_counted, n_unclassified);
            } else
                t = eval_pixel_mem(s, logits + x, plane, a.gains, k, y, w, a.error_flag, n_counted, n_unclassified);
            s.w[x] = t.w; s.nl[x] = t.nl;
            if (predicted) predicted[x] = t.predicted;
        }
    }
    if (n_counted) atomicAdd(&s.counted, n_counted);
    if (n_unclassified) atomicAdd(&s.unclassified, n_unclassified);
    __syncthreads();

    if (threadIdx.x == 0) {
        if (s.counted) atomicAdd(reinterpret_cast<unsigned long long*>(&a.images[image].counted), (unsigned long long)s.counted);
        if (s.unclassified) atomicAdd(reinterpret_cast<unsigned long long*>(&a.images[image].unclassified), (unsigned long long)s.unclassified);
    }
    unsigned long long* confusion = a.confusion + (size_t)image * k * k;
    for (int i = threadIdx.x; i < k * k; i += 256)
        if (s.cells[i]) atomicAdd(confusion + i, (unsigned long long)s.cells[i]);
    // the two double sums of the workgroup, in position order whatever thread computed a pixel
    double loss = 0.0, weight = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) {
        loss += (double)s.w[i] * (double)s.nl[i];
        weight += (double)s.w[i];
    }
    s.red[0][threadIdx.x] = loss; s.red[1][threadIdx.x] = weight;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (threadIdx.x < step) { s.red[0][threadIdx.x] += s.red[0][threadIdx.x + step]; s.red[1][threadIdx.x] += s.red[1][threadIdx.x + step]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { a.partials[(size_t)blockIdx.x * 2] = s.red[0][0]; a.partials[(size_t)blockIdx.x * 2 + 1] = s.red[1][0]; }
}

// one wave per image: its workgroups' partials in a fixed order (lane l takes l, l + 64, ...; then the butterfly)
__global__ __launch_bounds__(64) void eval_finalize_kernel(const double* partials, unsigned per_image, anh_eval_image* images) {
    const double* mine = partials + (size_t)blockIdx.x * per_image * 2;
    double loss = 0.0, weight = 0.0;
    for (unsigned b = threadIdx.x; b < per_image; b += 64) { loss += mine[(size_t)b * 2]; weight += mine[(size_t)b * 2 + 1]; }
    for (int off = 32; off > 0; off >>= 1) { loss += __shfl_xor(loss, off, 64); weight += __shfl_xor(weight, off, 64); }
    if (threadIdx.x == 0) { images[blockIdx.x].loss_sum = loss; images[blockIdx.x].weight_sum = weight; }
}

unsigned eval_blocks_per_image(int64_t pixels) { return (unsigned)((pixels + kEvalBlockPixels - 1) / kEvalBlockPixels); }

}  // namespace

size_t eval_partial_doubles(int count, int64_t pixels) { return (size_t)count * eval_blocks_per_image(pixels) * 2; }

void launch_eval_tally(const float* d_logits, const uint16_t* d_labels, const float* d_weights, int count, int k, int64_t pixels, const double* d_gains,
                       anh_eval_image* d_images, unsigned long long* d_confusion, uint16_t* d_predicted, double* d_partials, int* d_error_flag, hipStream_t s) {
    ANH_REQUIRE(count >= 1 && pixels >= 1, "evaluate: empty batch");
    ANH_REQUIRE(k >= 1 && k <= kEvalMaxClasses, "evaluate: the class count must be within 1..64");
    const unsigned per_image = eval_blocks_per_image(pixels);
    ANH_REQUIRE((uint64_t)count * per_image < (1ull << 31), "evaluate: too many pixels for one launch");
    EvalArgs a{d_logits, d_labels, d_weights, d_gains, k, pixels, per_image, d_images, d_confusion, d_predicted, d_partials, d_error_flag};
    hipLaunchKernelGGL(eval_tally_kernel, dim3(per_image * (unsigned)count), dim3(256), 0, s, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(eval_finalize_kernel, dim3((unsigned)count), dim3(64), 0, s, d_partials, per_image, d_images);
    HIP_CHECK(hipGetLastError());
}

}  // namespace anh
