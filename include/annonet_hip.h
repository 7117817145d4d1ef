/*
 * annonet_hip.h — C ABI of libannonet_hip.so, the MI355X (gfx950) implementation of annonet's hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * The C++ shims include/NetPimpl.h and include/tiling/tiling.h wrap it back into the class surface
 * annonet's host code uses (dlib-dnn-pimpl-wrapper/NetPimpl.h and tiling/tiling.h, both absent from the
 * reference snapshot and therefore known only from their call sites, cited per function below).
 * All file:line citations are relative to the reference tree.
 *
 * Conventions
 *   - every function returns anh_status (0 = ok) unless stated; on failure anh_last_error() (thread-local)
 *     holds the message.  Nothing aborts: device out-of-memory is ANH_ERR_OOM, so a host that throws on
 *     failure exits with a positive code (find_max_mini-batch_size.cmd:49-53 relies on that).
 *   - images are u8, row-major HWC, channel order R,G,B (dlib::matrix<rgb_pixel>) or one channel.
 *   - network outputs are fp32 NCHW (annonet_infer.cpp:26-30).
 *   - "host" entry points take host pointers and copy; "_device" entry points take pointers that are
 *     already resident in this GPU's HBM and enqueue on the handle's stream without synchronising.
 *   - one thread drives a handle at a time (annonet_train_main.cpp:583-614, annonet_infer_main.cpp:446-494).
 */
#ifndef ANNONET_HIP_H
#define ANNONET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ANH_OK = 0,
    ANH_ERR_INVALID = 1,  /* bad argument / precondition (DLIB_CASSERT analogue, annonet_infer.cpp:90-94) */
    ANH_ERR_OOM = 2,      /* device or host allocation failed */
    ANH_ERR_DEVICE = 3,   /* HIP runtime error, no usable GPU */
    ANH_ERR_IO = 4,       /* malformed blob / file error */
    ANH_ERR_INTERNAL = 5
} anh_status;

typedef enum {
    ANH_FP32 = 0, /* parity mode: fp32 storage, fp32 k-ordered fmaf chains (bit-exact inference vs the oracle) */
    ANH_BF16 = 1  /* throughput mode: bf16 storage + bf16 MFMA, fp32 accumulate, fp32 master weights */
} anh_precision;

#define ANH_LABEL_IGNORE 65535 /* dlib::loss_multiclass_log_per_pixel_::label_to_ignore (annonet.cpp:25) */

/* Build-time knobs of the reference made run-time: DLIB_DNN_PIMPL_WRAPPER_LEVEL_COUNT (appveyor.yml:7-20),
 * DLIB_DNN_PIMPL_WRAPPER_GRAYSCALE_INPUT (annonet_train_main.cpp:93-100), SetNetWidth (annonet_train_main.cpp:402),
 * SetClassCount (:405). */
typedef struct {
    int levels;          /* 0..3 down/up-sampling levels */
    int in_channels;     /* 3 = RGB, 1 = grayscale */
    int classes;         /* K */
    double width_scaler; /* --net-width-scaler */
    int min_filters;     /* --net-width-min-filter-count */
    int precision;       /* anh_precision */
} anh_net_config;

/* One layer of the net (the stand-in for NetStructure.h). Offsets index the canonical
 * parameter blob: con filters [cout][cin][ky][kx], cont filters [cin][cout][ky][kx], bias[cout],
 * gamma[cout], beta[cout]; running-stats blob: mean[cout], var[cout] per bn layer. */
typedef struct {
    int type; /* 0 = con, 1 = cont */
    int k, stride, pad, cin, cout;
    int in_a, in_b; /* producing layer; -1 = image; in_b = -2: no skip input */
    int has_bn, has_bias;
    int64_t w_off, b_off, g_off, beta_off, rs_off;
} anh_layer_desc;

typedef struct { uint16_t label; float weight; } anh_wlabel; /* dlib weighted_label (annonet_train.h:80) */
typedef struct { long left, top, right, bottom; } anh_rect;   /* dlib::rectangle, inclusive */
typedef struct { anh_rect full_rect, unique_rect; } anh_tile; /* tiling::dlib_tile (annonet_infer.cpp:46-47,118,138) */
typedef struct { int max_tile_width, max_tile_height, overlap_x, overlap_y; } anh_tiling_params; /* tiling::parameters (annonet_infer_main.cpp:423-427) */

typedef struct anh_runtime anh_runtime; /* NetPimpl::RuntimeNet */
typedef struct anh_trainer anh_trainer; /* NetPimpl::TrainingNet */

const char* anh_last_error(void);
void anh_free(void* p); /* releases buffers this library returned (serialize, get_tiles) */

/* dlib::cuda::set_device (annonet_train_main.cpp:392-394): device used by handles created afterwards on this thread */
int anh_set_device(int device);
int anh_device_count(void); /* number of visible GPUs; 0 when none (never fails) */
/* One process, several GPUs (the reference has only --primary-cuda-device, annonet_train_main.cpp:307,392-394):
 * handles created afterwards ON THIS THREAD hold one replica per listed device.
 *   TrainingNet::StartTraining (anh_trainer_step) splits the mini-batch along N over the replicas (annonet_train_main.cpp:583-614
 *     stays unchanged), sums the flat gradient buckets with ONE all-reduce (RCCL over xGMI) and applies the identical update;
 *     the loss scale uses the whole batch, batch-norm statistics are per replica;
 *   annonet_infer (anh_infer) splits the tile list into contiguous chunks, exchanges the plane sums where tiles of different
 *     replicas overlap (one RCCL all-reduce) and returns ONE host label map.
 * n = 0 returns to "the thread's current device".  A list that repeats a device is a rehearsal on fewer GPUs (tests): the
 * exchange then runs as a fixed-order sum on the first replica's stream instead of RCCL. */
int anh_set_devices(const int* devices, int n);
int anh_handle_replicas(void* handle, int is_trainer); /* number of replicas (devices) a handle drives */
/* What the exchange step of data-parallel StartTraining (anh_trainer_step on a handle with several replicas) costs: the HOST time of a
 * call (the reference's loop is one thread: /root/reference/annonet_train_main.cpp:583-614 — what it spends inside StartTraining bounds
 * the step rate whatever the GPUs do), and, on every 8th step (ANH_EXCHANGE_SAMPLE), the device time of the all-reduce's two parts on
 * replica 0 (tail = the bulk of the bucket, reduced on a side stream while backward still runs; head = the first layers, on the main
 * stream).  The replicas of a handle are driven by persistent worker threads; worker_calls counts their wake-ups.
 * uses_rccl names the transport of the exchange: 1 = RCCL over xGMI; 2 = peer copies between distinct devices (taken by itself, in the
 * same process, when the RCCL communicators cannot be created, or with ANH_COLLECTIVE_TRANSPORT=peer); 0 = a device list that repeats
 * a device (rehearsal on fewer GPUs).  One host thread per handle; host-side waits of a handle with several replicas give up after
 * ANH_REPLICA_TIMEOUT_S seconds (default 180) with ANH_ERR_DEVICE instead of blocking for ever. */
typedef struct {
    int replicas, early_reduce, uses_rccl, rccl_version;
    int64_t steps, samples, worker_calls, bucket_bytes;
    double host_us_mean, host_us_last, host_wait_us_mean; /* wall time of a call; of which blocked on the GPU (staging set of step k-2 still uploading) */
    double allreduce_tail_us_mean, allreduce_head_us_mean, allreduce_tail_us_last, allreduce_head_us_last;
} anh_exchange_stats;
int anh_trainer_exchange_stats(anh_trainer* h, anh_exchange_stats* out);
void anh_trainer_reset_exchange_stats(anh_trainer* h);
/* Per-rank delivery of a sharded annonet_infer()'s label map (the reference's writer threads consume HOST label maps,
 * /root/reference/annonet_infer_main.cpp:403-419): every rank copies the rectangles it answers for from its device-resident map straight
 * into ONE host map that all ranks of the job map (POSIX shared memory), over its own PCIe link — nothing funnels through rank 0.
 * anh_host_register page-locks host memory the caller owns (the shared map) so the copies run asynchronously; anh_labels_rect_to_host
 * enqueues the copy of rows [top, bottom] x columns [left, right] (inclusive) of a [height x width] u16 map on `stream`. */
int anh_host_register(void* p, size_t bytes);
int anh_host_unregister(void* p);
int anh_labels_rect_to_host(const uint16_t* d_labels, uint16_t* h_labels, int width, int height, int left, int top, int right, int bottom, void* stream);
/* the host logic of the two splits, exported for tests: replica `rank` of `world` takes units [*lo, *hi) of n */
int anh_shard_range(int64_t n, int world, int rank, int64_t* lo, int64_t* hi);

/* ---- static dimension maths ---- */
/* TrainingNet::GetRequiredInputDimension() (annonet_train_main.cpp:376,441; annonet_infer_main.cpp:421): receptive-field side */
int anh_required_input_dim(const anh_net_config* cfg);
/* RuntimeNet::GetRecommendedInputDimension(int) (annonet_infer.cpp:49-50; annonet_train_main.cpp:382): smallest valid side >= n */
int anh_recommended_input_dim(int levels, int n);

/* ---- net description ---- */
int anh_net_layer_count(const anh_net_config* cfg);
int anh_net_layer(const anh_net_config* cfg, int index, anh_layer_desc* out);
int64_t anh_net_param_count(const anh_net_config* cfg);
int64_t anh_net_running_count(const anh_net_config* cfg);

/* ---- RuntimeNet ---- */
int anh_runtime_create(const anh_net_config* cfg, anh_runtime** out); /* default-constructed RuntimeNet (annonet_infer_main.cpp:347) */
void anh_runtime_destroy(anh_runtime* h);
int anh_runtime_config(const anh_runtime* h, anh_net_config* out);
int anh_runtime_set_params(anh_runtime* h, const float* params, int64_t n_params, const float* running, int64_t n_running);
int anh_runtime_get_params(const anh_runtime* h, float* params, int64_t n_params, float* running, int64_t n_running);
/* RuntimeNet::Serialize / Deserialize (annonet_train_main.cpp:558-561; annonet_infer_main.cpp:347-351): opaque blob */
int anh_runtime_serialize(const anh_runtime* h, void** blob, size_t* size);
int anh_runtime_deserialize(const void* blob, size_t size, int precision, anh_runtime** out);
/* RuntimeNet::Forward(const input_type&) (annonet_infer.cpp:77): returns a library-owned fp32 NCHW tensor,
 * valid until the next call on this handle; k = classes, nr x nc = input tile size (annonet_infer.cpp:80-100). */
int anh_runtime_forward(anh_runtime* h, const uint8_t* image_hwc, int n, int height, int width,
                        const float** out_nchw, int* k, int* nr, int* nc);
int anh_runtime_forward_device(anh_runtime* h, const uint8_t* d_image_hwc, int n, int height, int width, float* d_out_nchw);
/* annonet_infer() (annonet_infer.h:34-42, annonet_infer.cpp:32-240) in one call: tile, clamp-pad, forward, blend,
 * argmax(+gain), optional detection-level blob filter.  gains / detection_levels: K doubles or NULL.
 * tiling: NULL = one tile (tiling::parameters() default argument, annonet_infer.h:41).
 * blended_out (optional, host): K planes H*W fp32 = annonet_infer_temp::blended_output (annonet_infer.h:31). */
int anh_infer(anh_runtime* h, const uint8_t* image_hwc, int height, int width,
              const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
              uint16_t* result_labels, float* blended_out);
/* same with the image and the label map resident in HBM; explicit tile list (e.g. one rank's shard) when tiles != NULL */
int anh_infer_device(anh_runtime* h, const uint8_t* d_image_hwc, int height, int width,
                     const double* gains, const anh_tiling_params* tiling,
                     const anh_tile* tiles, size_t n_tiles, uint16_t* d_result_labels, float* d_blended);
/* annonet_infer() over n >= 1 images of ONE size in one call (a folder of camera frames): the images' tile lists are concatenated image by
 * image and cut into forward batches that may span image boundaries, so frames that are one tile each run the net with several frames
 * per launch.  Every image's label map (and planes) equal, bit for bit, what anh_infer returns for that image alone.
 * images_hwc / results: n host pointers; blended_out: NULL, or n pointers of which each may be NULL.  Where every image is one tile and
 * neither planes nor detection levels are asked for, the labels come straight from the batch's logits and no planes are written.
 * A batch that does not fit returns ANH_ERR_OOM before any kernel is enqueued and leaves the handle usable.  On a handle with R replicas
 * replica r computes the images anh_shard_range(n, R, r) (an image is computed wholly on one replica); n < R goes image by image. */
int anh_infer_batch(anh_runtime* h, const uint8_t* const* images_hwc, int n, int height, int width,
                    const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                    uint16_t* const* results, float* const* blended_out);
/* the same with everything resident in HBM on the handle's first device, enqueued on the handle's stream without synchronising:
 * d_images_hwc [n][H][W][C], d_results [n][H][W], d_blended [n][K][H][W] or NULL */
int anh_infer_batch_device(anh_runtime* h, const uint8_t* d_images_hwc, int n, int height, int width,
                           const double* gains, const anh_tiling_params* tiling, uint16_t* d_results, float* d_blended);
/* find_label (annonet_infer.cpp:170-185) straight from the logits of a batch whose samples are whole images: d_logits
 * [count][classes][win_height][win_width] fp32, the net input window starting at (left, top) in image coordinates and covering the image
 * (top <= 0, left <= 0, height - top <= win_height, width - left <= win_width); d_result [count][height][width].  gains: `classes`
 * host doubles or NULL.  With the window equal to the image it labels `count` sets of class planes in one launch. */
int anh_labels_from_logits_device(anh_runtime* h, const float* d_logits, int count, int classes, int win_height, int win_width, int top, int left,
                                  int height, int width, const double* gains, uint16_t* d_result);
/* the host logic of the batches, exported for tests: the tile list of ONE image, n_images images, the net's level count and a cap on the
 * batch size -> *pairs = (image, tile) index pairs in forward order (2 * n_tiles * n_images ints), *batch_sizes = the size of each of the
 * *n_batches batches; both blocks are released with anh_free */
int anh_infer_batch_plan(const anh_tile* tiles, size_t n_tiles, int n_images, int levels, int cap, int** pairs, int** batch_sizes, size_t* n_batches);
/* ---- downscaled inference: a net trained with a downscaling factor (annonet.dnn carries it) sees every image shrunk by it ----
 * read_sample shrinks the image with dlib::resize_image(1.0 / factor, image), bilinear (annonet.cpp:153); the inference program blows the
 * label map back up with resize_label_image, nearest neighbour (annonet_infer_main.cpp:413, annonet.cpp:132-141).  Both run on the device
 * here, with the arithmetic of annonet_amd/host/annonet_host.h (dlib's sampling grid is restated there [UPSTREAM-UNVERIFIED]): bit-exact
 * against that host code, any source and destination size.
 * anh_scaled_dims: the size dlib::resize_image(1.0 / factor, img) gives: round(height * (1.0 / factor)), round(width * (1.0 / factor))
 * — the factor is inverted first, as read_sample does.  Any factor > 0 whose scaled sides stay within 1..32768 is accepted. */
int anh_scaled_dims(int height, int width, double downscaling_factor, int* scaled_height, int* scaled_width);
/* the two resizes on their own, device-resident, enqueued on the given stream: u8 HWC image with 1 or 3 channels; u16 label map */
int anh_resize_image_device(const uint8_t* d_src_hwc, int channels, int src_h, int src_w, uint8_t* d_dst_hwc, int dst_h, int dst_w, void* hip_stream);
int anh_resize_labels_device(const uint16_t* d_src, int src_h, int src_w, uint16_t* d_dst, int dst_h, int dst_w, void* hip_stream);
/* read_sample's resize + annonet_infer() + resize_label_image in one call: image_hwc comes at its ORIGINAL size height x width.
 * result_labels: height x width (original size).  scaled_labels (optional): the map at the net's resolution (anh_scaled_dims), as
 * annonet_infer() leaves it — the inference program scores on it (annonet_infer_main.cpp:482-492).  blended_out (optional): K planes at
 * the net's resolution.  The detection-level filter runs at the net's resolution, before the map is blown up, as in the reference.
 * downscaling_factor == 1 returns exactly what anh_infer returns.  On a handle with several replicas every replica shrinks the image
 * itself and replica 0 blows up the merged map. */
int anh_infer_scaled(anh_runtime* h, const uint8_t* image_hwc, int height, int width, double downscaling_factor,
                     const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                     uint16_t* result_labels, uint16_t* scaled_labels, float* blended_out);
/* the same with the image and the maps resident in HBM, enqueued on the handle's stream without synchronising: d_result_labels
 * height x width; d_scaled_labels (optional) and d_blended (optional, K planes) at the net's resolution */
int anh_infer_scaled_device(anh_runtime* h, const uint8_t* d_image_hwc, int height, int width, double downscaling_factor,
                            const double* gains, const anh_tiling_params* tiling,
                            uint16_t* d_result_labels, uint16_t* d_scaled_labels, float* d_blended);
/* ---- downscaled inference over n >= 1 images of ONE original size (anh_infer_scaled composed with anh_infer_batch) ----
 * the two resizes over `count` images that lie back to back, [count][h][w][C] and [count][h][w], by ONE launch each: every image is
 * resized on its own (no row or column reads a neighbouring image) and equals what the single-image call gives for it */
int anh_resize_image_batch_device(const uint8_t* d_src_hwc, int count, int channels, int src_h, int src_w,
                                  uint8_t* d_dst_hwc, int dst_h, int dst_w, void* hip_stream);
int anh_resize_labels_batch_device(const uint16_t* d_src, int count, int src_h, int src_w,
                                   uint16_t* d_dst, int dst_h, int dst_w, void* hip_stream);
/* n originals up, ONE batched shrink, the forward batches of anh_infer_batch at the net's resolution (anh_scaled_dims), the detection-level
 * filter per image at the net's resolution, ONE batched blow-up, n original-size maps down.  results[i] (height x width) equals, bit for
 * bit, what anh_infer_scaled returns for image i alone.  scaled_labels / blended_out: NULL, or n pointers of which each may be NULL:
 * scaled_labels[i] is the map at the net's resolution, blended_out[i] K planes at the net's resolution.  downscaling_factor == 1 is
 * exactly anh_infer_batch (the scaled maps are copies of the results).  Everything the call needs is reserved before its first kernel
 * or copy: a batch that does not fit returns ANH_ERR_OOM and leaves the handle usable.  On a handle with R replicas replica r shrinks,
 * infers and blows up the images anh_shard_range(n, R, r) on its own; n < R goes image by image through anh_infer_scaled. */
int anh_infer_scaled_batch(anh_runtime* h, const uint8_t* const* images_hwc, int n, int height, int width, double downscaling_factor,
                           const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                           uint16_t* const* results, uint16_t* const* scaled_labels, float* const* blended_out);
/* the same with everything resident in HBM on the handle's first device, enqueued on the handle's stream without synchronising:
 * d_images_hwc [n][H][W][C], d_results [n][H][W]; d_scaled_labels [n][sh][sw] and d_blended [n][K][sh][sw] are optional (NULL) */
int anh_infer_scaled_batch_device(anh_runtime* h, const uint8_t* d_images_hwc, int n, int height, int width, double downscaling_factor,
                                  const double* gains, const anh_tiling_params* tiling,
                                  uint16_t* d_results, uint16_t* d_scaled_labels, float* d_blended);
/* ---- connected blobs: what annonet_infer() leaves in annonet_infer_temp::connected_blobs / detection_seeds (annonet_infer.cpp:194-223) ----
 * A blob is an 8-connected set of pixels of EQUAL non-zero label (0 = background; every other value, ANH_LABEL_IGNORE included, is a
 * label like the rest).  Blobs are numbered 1, 2, ... in raster order of their first pixel, the numbering annonet_amd/host/annonet_host.h:
 * label_connected_blobs restates for dlib's routine [UPSTREAM-UNVERIFIED].  Labelling runs on the device (block-based union-find); the maps
 * are limited to height * width < 2^31 pixels (ANH_ERR_INVALID beyond).  All work runs on the handle's stream (replica 0 of a handle with
 * several); the calls synchronise it, because the blob count comes back to the host.
 * One row of the region table, by integer atomics only — the same bits on every run: */
typedef struct {
    uint32_t blob;                   /* the blob's number, 1-based: row i of a table describes blob i + 1 */
    uint16_t label;
    uint16_t detected;               /* a positive detection level was given: seeds > 0; none: 1 */
    int32_t left, top, right, bottom; /* bounding box, inclusive */
    int32_t first_row, first_col;    /* the blob's first pixel in raster order */
    int64_t area, seeds;             /* pixels; detection seeds attributed to the blob (annonet_infer.cpp:199-213,222) */
    float peak;                      /* largest blended[label][p] - blended[0][p] over the blob's pixels, subtracted in float; NaN never wins;
                                        -inf for a label >= classes (and where every margin is NaN) */
} anh_region;
/* d_labels [height][width] u16 -> d_blobs [height][width] u32 (0 on background, else the blob's number);
 * *count = "labels including the background one" = blobs + 1, as label_connected_blobs returns it */
int anh_label_blobs_device(anh_runtime* h, const uint16_t* d_labels, int height, int width, uint32_t* d_blobs, uint32_t* count);
/* The table of every blob of the label map AS IT COMES IN, in number order: *regions (malloc'd, release with anh_free) holds *n_regions
 * rows.  d_blended: `classes` planes [height][width].  detection_levels: `classes` host doubles or NULL; a pixel is a seed of its blob
 * where blended[label] - blended[0] > levels[label] - levels[0], as the detection-level filter of anh_infer decides it
 * (ANH_DET_SEED_REFERENCE_ORDER=1: the reference's transposed lookup, as there).  When no level is positive (NULL or all zero) the levels
 * count as zeros for `seeds`, nothing is ever removed and detected = 1 in every row.  apply_filter != 0 with a positive level: ONE launch
 * afterwards sets d_labels to 0 on every blob without a seed — the map anh_infer's filter leaves; the blob map keeps the numbers of the
 * removed blobs.  d_blobs: NULL, or height * width u32 that receive the blob map.  Everything but the table is reserved before the
 * first kernel; the table is reserved once the count is known, and if that fails the call returns ANH_ERR_OOM and the handle stays usable. */
int anh_regions_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int classes, int height, int width,
                       const double* detection_levels, int apply_filter, uint32_t* d_blobs, anh_region** regions, size_t* n_regions);
/* The detection-level filter of anh_infer alone, on a resident label map [height][width] and its `classes` planes, in place: the flood
 * launches every anh_infer form with a positive level runs (not the one-launch filter of the regions calls; both leave the same map).
 * detection_levels: `classes` host doubles or NULL.  No positive level: the map is left untouched and *rounds = 0.  Otherwise every blob
 * without a seed becomes 0 and *rounds (NULL allowed) receives the host rounds made, the quiet last one included.  The call waits for
 * the stream: the map is final when it returns. */
int anh_detection_filter_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int classes, int height, int width,
                                const double* detection_levels, int* rounds /* nullable */);
/* anh_infer plus the region table of its UNFILTERED label map (annonet_infer.cpp:217 labels before :229-238 filter): result_labels and
 * blended_out are bit-identical to what anh_infer returns for the same arguments on one device.  blobs: NULL, or height * width u32 on
 * the host. */
int anh_infer_regions(anh_runtime* h, const uint8_t* image_hwc, int height, int width,
                      const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                      uint16_t* result_labels, uint32_t* blobs, float* blended_out, anh_region** regions, size_t* n_regions);
/* ---- the same over n >= 1 label maps of ONE size lying back to back, with a number of launches that does not depend on n ----
 * d_labels [n][height][width], d_blobs [n][height][width], d_blended [n][classes][height][width].  Every image is labelled on its own
 * (no blob reaches from one image into the next) and its blob numbers restart at 1: image i gets, bit for bit, the blob map, the count
 * and the rows the single-image calls give that map.  Limits: height * width < 2^31 as above, and n * height * width, with the sides
 * rounded up to 32, < 2^32 pixels (ANH_ERR_INVALID beyond).
 * counts: n host values, blobs + 1 each.  The call synchronises the stream once. */
int anh_label_blobs_batch_device(anh_runtime* h, const uint16_t* d_labels, int n, int height, int width, uint32_t* d_blobs, uint32_t* counts);
/* *regions is ONE malloc'd block (release with anh_free): image 0's rows, then image 1's, ...; n_regions: n host values, n_regions[i] =
 * rows of image i; row.blob restarts at 1 per image.  d_blobs: NULL or [n][height][width].  Levels, `detected`, `peak`, apply_filter and
 * ANH_DET_SEED_REFERENCE_ORDER as anh_regions_device documents them; the filter zeroes the blobs without a seed in all n maps by one
 * launch.  The call waits on the host twice whatever n is: for the counts (the host sums them into the images' row offsets) and for the
 * table.  Everything but the table is reserved before the first kernel; the table once the counts are known, and if that fails the call
 * returns ANH_ERR_OOM and the handle stays usable. */
int anh_regions_batch_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int n, int classes, int height, int width,
                             const double* detection_levels, int apply_filter, uint32_t* d_blobs /* NULL or [n][H][W] */,
                             anh_region** regions, size_t* n_regions /* n host values */);
/* anh_infer_batch plus the region tables of its UNFILTERED label maps, by ONE batched regions call per share.  results[i], blobs[i],
 * blended_out[i] and image i's rows equal, bit for bit, what anh_infer_regions returns for image i alone.  blobs / blended_out: NULL, or
 * n pointers of which each may be NULL.  *regions: ONE malloc'd block, image 0's rows first; n_regions: n host values.  On a handle with
 * R replicas replica r serves the images anh_shard_range(n, R, r) and the host concatenates the shares' tables in image order; n < R
 * goes image by image on replica 0, as anh_infer_regions does. */
int anh_infer_regions_batch(anh_runtime* h, const uint8_t* const* images_hwc, int n, int height, int width,
                            const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                            uint16_t* const* results, uint32_t* const* blobs, float* const* blended_out, anh_region** regions, size_t* n_regions);
/* anh_infer_scaled plus the region table: table and blob map belong to the map at the net's resolution (anh_scaled_dims), where the
 * reference runs its filter; the result map is blown up afterwards.  What comes back equals anh_infer_regions of the shrunk image (and
 * the nearest-neighbour blow-up of its map); labels and planes equal anh_infer_scaled's.  Factor 1.0 is exactly anh_infer_regions.
 * scaled_labels, blobs, blended_out: optional (NULL), at the net's resolution. */
int anh_infer_regions_scaled(anh_runtime* h, const uint8_t* image_hwc, int height, int width, double downscaling_factor,
                             const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                             uint16_t* result_labels, uint16_t* scaled_labels, uint32_t* blobs, float* blended_out, anh_region** regions, size_t* n_regions);
/* anh_infer_scaled_batch plus the region tables: one batched shrink, the forward batches, ONE batched regions call at the net's
 * resolution, one batched blow-up.  Image i equals anh_infer_regions_scaled of image i alone; scaled_labels / blobs / blended_out: NULL,
 * or n pointers of which each may be NULL.  Factor 1.0 is exactly anh_infer_regions_batch.  Replicas as for anh_infer_regions_batch. */
int anh_infer_regions_scaled_batch(anh_runtime* h, const uint8_t* const* images_hwc, int n, int height, int width, double downscaling_factor,
                                   const double* gains, const double* detection_levels, const anh_tiling_params* tiling,
                                   uint16_t* const* results, uint16_t* const* scaled_labels, uint32_t* const* blobs, float* const* blended_out,
                                   anh_region** regions, size_t* n_regions);
/* ---- scoring result maps against their ground truth: the two confusion matrices of the inference program (annonet_infer_main.cpp:482-491
 * per pixel, :202-272 per region, two-way) on the device ----
 * truth and result are u16 label maps of one size, `classes` = K.  A pixel is LABELLED where truth < K (ANH_LABEL_IGNORE is not); a
 * prediction >= K (65535: an all-NaN pixel) casts no vote.
 *   labelled        the number of labelled pixels
 *   per_pixel[t][p] the number of labelled pixels with truth == t and result == p < K
 *   per_region      for each map M of (truth, result): M's regions are its blobs (anh_label_blobs_device: 8-connected, equal non-zero
 *                   value, 65535 a value like any other) plus region 0 = all pixels where M == 0.  With T[c] / P[c] the number of the
 *                   region's labelled pixels whose truth / result (< K) is c: no vote where T is all zero; t = first index of max(T);
 *                   where t != 0 and P is not "background only" (P[0] > 0, nothing else) P[0] counts as 0; no vote where P is all zero;
 *                   else per_region[t][first index of max(P)] += 1.  Ties go to the smaller class.
 * One batched labelling of the 2n maps, one tally pass over the pixels, one launch over the regions: the number of launches does not
 * depend on n, all sums are integer atomics (the same bits on every run), and image i of a batch equals the single call on that pair
 * bit for bit.  The calls run on the handle's stream (replica 0 of a handle with several) and wait on the host twice whatever n is: for
 * the blob counts, which size the vote table, and for the matrices.  Everything but the vote table is reserved before the first
 * kernel; the table once the counts are known, and if that fails the call returns ANH_ERR_OOM and the handle stays usable.
 * ANH_ERR_INVALID before anything is enqueued: classes outside 1..65535, n < 1, empty maps, height * width >= 2^31, 2n maps beyond the
 * batched labeller's limit (2 * n * height * width, sides rounded up to 32, < 2^32 pixels), a NULL map.  `classes` need not be the net's.
 * Counts of n >= 1 pairs of maps of ONE size; all outputs are OVERWRITTEN and are per image: per_pixel, per_region [n][classes][classes]
 * u64, first index ground truth; labelled [n] u64 (any output may be NULL).  d_truth, d_result: [n][height][width], resident. */
int anh_score_batch_device(anh_runtime* h, const uint16_t* d_truth, const uint16_t* d_result, int n, int classes, int height, int width,
                           uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled);
/* n = 1 */
int anh_score_device(anh_runtime* h, const uint16_t* d_truth, const uint16_t* d_result, int classes, int height, int width,
                     uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled);
/* host maps (n pointers each), uploaded at 2 bytes per pixel and map */
int anh_score_batch(anh_runtime* h, const uint16_t* const* truth, const uint16_t* const* result, int n, int classes, int height, int width,
                    uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled);
/* n = 1, host maps */
int anh_score(anh_runtime* h, const uint16_t* truth, const uint16_t* result, int classes, int height, int width,
              uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled);
/* ---- held-out evaluation: the loss the trainer optimises and the confusion counts of the inference program's argmax, from the logits
 * of an inference-mode forward (bn folded from the running statistics), per window ("image") ----
 * For every pixel with logits z[0..K), label y and weight w:
 *   predicted     find_label (annonet_infer.cpp:170-185) on z with the gains: the first class with the strictly largest
 *                 (float)((double)z + gain); 65535 when no class exceeds -inf (every logit NaN or -inf).  A predicted map, when asked for,
 *                 receives it for every pixel, labelled or not.
 *   y == ANH_LABEL_IGNORE: the pixel is skipped.  Another y >= K: the call returns ANH_ERR_INVALID and its outputs are unspecified.
 *   counted       += 1; where predicted == 65535: unclassified += 1 and nothing else; otherwise
 *   confusion[y][predicted] += 1, weight_sum += w, loss_sum += w * (-log max(softmax(z)[y], 1e-10)) — the term of
 *                 loss_multiclass_log_per_pixel_weighted as the training step computes it (float max, expf, float sum, z / sum, logf;
 *                 product and accumulation in double), without the gains.
 * So the sum of an image's confusion matrix plus unclassified equals counted; mean loss = sum loss_sum / sum weight_sum, pixel accuracy =
 * trace / sum counted.  Pixels where some but not all logits are NaN are unspecified.
 * All outputs are per image and OVERWRITTEN: per_image [n]; confusion [n][K][K] u64 (first index ground truth) or NULL; d_predicted /
 * predicted [n][H][W] u16 or NULL.  gains: K host doubles or NULL.  weights NULL = 1 everywhere.  K <= 64 (the net's limit).
 * The counts are integer atomics; the double sums are fixed-order sums of per-workgroup partials, and how an image is cut into workgroups
 * depends on its size alone: image i of any call equals the call on that image alone bit for bit, on every run, wherever its maps lie.
 * The calls run on the handle's stream (replica 0 of a handle with several) and wait on the host once, for the results.  Everything a
 * call needs is reserved before its first kernel: one that does not fit returns ANH_ERR_OOM and leaves the handle usable. */
typedef struct { double loss_sum, weight_sum; uint64_t counted, unclassified; } anh_eval_image;
/* the tally alone, on resident logits [n][classes][height][width] fp32 (what anh_runtime_forward_device writes), d_labels [n][H][W] u16,
 * d_weights [n][H][W] fp32 or NULL; `classes` need not be the net's */
int anh_eval_logits_device(anh_runtime* h, const float* d_logits, const uint16_t* d_labels, const float* d_weights, int n, int classes, int height, int width,
                           const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted);
/* n windows of one size, d_images [n][H][W][C] resident (the sizes anh_runtime_forward_device accepts): cut into forward batches no larger
 * than an inference tile batch, each followed by the tally on its logits; image i does not depend on the cut */
int anh_runtime_evaluate_device(anh_runtime* h, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights, int n, int height, int width,
                                const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted);
/* host samples as anh_trainer_step takes them: images[i] height*width*channels u8, labels[i] height*width weighted labels */
int anh_runtime_evaluate(anh_runtime* h, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width,
                         const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* predicted);
/* label rows [row0, row1) of device-resident blended planes (find_label, annonet_infer.cpp:170-185): the second half of a
   sharded annonet_infer(), run after the ranks have exchanged the plane sums of their overlapping tiles */
int anh_argmax_device(anh_runtime* h, const float* d_blended, int height, int width, int row0, int row1, const double* gains, uint16_t* d_result);
/* A handle launches on ONE stream (its own, non-blocking, unless set).  NULL returns the handle to a stream of its own — it does
   NOT mean the legacy default stream.  A host that mixes its own GPU work with the handle's (torch.distributed's all-reduce of the
   gradient bucket, torch kernels on the blended planes) takes the handle's stream with _get_stream and enqueues that work on it. */
int anh_runtime_set_stream(anh_runtime* h, void* hip_stream);
int anh_runtime_get_stream(anh_runtime* h, void** hip_stream);
/* bf16 inference has two forms: when every layer runs on a persistent MFMA kernel, each layer stores its post-activation output
 * relu(bn(y)) (one rounding of the fp32 accumulator); otherwise layers store the raw conv output and consumers re-apply bn + relu.
 * *yes = the form of the handle's LAST inference pass (parity tests pick the matching CPU restatement; ANH_INFER_POST_ACT=0 forces
 * the second form). */
int anh_runtime_stores_activations(anh_runtime* h, int* yes);
/* parity tap: the tensor bn layer `layer` stored in the handle's LAST inference pass (replica 0), as fp32 NHWC; out = NULL asks for the
 * dimensions only.  Fails ("tensor not available") for a layer that pass did not store: the head, the layer whose epilogue ran the head,
 * every layer before the first pass.  Synchronises the handle's stream. */
int anh_runtime_layer_tensor(anh_runtime* h, int layer, float* out, int64_t capacity, int dims4[4]);
int anh_runtime_synchronize(anh_runtime* h);

/* ---- TrainingNet (annonet_train_main.cpp:396-410) ---- */
int anh_trainer_create(anh_trainer** out);                                      /* TrainingNet ctor */
void anh_trainer_destroy(anh_trainer* h);
int anh_trainer_set_net_width(anh_trainer* h, double scaler, int min_filters); /* SetNetWidth */
int anh_trainer_set_class_count(anh_trainer* h, size_t classes);               /* SetClassCount */
int anh_trainer_set_levels(anh_trainer* h, int levels);                        /* LEVEL_COUNT */
int anh_trainer_set_input_channels(anh_trainer* h, int channels);              /* GRAYSCALE_INPUT */
int anh_trainer_set_precision(anh_trainer* h, int precision);
int anh_trainer_set_seed(anh_trainer* h, uint64_t seed);
int anh_trainer_initialize(anh_trainer* h);                                    /* Initialize(): builds the net, random init */
int anh_trainer_set_learning_rate(anh_trainer* h, double lr);                  /* SetLearningRate */
int anh_trainer_set_learning_rate_shrink_factor(anh_trainer* h, double f);     /* SetLearningRateShrinkFactor */
int anh_trainer_set_iterations_without_progress_threshold(anh_trainer* h, unsigned long n);
int anh_trainer_set_previous_loss_values_dump_amount(anh_trainer* h, unsigned long n);
int anh_trainer_set_all_bn_running_stats_window_sizes(anh_trainer* h, unsigned long n);
int anh_trainer_set_synchronization_file(anh_trainer* h, const char* path, double seconds); /* SetSynchronizationFile */
int anh_trainer_be_verbose(anh_trainer* h);                                    /* BeVerbose */
int anh_trainer_set_sgd(anh_trainer* h, double weight_decay, double momentum); /* dlib sgd defaults 0.0005 / 0.9 */
double anh_trainer_get_learning_rate(const anh_trainer* h);                    /* GetLearningRate (annonet_train_main.cpp:570) */
double anh_trainer_get_last_loss(anh_trainer* h);                              /* synchronises */
unsigned long anh_trainer_get_step_count(const anh_trainer* h);
int anh_trainer_config(const anh_trainer* h, anh_net_config* out);
/* StartTraining(samples, labels) (annonet_train_main.cpp:609): one optimiser step; inputs are consumed (copied to
 * HBM) before this returns (annonet_train_main.cpp:585-586). images[i]: height*width*channels u8; labels[i]: height*width. */
int anh_trainer_step(anh_trainer* h, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width);
/* the same step on inputs resident in HBM, split so that data-parallel ranks can all-reduce the gradient
 * bucket in between: forward_backward -> (RCCL all-reduce of grad_buffer) -> apply_update.
 * loss_scale_n: the N of the loss scale 1/(N*nr*nc), i.e. the GLOBAL batch. */
int anh_trainer_forward_backward_device(anh_trainer* h, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights,
                                        int n, int height, int width, double loss_scale_n);
int anh_trainer_apply_update(anh_trainer* h, double grad_scale);
int anh_trainer_grad_buffer(anh_trainer* h, void** d_ptr, int64_t* count); /* flat fp32 gradients (+1 trailing slot: loss) */
int anh_trainer_get_params(anh_trainer* h, float* params, int64_t n_params, float* running, int64_t n_running);
int anh_trainer_set_params(anh_trainer* h, const float* params, int64_t n_params, const float* running, int64_t n_running);
int anh_trainer_get_grads(anh_trainer* h, float* grads_canonical, int64_t n_params);
int anh_trainer_replica_params(anh_trainer* h, int replica, float* params, int64_t n_params); /* anh_set_devices: every replica must hold the same weights */
int anh_trainer_get_momentum(anh_trainer* h, float* momentum, int64_t n_params);
int anh_trainer_set_momentum(anh_trainer* h, const float* momentum, int64_t n_params);
/* GetRuntimeNet() (annonet_train_main.cpp:558): independent by-value snapshot; quiesces the device first */
int anh_trainer_snapshot_runtime(anh_trainer* h, int precision, anh_runtime** out);
/* Held-out evaluation in the middle of a training run (see anh_runtime_evaluate): the parameters and running statistics as they stand
 * after the last step issued — a step in flight finishes first — go into an inference net of `precision` that the handle keeps for
 * this purpose (made on first use on the trainer's first device, like a snapshot, and refreshed on every call), which evaluates the
 * samples.  The result equals anh_trainer_snapshot_runtime followed by anh_runtime_evaluate / _evaluate_device, bit for bit.  Nothing of
 * the training state is touched: parameters, momentum, running statistics and their update counts, step count, the losses in flight and
 * the learning-rate history, the accumulator tables, the step's streams and events.  On a handle with several replicas the evaluation
 * runs on replica 0's device only.  The _device form takes pointers resident on that device. */
int anh_trainer_evaluate(anh_trainer* h, int precision, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width,
                         const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* predicted);
int anh_trainer_evaluate_device(anh_trainer* h, int precision, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights, int n, int height,
                                int width, const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted);
int anh_trainer_save_state(anh_trainer* h, const char* path); /* trainer synchronization file */
int anh_trainer_load_state(anh_trainer* h, const char* path);
int anh_trainer_set_stream(anh_trainer* h, void* hip_stream);
int anh_trainer_get_stream(anh_trainer* h, void** hip_stream);
/* Overlapping the gradient all-reduce with the end of backward (data-parallel hosts; annonet_train_main.cpp:583-614 hands the
 * mini-batch to dlib's multi-GPU trainer, whose averaging this replaces): after forward_backward the bucket elements
 * [*first, n_params + 1) — every layer but the first two, the head and the loss slot — become final while the last
 * backward-data convs still run.  wait_early_grads makes `hip_stream` (a stream of the caller's) wait for exactly that point;
 * the elements [0, *first) are final when the handle's own stream has drained.  *first > n_params: no early part. */
int anh_trainer_early_grads(anh_trainer* h, int64_t* first);
/* ANH_STEP_GRAPH=1 (off by default): the launches of a training step behind the fused head — bn backward passes, backward-data convs and,
 * on the second stream, the filter gradients with their hand-over events — are captured once per (shape, buffers, input pointer) and
 * replayed with one hipGraphLaunch per StartTraining (/root/reference/annonet_train_main.cpp:609).  captures / launches: how often
 * replica 0 of the handle instantiated / replayed a graph (0 / 0 when the switch is off or the profiler is on). */
int anh_trainer_step_graph_stats(anh_trainer* h, int64_t* captures, int64_t* launches);
int anh_trainer_wait_early_grads(anh_trainer* h, void* hip_stream);
int anh_trainer_synchronize(anh_trainer* h);
/* debugging / parity taps: raw conv output (which=0) or gradient w.r.t. the layer's activation (which=1), as fp32 NHWC */
int anh_trainer_layer_tensor(anh_trainer* h, int layer, int which, float* out, int64_t capacity, int dims4[4]);

/* ---- per-kernel timing (HIP events on the handle's stream), for bench.py's roofline line ---- */
int anh_profile_enable(void* handle, int is_trainer, int enable);
int anh_profile_set_filter(void* handle, int is_trainer, const char* substring); /* NULL or "" = time every kernel */
int anh_profile_set_sampling(void* handle, int is_trainer, int every);         /* time every n-th forward(+backward) pass only */
int anh_profile_reset(void* handle, int is_trainer);
int anh_profile_count(void* handle, int is_trainer);
int anh_profile_entry(void* handle, int is_trainer, int index, char* name, size_t name_cap,
                      double* total_ms, int64_t* launches, double* flops, double* bytes);
/* entry names of the most recent pass (forward [+ backward + update]) in host enqueue order, one per kernel-class launch,
 * newline-separated; *needed = bytes incl. the terminator.  tools/pmc_traffic.py maps rocprofv3 dispatches onto entries with it. */
int anh_profile_launch_order(void* handle, int is_trainer, char* buf, size_t cap, size_t* needed);

/* ---- single-layer ops on host tensors (kernel-level parity tests and micro-benchmarks) ----
 * The same kernels the net runs, on caller-provided data.  Tensors are fp32 NHWC on the host; in ANH_BF16 they are
 * rounded to bf16 on upload and the result is rounded to bf16 storage before it comes back (filter gradients stay fp32).
 * An input is a producer's raw conv output plus its folded batch-norm: value = relu(x*scale+shift); scale == NULL means
 * "use x as it is".  A second input, when given, is added (skip connection). */
typedef struct { int type, k, stride, pad, cin, cout; } anh_conv_desc; /* type 0 = con, 1 = cont */
typedef struct { const float* x; const float* scale; const float* shift; } anh_op_input;
int anh_op_conv_forward(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                        const float* filters_canonical, const float* bias, float* y_nhwc, int* used_mfma);
int anh_op_conv_backward_data(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy_nhwc,
                              const float* filters_canonical, float* dx_nhwc, int* used_mfma);
int anh_op_conv_backward_filter(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                                const float* dy_nhwc, float* dw_canonical, int* used_mfma);
/* The same ops with the epilogues / prologues the training step fuses into them (kernel-level parity tests):
 *  _forward_stats      also returns the batch-norm statistics of the STORED output: sums[2*cout] = per channel (sum y, sum y*y);
 *                      *fused = 1 when the conv kernel produced them itself (else the separate statistics kernel ran).
 *  _backward_data_bn   dx (+= dx_init when given: the skip-gradient accumulation) and the bn + relu backward sums of the layer
 *                      that receives dx: y_prev = its raw output, (scale, shift, mean, invstd)[cin];
 *                      sums[2*cin] = per channel (sum dz*xhat, sum dz), dz = (y*scale+shift > 0) ? dx : 0, xhat = (y-mean)*invstd.
 *  bn_dy               describes a gradient that is not materialised: dy = coef0*(dz - coef1 - xhat*coef2) from (da, y) */
typedef struct { const float* da; const float* y; const float* scale; const float* shift; const float* mean; const float* invstd; const float* coef; } anh_op_bn_dy;
int anh_op_conv_forward_stats(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const anh_op_input* a, const anh_op_input* b,
                              const float* filters_canonical, float* y_nhwc, double* sums, int* fused);
int anh_op_conv_backward_data_bn(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy_nhwc,
                                 const float* filters_canonical, const float* dx_init, const float* y_prev, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, float* dx_nhwc, double* sums, int* fused);
int anh_op_conv_backward_filter_bn(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const uint8_t* image_u8,
                                   const anh_op_bn_dy* dy, float* dw_canonical, int* computed_dy_in_kernel);

/* ---- the batch-norm accumulator-table forms ("table mode", the default of the bf16 training step) and the training kernels that are
 * not convolutions, one at a time on host tensors (tests/test_gpu_train_ops.py).  A table is built on the host from per-channel sums
 * (each split into its two words and spread unevenly over every replica of the table) and decoded on the host the same way.
 *
 * anh_op_bn_layer   one bn layer of c channels over `pixels` values per channel.  In: sums[2*c] = per channel (sum y, sum y*y) where a
 *                   table is built from them (each must be a multiple of 2^-60 below 3e16), gamma, beta, eps, and the running statistics
 *                   (in / out; NULL = no running update) with their averaging factor and unbias factor.  Out: mean, invstd, scale, shift [c]
 *                   and the biased variance var[c]. */
typedef struct {
    int c; double pixels; float eps; double af, unbias;
    const double* sums; const float* gamma; const float* beta;
    float* running_mean; float* running_var;
    float* mean; float* invstd; float* scale; float* shift; double* var;
} anh_op_bn_layer;
/* ONE launch of the fold kernel over n_jobs <= 16 layers, each from its own table */
int anh_op_bn_fold(anh_op_bn_layer* jobs, int n_jobs, uint64_t spread_seed);
/* the partials form of the same arrays: statistics kernel over y[pixels][c] + finalize; sums_out[2*c] = the totals of its partials */
int anh_op_bn_forward_stats(int precision, const float* y, anh_op_bn_layer* layer, double* sums_out);

/* An input of a table-mode consumer: the producer's raw output x plus EITHER its folded (scale, shift) OR (sums != NULL) its sums,
 * gamma, beta and eps — a table is built from them and the kernel folds (scale, shift) in its prologue (pixels = those of x). */
typedef struct { const float* x; const float* scale; const float* shift; const double* sums; const float* gamma; const float* beta; float eps; } anh_op_bn_input;
/* anh_op_conv_forward_stats with the forms the engine's table mode uses.  image_u8 != NULL: the stem, reading a u8 NHWC image (a, b NULL).
 * tables = 0: per-workgroup partials (as anh_op_conv_forward_stats; requires the conv kernel to fuse them); tables = 1: the kernel adds into
 * a zeroed table; sums[2*cout] = the decoded totals, *poison / *ticket = the table's two control words, *workgroups = the launch's. */
int anh_op_conv_forward_stats_table(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const uint8_t* image_u8,
                                    const anh_op_bn_input* a, const anh_op_bn_input* b, const float* filters_canonical, int tables,
                                    float* y_nhwc, double* sums, int64_t* poison, int64_t* ticket, int* workgroups);
/* anh_op_conv_backward_data_bn with the sums added to a zeroed table and folded by the launch's last workgroup: dgamma[cin], dbeta[cin],
 * coef[3*cin] = [gamma*invstd | sum dz / P | sum dz*xhat / P] (prefilled with NaN), *ticket = the table's counter afterwards. */
int anh_op_conv_backward_data_bn_table(int precision, const anh_conv_desc* d, int n, int h_in, int w_in, const float* dy_nhwc,
                                       const float* filters_canonical, const float* dx_init, const float* y_prev, const float* scale,
                                       const float* shift, const float* mean, const float* invstd, const float* gamma, float* dx_nhwc,
                                       double* sums, float* dgamma, float* dbeta, float* coef, int64_t* ticket, int* workgroups);

/* bn + relu backward of one layer on (da, y)[pixels][c]: stages & 1 = reduce, & 2 = finalize, & 4 = apply.  tables = 1: the reduce adds
 * into a zeroed table and its last workgroup is the finish (no finalize kernel; vector widths only).  Without stage 2 the apply reads
 * coef_in[3*c].  Head form (head_g[pixels][head_k], head_w_tm[32][head_k], da NULL, stage 4 only): da is recomputed from the head's dlogits.
 * out_of_place: dy goes to its own buffer instead of over da.  Out: sums[2*c] = (sum dz*xhat, sum dz), dgamma, dbeta [c], coef[3*c]
 * (NaN where no stage wrote them), dy[pixels][c], *ticket (tables), *workgroups of the reduce. */
typedef struct {
    int c, head_k; int64_t pixels;
    const float* da; const float* y; const float* gamma; const float* mean; const float* invstd; const float* scale; const float* shift;
    const float* head_g; const float* head_w_tm; const float* coef_in;
    int tables, out_of_place, stages;
    double* sums; float* dgamma; float* dbeta; float* coef; float* dy;
    int64_t ticket; int workgroups;
} anh_op_bn_bwd;
int anh_op_bn_backward(int precision, anh_op_bn_bwd* op);

/* The fused tail of a training step (1x1 head on 32 channels, k <= 4 classes: logits, weighted softmax log-loss, head backward-data,
 * filter and bias gradient) in one launch.  a (and b: skip sum) as anh_op_bn_input; w_tm[32][k]; labels (ANH_LABEL_IGNORE = none).
 * da_virtual: da is not stored, dlogits is.  bn_sums: 0 none, 1 per-workgroup partials, 2 table + finish (needs a in table form) — the
 * bn + relu backward sums of a's layer (single input only), with bn_mean / bn_invstd (partials form) and bn_gamma (finish).
 * fold_jobs: bn layers whose fold rides in the launch's first workgroups.  Out: logits, dlogits [pixels][k], da[pixels][32], loss,
 * dbias[k], dw[32][k], bn_sums_out[64] = (sum dz*xhat, sum dz), dgamma, dbeta [32], coef[96] (NaN unless the finish ran), error_flag. */
typedef struct {
    int k; int64_t pixels; double scale;
    const anh_op_bn_input* a; const anh_op_bn_input* b;
    const float* w_tm; const float* bias; const uint16_t* labels; const float* weights;
    int da_virtual, bn_sums;
    const float* bn_mean; const float* bn_invstd; const float* bn_gamma;
    anh_op_bn_layer* fold_jobs; int n_fold_jobs;
    float* logits; float* dlogits; float* da; double* loss; float* dbias; float* dw;
    double* bn_sums_out; float* dgamma; float* dbeta; float* coef;
    int error_flag; int64_t ticket; int workgroups;
} anh_op_head;
int anh_op_head_train(int precision, anh_op_head* op);
/* the unfused loss kernel on fp32 logits[pixels][k], k <= 64 */
int anh_op_loss(const float* logits, const uint16_t* labels, const float* weights, int64_t pixels, int k, double scale,
                float* dlogits, double* loss, float* dbias, int* error_flag);

/* ---- host logic ---- */
/* tiling::get_tiles(width, height, params) (annonet_infer.cpp:42): *tiles is malloc'd, release with anh_free */
int anh_get_tiles(int width, int height, const anh_tiling_params* params, anh_tile** tiles, size_t* count);
/* the rectangles (inclusive, clipped to the image) in which tiles owned by different replicas overlap when the tile list is split
   into `world` contiguous chunks: the pixels whose plane sums the replicas exchange.  *rects is malloc'd, release with anh_free */
int anh_cross_replica_overlaps(const anh_tile* tiles, size_t n_tiles, int world, int width, int height, anh_rect** rects, size_t* count);
/* set_weights() (annonet_train.h:20-83) */
int anh_set_weights(const uint16_t* labels, int nr, int nc, double class_weight, double image_weight, anh_wlabel* out);
/* random_rect_containing_point() (annonet_train.h:85-105); the two 32-bit draws of dlib::rand are passed in */
int anh_random_rect_containing_point(uint32_t draw_x, uint32_t draw_y, long px, long py, long width, long height, anh_rect* out);
/* outpaint() (annonet.h:74-120), in place on a u8 image with `channels` interleaved channels */
int anh_outpaint(uint8_t* image, int nr, int nc, int channels, const anh_rect* inside);
/* ---- training crops cut on the device ----
   The reference cuts every training crop on the CPU (randomly_crop_image, annonet_train_main.cpp:110-232, in loader threads)
   and hands StartTraining host matrices.  Here the full images of the dataset live in HBM (288 GB) and a mini-batch of
   crops is produced there: extract_image_chip at scale 1 + outpaint (= clamp-to-edge crop, :160-176), labels set to
   "ignore" outside the image (:150-158), set_weights (:178), flips (:183-194) and the multiplicative brightness change
   (:196-216), for further_downscaling_factor = 1.  The random draws stay with the caller (dlib::rand is the host's): a
   crop is described by its rectangle (random_rect_containing_point), the two flip decisions and the brightness factor.
   Further downscaling, add_random_noise and apply_random_color_offset are covered with the host's draws passed in (see anh_crop_spec);
   dlib's own routines are absent from the snapshot, so their arithmetic is restated [UPSTREAM-UNVERIFIED]. */
typedef struct anh_dataset anh_dataset;
typedef struct {
    int image; long left, top; int flip_left_right, flip_upside_down;
    double brightness_change;          /* multiplicative (:196-216); 1 = none */
    double further_downscaling_factor; /* :124-127,160-171: the rectangle is round(dim * factor) wide and is resized to dim (bilinear image,
                                          nearest-neighbour labels, dlib::resize_image's corner-aligned grid); 0 or 1 = none */
    int noise_level;                   /* add_random_noise (:73-105): uniform integer in [-level, level] per channel value; 0 = none.  The draws
                                          come from a counter-based generator keyed by (noise_seed, position), not from dlib::rand's sequence */
    uint64_t noise_seed;
    int color_offset[3];               /* apply_random_color_offset (:226-231): per-channel offsets drawn by the host (RGB nets); 0 = none */
} anh_crop_spec;
int anh_dataset_create(int channels, anh_dataset** out);
void anh_dataset_destroy(anh_dataset* d);
/* uploads one full image (u8, HWC, `channels` interleaved) and its label image (u16) and keeps them resident; *index = its number */
int anh_dataset_add(anh_dataset* d, const uint8_t* image_hwc, const uint16_t* labels, int height, int width, int* index);
/* frees the image with that index (after the crops in flight that read it): the index becomes invalid (a crop spec naming it is
   ANH_ERR_INVALID) and is handed out again by a later anh_dataset_add.  With anh_dataset_resident_bytes a host bounds the HBM the
   resident set may take (the reference bounds its decoded images by --cached-image-count, annonet_train_main.cpp:301,504-518). */
int anh_dataset_remove(anh_dataset* d, int index);
int anh_dataset_resident_bytes(const anh_dataset* d, uint64_t* bytes);
/* n crops of dim x dim into host arrays: images n*dim*dim*channels u8, weighted labels n*dim*dim (tests, non-resident hosts) */
int anh_dataset_crop_batch(anh_dataset* d, const anh_crop_spec* specs, int n, int dim, int classes, double class_weight, double image_weight,
                           uint8_t* images, anh_wlabel* labels);
/* StartTraining on n crops cut on the device: the mini-batch never exists on the host */
int anh_trainer_step_crops(anh_trainer* h, anh_dataset* d, const anh_crop_spec* specs, int n, int dim, double class_weight, double image_weight);
/* ---- dataset preparation and crop-centre sampling on the device (opt-in; the calls above keep their behaviour) ----
   What the reference does once per decoded image on the host — ignore_classes_to_ignore (annonet_train_main.cpp:414-424),
   ignore_large_nonzero_regions (:434-502) and the labelled-point lists of decode_rgba_label_image (annonet.cpp:41-58), kept only so that
   randomly_crop_image can take "the k-th labelled point of the j-th class" (annonet_train_main.cpp:121-131) — runs on the resident label
   image instead.  No point list exists: an index of 4 bytes per PRESENT class and 1024 pixels answers "the k-th pixel of class c in
   raster order", the order in which the reference pushes its points.
   anh_dataset_prepare, on the labels of image `index` as they stand, in place:
     1. labels equal to one of classes_to_ignore[0..n_ignore), n_ignore <= 64, become ANH_LABEL_IGNORE; info->ignored_by_class = pixels changed;
     2. unless all three limits are infinite: the blobs of kernels_blobs.hip (8-connected, equal non-zero label) with
        (double)area > by_area * rf^2, (double)width > by_width * rf or (double)height > by_height * rf (rf = receptive_field_side; the
        products in double, as anh_ignore_large_nonzero_regions forms them; strict; infinity = that test off) become ANH_LABEL_IGNORE;
        info->ignored_by_size = pixels changed that were not ANH_LABEL_IGNORE before — the map and the count anh_ignore_large_nonzero_regions gives;
     3. the index: a label >= 64 that is not ANH_LABEL_IGNORE is ANH_ERR_INVALID (the crop path's own limit) and leaves the image
        unprepared; info->classes[0..present) = the class values present, ASCENDING, counts[i] = pixels of classes[i].
   A call that fails after its first launch (such a label, the blob labeller's limits, ANH_ERR_OOM for the region table or the index) may
   already have applied one or both filters to the resident labels: they are rewritten in place, and the image is left unprepared.
   The call waits for the dataset's stream before it touches the labels (as anh_dataset_remove does) and again before it returns.  It may be
   called again (the filters then see the labels as they stand; the index is rebuilt).  The index, 4 * present * ceil(height * width / 1024)
   bytes, is added to anh_dataset_resident_bytes; anh_dataset_remove subtracts it.
   Scratch of the dataset, reused by every call and reserved before the first launch: 0.25 bytes per pixel for the index; with a finite
   limit another 8 bytes per pixel (union-find parents and the blob map, 4 each), also reserved before the first launch, plus a region
   table of 56 bytes per blob, reserved once the labelling's blob count is back (the labelling does not need it), before the size filter
   has changed anything.  All limits infinite: no blob scratch is reserved.  anh_dataset_scratch_bytes: the bytes of this scratch the
   dataset holds at the moment (it only grows). */
typedef struct { int64_t ignored_by_class, ignored_by_size; int present; uint16_t classes[64]; uint64_t counts[64]; } anh_dataset_info;
/* classes[0..present) ascending, counts[i] = labelled pixels of classes[i] after both filters; present == 0: nothing to draw from */
int anh_dataset_prepare(anh_dataset* d, int index, const uint16_t* classes_to_ignore, int n_ignore,
                        double by_area, double by_width, double by_height, int receptive_field_side, anh_dataset_info* info);
int anh_dataset_scratch_bytes(const anh_dataset* d, uint64_t* bytes);
int anh_dataset_labels(anh_dataset* d, int index, uint16_t* labels);            /* the resident label image as it stands (tests, hosts that want it back) */
/* The random draws of a crop centre (annonet_train_main.cpp:121,131 and random_rect_containing_point), in the reference's order */
typedef struct { uint32_t class_draw; uint64_t point_draw; uint32_t rect_draw_x, rect_draw_y; } anh_crop_draw;
typedef struct { uint16_t label; int32_t x, y; long left, top; } anh_crop_pick;
/* label = classes[class_draw % present], k = point_draw % counts[that slot] (64-bit).  The class order is ascending class value, where the
   reference iterates an unordered_map (implementation-defined order): both are uniform over the present classes.  Host logic, no GPU;
   ANH_ERR_INVALID for present outside 1..64 or an empty class. */
int anh_resolve_pick(const anh_dataset_info* info, uint32_t class_draw, uint64_t point_draw, uint16_t* label, uint64_t* k);
/* out[i] = the k-th pixel (x, y) of the resolved class of image specs[i].image in raster order, and the corner of
   anh_random_rect_containing_point(rect_draw_x, rect_draw_y, x, y, side, side), side = round(dim * further_downscaling_factor).  The library
   resolves on the host from the info it kept at prepare time; the device receives (label, k, the two rect draws).  Waits for the result. */
int anh_dataset_pick(anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, anh_crop_pick* out);
/* anh_dataset_crop_batch / anh_trainer_step_crops with the rectangle picked on the device: specs[i].left / .top are ignored, everything else
   in a spec means what it means there; the picked corner goes straight into the crop kernel's argument and never visits the host (picks,
   when given, receives it all the same).  ANH_ERR_INVALID for an image that is not prepared or has present == 0. */
int anh_dataset_crop_batch_picked(anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, int classes,
                                  double class_weight, double image_weight, uint8_t* images, anh_wlabel* labels, anh_crop_pick* picks /* nullable */);
int anh_trainer_step_crops_picked(anh_trainer* h, anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim,
                                  double class_weight, double image_weight);

/* ignore_large_nonzero_regions (annonet_train_main.cpp:434-502), in place on a u16 label image: 8-connected blobs of equal
   non-zero, non-ignored label larger than by_area * rf^2 pixels, wider than by_width * rf or taller than by_height * rf
   become ANH_LABEL_IGNORE (infinity = that test off, as the CLI defaults :339-341).  *ignored = pixels relabelled. */
int anh_ignore_large_nonzero_regions(uint16_t* labels, int nr, int nc, double by_area, double by_width, double by_height,
                                     int receptive_field_side, int64_t* ignored);
/* annonet.dnn = dlib serialize framing of (string anno_classes_json, double downscaling_factor, string serialized RuntimeNet)
   (written annonet_train_main.cpp:557-565, read annonet_infer_main.cpp:340-351).  Both calls work on memory images of the
   file; returned buffers are released with anh_free.  The net blob is what anh_runtime_serialize / _deserialize exchange. */
int anh_dnn_envelope_pack(const char* classes_json, size_t json_size, double downscaling_factor, const void* net_blob, size_t net_size,
                          void** file, size_t* file_size);
int anh_dnn_envelope_unpack(const void* file, size_t file_size, char** classes_json, size_t* json_size, double* downscaling_factor,
                            void** net_blob, size_t* net_size);
/* dlib count_steps_without_decrease, used by the learning-rate schedule */
int64_t anh_count_steps_without_decrease(const double* values, int64_t n, double probability_of_decrease);

#ifdef __cplusplus
}
#endif
#endif /* ANNONET_HIP_H */
