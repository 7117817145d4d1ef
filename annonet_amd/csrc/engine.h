// engine.h — owns one net's device state on one GPU and sequences the kernels for
//   * RuntimeNet::Forward and annonet_infer()  (inference: bn folded to affine)
//   * TrainingNet::StartTraining               (forward, loss, backward, SGD)
// Everything is enqueued on one HIP stream; nothing synchronises unless the caller asks for host data.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "common.h"
#include "hostlogic.h"
#include "kernels.h"
#include "spec.h"

namespace anh {

// Per-kernel-class timing with HIP events on the engine's stream (bench.py's roofline line reads this).
class Profiler {
  public:
    struct Entry { std::string name; double total_ms = 0; int64_t launches = 0; double flops = 0, bytes = 0; };
    bool enabled = false;
    std::string filter;  // when non-empty only kernels whose name contains it are timed
    int sample_every = 1;  // time the kernels of every n-th pass only (an event pair costs ~6 us of stream time per launch)
    int64_t pass_index = 0; // advanced by the engine at the start of every forward pass
    // entry names of the most recent pass in host enqueue order, one per begin() (kept whether or not that launch is timed):
    // tools/pmc_traffic.py maps the dispatches of a rocprofv3 trace onto bench.py's per-layer entries with it
    std::vector<std::string> order;
    bool hold_order = false;   // inside annonet_infer(): `order` spans the whole image (every tile batch is a forward pass of its own)
    void start_pass() { ++pass_index; if (enabled && !hold_order) order.clear(); }
    void start_image() { if (enabled) order.clear(); hold_order = true; }
    ~Profiler();
    int begin(hipStream_t s, const char* name, double flops, double bytes);  // returns a token (or -1 when disabled)
    void end(hipStream_t s, int token);
    void collect();  // stream must be idle
    void reset();
    std::vector<Entry> entries;

  private:
    struct Pending { int entry; hipEvent_t start, stop; };
    std::vector<Pending> pending_;
    std::vector<hipEvent_t> pool_;
    hipEvent_t get_event();
};

struct LayerState {
    DevBuf raw;    // raw conv output y (storage dtype), [n][h][w][cout]
    DevBuf dact;   // gradient w.r.t. this layer's post-activation output; becomes dy in place on the unfused path
    DevBuf bn;     // mean, invstd, scale, shift (4*C floats) then var (C doubles)
    float* mean = nullptr; float* invstd = nullptr; float* scale = nullptr; float* shift = nullptr; double* var = nullptr;
    float* coef = nullptr;  // bn backward coefficients [3][C] of this layer (its own slot: two streams read them)
    int n = 0, h_in = 0, w_in = 0, h = 0, w = 0;
    bool dact_written = false;
    bool stored = false;   // inference: the last pass wrote `raw` at the planned dimensions (Engine::layer_tensor reads nothing else)
    const void* da_alias = nullptr;   // backward: da of this layer lives in ANOTHER layer's buffer (skip gradient written once); its apply pass reads it from there
    // backward bookkeeping: a layer's da is final once all its consumers' backward-data convs have written it; the conv
    // that writes it last may also leave the dgamma / dbeta partial sums (fused bn backward reduction)
    int consumers = 0, da_writes = 0, fused_bwd_blocks = 0;
    DevBuf bwd_partials;
    double running_updates = 0;  // dlib bn_: number of running-stat updates so far (capped by the window)
    long long* acc = nullptr;    // table mode (bnacc.h): this layer's accumulator table inside Engine::bn_acc
    double fold_af = 1.0, fold_unbias = 1.0; bool fold_running = false;   // this step's running-statistics update, applied by the fold job
};

class Engine {
  public:
    Engine(const anh_net_config& cfg, bool training);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    Spec spec;
    DType dtype;
    bool training;
    int device = 0;
    hipStream_t stream = nullptr;   // the engine's own (own_stream_), or one borrowed through set_stream
    // filter gradients run on a second stream, concurrently with the backward-data / bn chain (both only read dy)
    Stream aux_stream;
    Event ev_dy_ready, ev_aux_done;
    // Data-parallel hosts start the gradient all-reduce before backward has finished: the filter gradients come out last layer
    // first, so once layer kEarlyLayer's is reduced every gradient element from that layer's first parameter to the end of the
    // bucket (deeper layers, head, loss slot) is final.  ev_early_grads fires there (on the stream that ran that filter gradient).
    static constexpr int kEarlyLayer = 2;
    Event ev_early_grads;
    Stream early_stream;       // where the in-library exchange reduces the early part (anh_set_devices), made on first use
    Event ev_early_reduced;
    hipStream_t early_reduce_stream();
    int64_t early_grad_first() const;   // first bucket element covered by ev_early_grads; n_params + 1 when there is no early part
    bool concurrent_wgrad = true;
    Profiler prof;
    unsigned long bn_window = 100;           // SetAllBatchNormalizationRunningStatsWindowSizes
    bool update_running_in_forward = true;   // training forwards update the running statistics (dlib bn_ semantics)

    // ---- parameters ----
    void set_params(const float* params, const float* running);  // host canonical blobs
    void get_params(float* params, float* running);              // synchronises
    void get_grads_canonical(float* out);
    void get_momentum(float* out);
    void set_momentum(const float* in);
    std::vector<double> get_running_updates() const;   // dlib bn_ num_updates, one per bn layer (trainer state file)
    void set_running_updates(const std::vector<double>& v);
    void random_init(uint64_t seed);
    float* grad_bucket() { return grad.as<float>(); }  // n_params + 1 floats (last = loss)

    // ---- forward ----
    // image: SRC_IMAGE source (device u8).  Inference writes fp32 NCHW logits to d_out_nchw.
    void forward_inference(const Src& image, int n, int h, int w, float* d_out_nchw);
    void forward_training(const Src& image, int n, int h, int w);
    // ---- training ----
    void backward(const uint16_t* d_labels, const float* d_weights, double loss_scale_n);
    // loss_post / loss_tag: SgdArgs::loss_post (the update kernel posts the step's loss to that pinned host word), or null
    void apply_update(double lr, double weight_decay, double momentum, double grad_scale, unsigned long bn_window, unsigned long long* loss_post = nullptr, unsigned int loss_tag = 0);
    double read_loss();  // synchronises
    int read_error_flag_and_clear();
    // training net: raw conv output (which = 0) or the gradient w.r.t. the layer's activation (which = 1).  Inference net: which = 0 only, the
    // tensor a bn layer stored in the LAST pass; "tensor not available" for a layer that pass did not store (the layer under a head in the
    // epilogue, the head itself, any layer before the first pass or after the dimensions were planned anew).
    void layer_tensor(int layer, int which, float* out_host, int64_t capacity, int dims[4]);

    // ---- tiled inference: annonet_infer.cpp:42-214 with image, blended planes and labels resident in HBM ----
    int head_epi_layer = -1; float* head_epi_out = nullptr;   // set around the conv launches of one inference batch (infer_tiles)
    static constexpr int kMaxTileBatch = 16;   // Src::img_win holds 16 windows (4096^2 image, 25 tiles of 1024^2: batches of 8+8+8+1 / 7+6+6+6 / 9+8+8 / 13+12 / 25: 3,838 / 3,865 / 3,917 / 3,960 / 3,938 Mpx/s)
    void infer_tile(const anh_tile& t, const uint8_t* d_image, int H, int W, float* d_blended);
    void infer_tiles(const anh_tile* ts, int count, const uint8_t* d_image, int H, int W, float* d_blended);
    // A batch whose samples are (image, tile) pairs over images of one size: sample i is tile ts[i] of image images[i], which lives
    // image_stride bytes per index behind d_images and blends into the planes plane_stride floats per index behind d_blended.
    // images == nullptr: every sample is a tile of the one image at d_images (infer_tiles).  d_direct_labels: every sample is a whole image
    // (single tile, consecutive images) and the labels are taken straight from the batch's logits — no planes are written.
    void infer_samples(const anh_tile* const* ts, const int* images, int count, const uint8_t* d_images, int64_t image_stride, int H, int W,
                       float* d_blended, int64_t plane_stride, uint16_t* d_direct_labels = nullptr, const double* d_gains = nullptr);
    // whether a batch of `count` windows of h x w leaves its logits in memory (fp32 mode, the generic head, bf16 with the head in the
    // conv epilogue) rather than on chip (the fused head + blend kernel); reserves the batch's layer tensors and logits
    bool batch_logits_in_memory(int count, int h, int w);
    struct TailForm { bool fuse_head = false, head_epi = false; HeadBlendArgs hb; };
    TailForm plan_tail_form(const Src& image, int count, int h, int w);
    // annonet_infer() over n images of one size, resident as [n][H][W][C]: labels [n][H][W], planes [n][K][H][W] (d_blended may be null:
    // planes of the engine's own are used where the labels cannot come straight from the logits).  `tiles` is the complete tiling of one image.
    void infer_batch_device(const uint8_t* d_images, int n, int H, int W, const double* gains_host, const std::vector<anh_tile>& tiles,
                            uint16_t* d_labels, float* d_blended);
    // the reservations of infer_batch_device, on their own (nothing is enqueued); true = the labels come straight from the logits
    bool reserve_infer_batch(const std::vector<std::vector<TileSample>>& plan, int n, int H, int W, const std::vector<anh_tile>& tiles, bool planes_given);
    bool reserve_infer_batch(int n, int H, int W, const std::vector<anh_tile>& tiles, bool planes_given);
    void labels_from_logits(const float* d_logits, int count, int k, int win_h, int win_w, int top, int left, int H, int W, const double* d_gains, uint16_t* d_labels);
    DevBuf batch_planes;
    bool infer_post = false;   // this inference pass stores post-activation tensors (choose_inference_form)
    ConvArgs forward_conv_args(int li, const Src& image, bool training_pass, float* d_out_nchw) const;
    void choose_inference_form(const Src& image);
    int tile_batch(int h, int w) const;
    const double* upload_gains(const double* gains_host, int k = 0);   // -> device pointer (or nullptr); k doubles, 0 = the net's class count
    void argmax_rows(const float* d_blended, int H, int W, int row0, int row1, const double* gains_host, uint16_t* d_labels);   // find_label over rows [row0, row1)
    // whole_image: `tiles` is the image's COMPLETE tiling (then only the frames the blends accumulate into are cleared first)
    void infer_device(const uint8_t* d_image, int H, int W, const double* gains_host, const std::vector<anh_tile>& tiles,
                      uint16_t* d_labels, float* d_blended, bool whole_image = false);
    DevBuf zero_rects; int zero_rects_n = 0; uint64_t zero_rects_key = 0;   // the frames of the last whole-image tiling
    void prepare_zero_rects(int H, int W, const std::vector<anh_tile>& tiles);

    // ANH_STEP_GRAPH=1: the backward pass behind the head replayed as a captured HIP graph (Engine::backward)
    struct StepGraph { uint64_t key; int eager_runs; hipGraphExec_t exec; };
    std::vector<StepGraph> step_graphs;
    long step_graph_captures = 0, step_graph_launches = 0;
    static bool step_graph_enabled();
    void synchronize();
    bool bounded_waits = false;   // one of several replicas behind a handle: host waits take the deadline of common.h (wait_stream)
    void set_stream(hipStream_t s);

    // scratch exposed to the C ABI layer (host-pointer entry points stage through these)
    DevBuf stage_image, stage_labels, stage_weights, stage_out, stage_blended, stage_result;
    // downscaled inference (anh_infer_scaled): the image at its original size, and the label map blown back up to it.  Buffers of their
    // own: the inference pass in between reads stage_image and writes stage_blended / stage_result.
    DevBuf stage_original, stage_upsampled;
    // read_sample's resize + annonet_infer() + resize_label_image on resident buffers: d_original [H][W][C] -> d_scaled_image
    // [sh][sw][C] -> tiles -> d_scaled_labels [sh][sw] (and d_blended [K][sh][sw]) -> d_labels [H][W]
    void resize_image(const uint8_t* d_src, int src_h, int src_w, uint8_t* d_dst, int dst_h, int dst_w);
    void resize_labels(const uint16_t* d_src, int src_h, int src_w, uint16_t* d_dst, int dst_h, int dst_w);
    // ... over `count` images of one size, back to back, by one launch each
    void resize_image_batch(const uint8_t* d_src, int count, int src_h, int src_w, uint8_t* d_dst, int dst_h, int dst_w);
    void resize_labels_batch(const uint16_t* d_src, int count, int src_h, int src_w, uint16_t* d_dst, int dst_h, int dst_w);
    std::vector<float> host_out;

    // ---- connected blobs and the region table (kernels_blobs.hip; annonet_infer.cpp:194-223) ----
    // Everything works on n maps of one size lying back to back ([n][H][W], planes [n][K][H][W]) with launches that do not depend on n;
    // one map is a stack with n = 1.  `stacked` only names the profiler tags after the form the caller asked for: label_blobs /
    // blob_regions for a single-image entry point, label_blobs_batch / blob_regions_batch for a batch one.
    // Scratch of n maps with K detection levels: [parents | block sums | counts | row offsets | levels | seed flags]; own_map: blob maps of
    // the engine's own as well (the caller gives none).  Nothing is enqueued.
    struct BlobScratch { int* parent; unsigned* sums; unsigned* counts; unsigned long long* offsets; double* det; uint8_t* flags; };
    BlobScratch reserve_blobs(int n, int H, int W, int K, bool own_map);
    DevBuf blob_scratch, blob_map, blob_table;
    // d_blobs [n][H][W] = the blob numbers of d_labels, restarting at 1 per image; counts: n host values, blobs + 1 each.  Synchronises once.
    void label_blobs(const uint16_t* d_labels, int n, int H, int W, uint32_t* d_blobs, uint32_t* counts, bool stacked);
    // the table of d_labels' blobs as ONE malloc'd block (the caller owns it) with image 0's rows, then image 1's, ...; n_regions: n host
    // values; levels_host: K doubles or null; filter: relabel the blobs without a seed to 0 when a level is positive.  d_blobs may be null.
    // Returns the blob maps it used.  Synchronises twice whatever n is: for the counts (the host sums them into the row offsets) and for
    // the table.
    uint32_t* regions(uint16_t* d_labels, const float* d_blended, int n, int K, int H, int W, const double* levels_host, bool filter, uint32_t* d_blobs,
                      anh_region** out, size_t* n_regions, bool stacked);

    // ---- scoring result maps against their ground truth (kernels_score.hip; annonet_infer_main.cpp:482-491, RegionScorer) ----
    // Everything a score call of n pairs of H x W maps with K classes needs but the vote table, reserved before anything is enqueued.
    // Returns the stack [2n][H][W] the caller copies the maps into: the n truth maps, then the n result maps.
    uint16_t* reserve_score(int n, int K, int H, int W);
    DevBuf score_maps, score_votes, score_out;
    std::vector<uint64_t> host_score;   // score_out as it comes back
    // the counts of the stack reserve_score returned: per_pixel, per_region [n][K][K], labelled [n], host u64, each may be null.  ONE
    // labelling of the 2n maps, the tally, the decide launch.  Synchronises twice whatever n is: for the counts (they size the vote
    // table) and for the matrices.
    void score_stacked(int n, int K, int H, int W, uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled);

    // ---- held-out evaluation (kernels_eval.hip): loss sums and confusion counts per window ----
    // The tally on resident logits [n][K][H][W] with labels [n][H][W], weights [n][H][W] (or null = 1) and K gains (host, or null):
    // per_image [n] and confusion [n][K][K] (or null) on the host, d_predicted [n][H][W] (or null).  A label >= K other than
    // ANH_LABEL_IGNORE is ANH_ERR_INVALID.  Synchronises once.
    void evaluate_logits(const float* d_logits, const uint16_t* d_labels, const float* d_weights, int n, int K, int H, int W, const double* gains_host,
                         anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted);
    // n windows [n][H][W][C] of the net's own input: forward batches of at most tile_batch(H, W) windows, each followed by the tally on its
    // logits.  The logits and layer tensors of the largest batch, the partials, the outputs and the error flag are reserved before the
    // first kernel.  Synchronises once.
    void evaluate_device(const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights, int n, int H, int W, const double* gains_host,
                         anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted);
    DevBuf eval_partials, eval_out;
    std::vector<uint64_t> host_eval;   // eval_out as it comes back: [n images | n K K cells | error flag]

  private:
    void reserve_eval(int n, int batch, int K, int H, int W);
    void eval_begin(int n, int K);
    void eval_batch(const float* d_logits, const uint16_t* d_labels, const float* d_weights, int first, int count, int K, int H, int W, const double* d_gains,
                    uint16_t* d_predicted);
    void eval_finish(int n, int K, anh_eval_image* per_image, uint64_t* confusion);
    void plan_dims(int n, int h, int w);
    void plan_dims_unguarded(int n, int h, int w);
    // Table mode (bnacc.h, default in bf16 training when every layer's kernels support it; ANH_BN_TABLES=0 switches it off): the bn
    // sums of every layer are added to accumulator tables by the kernels that see the values and folded by their consumers, so the
    // 18 finalize launches of a step disappear from the critical stream.
    bool tables = false, fold_pending = false;
    bool tables_clean = false;   // the update kernel of the previous step cleared the tables (Engine::apply_update)
    DevBuf bn_acc;
    size_t bn_acc_bytes = 0;
    BnFoldJobs fold_jobs;
    bool choose_table_mode(const Src& image);
    BnTable table_of(int li) const;
    BnBwdFinish finish_of(int li);
    void build_fold_jobs();
    bool head_is_fused() const;
    Src layer_source(int li, const Src& image, bool fold_tables = false) const;
    void run_conv_forward(int li, const Src& image, bool training_pass, float* d_out_nchw);
    void refresh_compute_weights();
    void fold_running_stats();  // inference: scale/shift from running stats, computed on the host
    void ensure_training_buffers();
    void conv_dispatch(const ConvArgs& a, const char* tag, double flops, double bytes);
    void wgrad_dispatch(WgradArgs& a, const char* tag, double flops, double bytes, hipStream_t on, DevBuf& scratch);

    std::vector<LayerState> ls;
    std::vector<ParamSegment> segments_host;
    DevBuf segments;
    DevBuf master, momentum, grad, w_tm_f32, w_km_f32, w_tm_bf16, w_km_bf16, running;
    DevBuf bn_partials, wgrad_partials, wgrad_partials_main, loss_partials, coef, logits, dlogits, scalars, gains_dev, tile_out;
    double* loss_dev = nullptr;
    int* error_flag = nullptr;
    std::vector<float> host_params, host_running;  // mirror kept for inference folding / serialization
    Src last_image{};
    int last_n = 0, last_h = 0, last_w = 0;
    bool have_forward = false;
    Stream own_stream_;   // owns `stream`; empty while a borrowed one is in use
};

}  // namespace anh
