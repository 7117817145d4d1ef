// api.cpp — the C ABI (include/annonet_hip.h) over Engine.  Exceptions stop here: every entry point returns a
// status code and leaves the message in a thread-local string (anh_last_error).
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <unordered_set>

#include "common.h"
#include "engine.h"
#include "hostlogic.h"
#include "multidev.h"

using namespace anh;

namespace {
thread_local std::string g_error;

const char kRuntimeMagic[8] = {'A', 'N', 'H', 'R', 'T', '0', '0', '1'};
const char kStateMagic[8] = {'A', 'N', 'H', 'T', 'S', '0', '0', '2'};   // 002: + bn update counters, schedule counter, unrecorded losses

struct BlobHeader {
    char magic[8];
    int32_t levels, in_channels, classes, min_filters;
    double width_scaler;
    int64_t n_params, n_running;
};
}  // namespace

namespace anh {
void set_last_error(const std::string& message) { g_error = message; }

int replica_timeout_seconds() {
    static const int s = getenv("ANH_REPLICA_TIMEOUT_S") && atoi(getenv("ANH_REPLICA_TIMEOUT_S")) > 0 ? atoi(getenv("ANH_REPLICA_TIMEOUT_S")) : 180;
    return s;
}
namespace {
template <class Query>
void poll_until_done(Query&& query, const char* what) {
    hipError_t e = query();
    if (e == hipSuccess) return;   // the common case (the staging set of step k - 2): no clock read
    const auto t0 = std::chrono::steady_clock::now();
    const auto deadline = t0 + std::chrono::seconds(replica_timeout_seconds());
    for (int spins = 0; e == hipErrorNotReady; ++spins) {
        if (spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((spins & 63) == 63 && std::chrono::steady_clock::now() > deadline)
            fail(ANH_ERR_DEVICE, std::string(what) + ": the device did not finish within " + std::to_string(replica_timeout_seconds()) +
                                     " s (ANH_REPLICA_TIMEOUT_S) — a collective between the replicas of this handle did not complete");
        e = query();
    }
    HIP_CHECK(e);
}
}  // namespace
void wait_event(hipEvent_t ev, bool bounded) {
    if (!bounded) { HIP_CHECK(hipEventSynchronize(ev)); return; }
    poll_until_done([&] { return hipEventQuery(ev); }, "wait for an event");
}
void wait_stream(hipStream_t st, bool bounded) {
    if (!bounded) { HIP_CHECK(hipStreamSynchronize(st)); return; }
    poll_until_done([&] { return hipStreamQuery(st); }, "wait for a stream");
}
}  // namespace anh

struct anh_runtime {
    struct Exchange { DevBuf packed, rects, offsets; };
    std::vector<Exchange> exchange;       // per replica: scratch of the overlap exchange
    // `only_device` >= 0: ONE replica on that device whatever anh_set_devices named (a trainer's snapshot, below)
    void build(const anh_net_config& cfg, int only_device = -1) {
        reps.build(only_device >= 0 ? std::vector<int>(1, only_device) : selected_devices(), cfg, false, nullptr);
        exchange = std::vector<Exchange>(reps.size());
    }
    void set_params_all(const float* params, const float* running) {
        reps.for_all([&](size_t, Engine& e) { e.set_params(params, running); });
    }
    // host-buffer annonet_infer(): image strips go up and label strips come down through small pinned rings while the tiles
    // compute, so that neither transfer is exposed (anh_infer below)
    static constexpr int kRing = 3;
    struct Pinned { PinnedBuf mem; Event done; bool busy = false; };
    Pinned up[kRing], down[kRing];
    Stream copy_up, copy_down;
    std::vector<Event> strip_events;
    Event labels_ready;   // a strip of the label map is final on the compute stream
    // anh_set_devices: one process drives several GPUs.  Every replica holds the same weights; annonet_infer() shards its tile list
    // over them (infer_multi below).  The last member: the engines drain and die before anything above is released.
    ReplicaSet reps;
};

struct anh_trainer {
    anh_net_config cfg{2, 3, 3, 1.0, 1, ANH_BF16};
    uint64_t seed = 0;
    LrSchedule sched;
    double weight_decay = 0.0005, momentum = 0.9;
    unsigned long bn_window = 100;
    std::string sync_path;
    double sync_seconds = 0;
    std::chrono::steady_clock::time_point last_sync = std::chrono::steady_clock::now();
    bool verbose = false;
    unsigned long steps = 0;
    double last_loss = 0;
    // Losses travel back asynchronously (pinned slots + events) and enter the learning-rate schedule at a FIXED lag: the
    // update of step k first records the loss of step k - kLossLag (waiting for it if it has not arrived).  Which loss drives
    // which lr decision therefore does not depend on GPU / host timing: runs are reproducible and the ranks of a data-parallel
    // job (who all see the same all-reduced loss) shrink their rate at the same step.
    static constexpr unsigned long kLossLag = 4;
    // pinned ring of posted losses: the update kernel of step k stores (tag(k) << 32 | float bits) into slot k mod 256 (SgdArgs::loss_post)
    PinnedBuf loss_ring;
    unsigned long long* loss_ring_dev = nullptr;  // the same words as the device sees them
    static unsigned int loss_tag(unsigned long step) { return (unsigned int)(step & 0x7fffffffu) | 0x80000000u; }   // never the 0 of a fresh slot
    struct PendingLoss { int slot; unsigned long step; bool arrived; double value; };
    std::deque<PendingLoss> pending;   // step order; not yet recorded into the schedule
    int next_slot = 0;
    bool resume_pending = false;       // SetSynchronizationFile named a file: resume from it once the net structure is final
    // Host-buffer steps (StartTraining): two staging sets, each a pinned host block + a device block holding
    // [images | labels u16 | weights f32].  Step k packs into set k&1 while the GPU still runs step k-1, uploads it on a copy
    // stream and chains the compute behind the upload with events; the call returns once the inputs are packed
    // (annonet_train_main.cpp:585-586 refills samples/labels right after StartTraining returns).
    struct StageSet {
        PinnedBuf pinned;
        DevBuf dev;
        Event uploaded, consumed;   // H2D of this set done / the step that read it has finished
        bool in_flight = false;
        double wait_us = 0;   // how long the last call that packed into this set waited for the GPU to release it
    };
    // per replica, sized once when the handle is created (a set is never moved while its upload is in flight)
    std::vector<std::array<StageSet, 2>> stage;
    std::vector<Stream> copy_stream;
    unsigned long host_steps = 0;
    // what one StartTraining costs the host, and the exchange step on the device (anh_trainer_exchange_stats): host time of every call;
    // on every `xs_every`-th step an event pair around each part of the all-reduce on replica 0's streams (ANH_EXCHANGE_SAMPLE, default 8, 0 = never)
    struct ExchangeStats {
        int64_t calls = 0; double host_us_sum = 0, host_us_last = 0, wait_us_sum = 0;
        uint64_t worker_calls_base = 0;
        Event tail0, tail1, head0, head1;
        bool pending = false, split = false;
        int64_t samples = 0; double tail_us_sum = 0, head_us_sum = 0, tail_us_last = 0, head_us_last = 0;
    } xs;
    void collect_exchange_sample() {   // the pair of a sampled step, once that step has finished (blocks until then)
        if (!xs.pending) return;
        DeviceScope scope(reps.device_of(0));
        float ms = 0;
        HIP_CHECK(hipEventSynchronize(xs.head1.get()));
        HIP_CHECK(hipEventElapsedTime(&ms, xs.head0.get(), xs.head1.get()));
        xs.head_us_last = 1e3 * ms; xs.head_us_sum += xs.head_us_last;
        xs.tail_us_last = 0;
        if (xs.split) { HIP_CHECK(hipEventSynchronize(xs.tail1.get())); HIP_CHECK(hipEventElapsedTime(&ms, xs.tail0.get(), xs.tail1.get())); xs.tail_us_last = 1e3 * ms; xs.tail_us_sum += xs.tail_us_last; }
        ++xs.samples;
        xs.pending = false;
    }
    bool initialized = false, dirty = false;
    // The reference configures AFTER Initialize() (annonet_train_main.cpp:400-410: Initialize, SetNetWidth, ..., SetClassCount);
    // dlib allocates lazily, so the net is (re)built here on first use after a structural setting changed.
    Engine& engine() {
        if (!initialized) fail(ANH_ERR_INVALID, "TrainingNet::Initialize has not been called");
        if (!reps.built() || dirty) {
            if (steps > 0) fail(ANH_ERR_INVALID, "the net structure cannot change once training has started");
            reps.build(reps.devices, cfg, true, &seed);   // same seed: every replica starts from the same weights
            dirty = false;
        }
        if (resume_pending) {   // the reference names the file BEFORE SetClassCount (annonet_train_main.cpp:400-405): resume on first use
            std::ifstream probe(sync_path, std::ios::binary);
            // A file that exists but cannot be loaded (older format, another net, truncated) is an ERROR on every use of the net until the
            // caller removes it or names another: the flag is cleared only once the resume has succeeded, so no step can run — and the
            // periodic save can never overwrite a state the user still has — after a failed resume.
            if (probe.good()) { probe.close(); resume(); }
            resume_pending = false;
        }
        return reps.engine(0);
    }
    void resume();
    void structural_change() { if (steps > 0) fail(ANH_ERR_INVALID, "the net structure cannot change once training has started"); dirty = true; }
    void arrive(PendingLoss& p) {   // blocks until the loss of that step is on the host
        if (p.arrived) return;
        const volatile unsigned long long* word = loss_ring.as<unsigned long long>() + p.slot;
        const unsigned int want = loss_tag(p.step);
        unsigned long long w = *word;
        if ((unsigned int)(w >> 32) != want) {
            // not there yet: the stream is at most kLossLag steps behind.  Drain it (this also surfaces a device fault) and look again.
            { DeviceScope scope(reps.device_of(0)); reps.engine(0).synchronize(); }
            w = *word;
            if ((unsigned int)(w >> 32) != want) fail(ANH_ERR_INTERNAL, "the loss of a finished step was not posted");
        }
        const unsigned int bits = (unsigned int)(w & 0xffffffffu);
        float v;
        std::memcpy(&v, &bits, sizeof v);
        p.value = (double)v;
        p.arrived = true;
    }
    // records the losses of steps <= upto into the schedule, oldest first
    void record_until(unsigned long upto) {
        while (!pending.empty() && pending.front().step <= upto) {
            arrive(pending.front());
            sched.record(pending.front().value);
            pending.pop_front();
        }
    }
    // waits for every loss in flight (host queries: GetLastLoss, state file) WITHOUT recording any of them early
    void fetch_all() {
        for (auto& p : pending) arrive(p);
        if (!pending.empty()) last_loss = pending.back().value;
    }
    // anh_set_devices: data-parallel training from ONE process (annonet_train_main.cpp:583-614 stays as it is).  Replica r has its
    // own staging sets; StartTraining splits the mini-batch along N, one all-reduce (RCCL) sums the flat gradient buckets, every
    // replica applies the identical update.  Batch-norm statistics are per replica.  The last member: the engines
    // drain and die before the staging sets, the loss ring and the events above are released.
    // eval_net: the inference net of anh_trainer_evaluate, made on first use (one replica on the first device, like a snapshot) and
    // refreshed from the parameters on every call; it shares nothing with the training engines.
    std::unique_ptr<anh_runtime> eval_net;
    ReplicaSet reps;
};

// Full images of a dataset, resident in HBM, plus the scratch of the device crop path.
struct anh_dataset {
    int channels = 3;
    // prepared: anh_dataset_prepare has built the point index of the labels as they stand (index: one row of `blocks` words per present
    // class, in info.classes order — the class's pixel count in the blocks before each block)
    struct Item { DevBuf image, labels, index; int height = 0, width = 0; bool prepared = false; uint64_t index_bytes = 0; anh_dataset_info info{}; };
    std::vector<Item> items;          // a removed image leaves an empty slot (height 0) that a later add reuses
    std::vector<int> free_slots;
    uint64_t resident_bytes = 0;
    Stream stream;
    DevBuf d_specs, d_hist, d_first, d_table, d_bad, d_jobs, d_picks;
    DevBuf prep_counts, prep_words, blob_parent, blob_map, blob_sums, blob_table;   // scratch of anh_dataset_prepare
    PinnedBuf pinned;
    DevBuf out;   // outputs of the host-array form
    ~anh_dataset() { if (stream.get()) (void)hipStreamSynchronize(stream.get()); }
    Item& item(int index, const char* what) {
        if (!(index >= 0 && (size_t)index < items.size() && items[(size_t)index].height > 0)) fail(ANH_ERR_INVALID, std::string(what) + ": image index out of range (or removed)");
        return items[(size_t)index];
    }
    void drop_index(Item& it) { resident_bytes -= it.index_bytes; it.index.release(); it.index_bytes = 0; it.prepared = false; it.info = anh_dataset_info{}; }

    // What a crop batch stages in ONE pinned block: the kernel's specs, the histograms that come back, the weight tables that go up, the
    // two error words and, for picked crops, the pick jobs that go up and the picks that may come back.
    struct Staged {
        size_t spec_bytes, tab;
        CropSource* hs; unsigned* h_hist; unsigned* h_first; float* h_table; int* h_bad; DatasetPickJob* h_jobs; DatasetPick* h_picks;
    };
    // Validates the specs, fills and uploads the kernel's specs on `stream`.  draws != nullptr: the rectangle's corner does not come from
    // the spec: the host resolves (class, k) from the info kept at prepare time and ONE launch picks the pixel and writes the corner
    // into the uploaded specs.
    Staged stage_specs(const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim) {
        ANH_REQUIRE(specs && n >= 1 && dim >= 1 && dim <= 32768, "crop batch: bad argument");
        Staged g;
        g.spec_bytes = (size_t)n * sizeof(CropSource); g.tab = (size_t)n * kCropMaxClasses * 4;
        const size_t jobs_off = g.spec_bytes + 3 * g.tab + 64, picks_off = jobs_off + (size_t)n * sizeof(DatasetPickJob);
        const size_t need = draws ? picks_off + (size_t)n * sizeof(DatasetPick) : jobs_off;
        const hipStream_t st = stream.get();
        if (need > pinned.bytes) { HIP_CHECK(hipStreamSynchronize(st)); pinned.reserve(need); }
        d_specs.reserve(g.spec_bytes); d_hist.reserve(g.tab); d_first.reserve(g.tab); d_table.reserve(g.tab); d_bad.reserve(8);
        if (draws) { d_jobs.reserve((size_t)n * sizeof(DatasetPickJob)); d_picks.reserve((size_t)n * sizeof(DatasetPick)); }
        char* pin = pinned.as<char>();
        g.hs = reinterpret_cast<CropSource*>(pin);
        g.h_hist = reinterpret_cast<unsigned*>(pin + g.spec_bytes);
        g.h_first = reinterpret_cast<unsigned*>(pin + g.spec_bytes + g.tab);
        g.h_table = reinterpret_cast<float*>(pin + g.spec_bytes + 2 * g.tab);
        g.h_bad = reinterpret_cast<int*>(pin + g.spec_bytes + 3 * g.tab);
        g.h_jobs = reinterpret_cast<DatasetPickJob*>(pin + jobs_off);
        g.h_picks = reinterpret_cast<DatasetPick*>(pin + picks_off);
        for (int i = 0; i < n; ++i) {
            const anh_crop_spec& c = specs[i];
            ANH_REQUIRE(c.image >= 0 && (size_t)c.image < items.size() && items[(size_t)c.image].height > 0, "crop batch: image index out of range (or removed)");
            if (!draws) ANH_REQUIRE(c.left > -(1L << 30) && c.left < (1L << 30) && c.top > -(1L << 30) && c.top < (1L << 30), "crop batch: rectangle out of range");
            ANH_REQUIRE(c.brightness_change >= 0, "crop batch: negative brightness change");
            const Item& it = items[(size_t)c.image];
            ANH_REQUIRE(c.further_downscaling_factor == 0.0 || (c.further_downscaling_factor >= 1.0 && c.further_downscaling_factor <= 64.0), "crop batch: further downscaling factor must be >= 1");
            ANH_REQUIRE(c.noise_level >= 0 && c.noise_level <= 255, "crop batch: noise level must be 0..255");
            const double f = c.further_downscaling_factor == 0.0 ? 1.0 : c.further_downscaling_factor;
            const int src_dim = (int)std::round(dim * f);   // dim_before_downscaling (annonet_train_main.cpp:127)
            g.hs[i] = CropSource{it.image.as<uint8_t>(), it.labels.as<uint16_t>(), it.height, it.width, draws ? 0 : (int)c.left, draws ? 0 : (int)c.top,
                                 c.flip_left_right ? 1 : 0, c.flip_upside_down ? 1 : 0, c.brightness_change, src_dim, c.noise_level,
                                 (unsigned long long)c.noise_seed, {c.color_offset[0], c.color_offset[1], c.color_offset[2]}};
            if (draws) {
                ANH_REQUIRE(it.prepared && it.info.present >= 1, "picked crops: the image has not been prepared (anh_dataset_prepare) or has no labelled pixel");
                uint16_t label; uint64_t k;
                const int slot = resolve_pick(it.info, draws[i].class_draw, draws[i].point_draw, &label, &k);
                const size_t blocks = dataset_index_blocks((int64_t)it.height * it.width);
                g.h_jobs[i] = DatasetPickJob{it.labels.as<uint16_t>(), it.index.as<unsigned>() + (size_t)slot * blocks, (long long)it.height * it.width, it.width, (int)blocks,
                                             (unsigned)k, draws[i].rect_draw_x, draws[i].rect_draw_y, src_dim, label};
            }
        }
        HIP_CHECK(hipMemcpyAsync(d_specs.p, g.hs, g.spec_bytes, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_bad.p, 0, 8, st));
        if (draws) {
            HIP_CHECK(hipMemcpyAsync(d_jobs.p, g.h_jobs, (size_t)n * sizeof(DatasetPickJob), hipMemcpyHostToDevice, st));
            launch_dataset_pick(d_jobs.as<DatasetPickJob>(), n, d_specs.as<CropSource>(), d_picks.as<DatasetPick>(), d_bad.as<int>() + 1, st);
        }
        return g;
    }
    static void picks_to_host(const Staged& g, const DatasetPickJob* jobs, int n, anh_crop_pick* out) {
        for (int i = 0; i < n; ++i) out[i] = anh_crop_pick{jobs[i].label, g.h_picks[i].x, g.h_picks[i].y, (long)g.h_picks[i].left, (long)g.h_picks[i].top};
    }
    // Cuts n crops into device arrays on `stream`.  One host round trip inside: the per-crop label histograms come back,
    // set_weights' table is computed with the host's own arithmetic (bit-identical to set_weights on the crop) and goes up.
    // draws (nullable): see stage_specs; picks (nullable, with draws): the picked pixels and corners, which ride back with the histograms.
    void crop_batch(const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, int classes, double cw, double iw, uint8_t* d_images, uint16_t* d_labels,
                    float* d_weights, anh_crop_pick* picks) {
        ANH_REQUIRE(classes >= 1 && classes <= kCropMaxClasses, "crop batch: class count must be 1..64");
        const Staged g = stage_specs(specs, draws, n, dim);
        const hipStream_t st = stream.get();
        launch_crop_pixels(d_specs.as<CropSource>(), n, dim, channels, d_images, d_labels, d_hist.as<unsigned>(), d_first.as<unsigned>(), d_bad.as<int>(), classes, st);
        HIP_CHECK(hipMemcpyAsync(g.h_hist, d_hist.p, g.tab, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(g.h_first, d_first.p, g.tab, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(g.h_bad, d_bad.p, 8, hipMemcpyDeviceToHost, st));
        if (draws && picks) HIP_CHECK(hipMemcpyAsync(g.h_picks, d_picks.p, (size_t)n * sizeof(DatasetPick), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ANH_REQUIRE(g.h_bad[1] == 0, "picked crops: the point index does not match the resident labels");
        ANH_REQUIRE(g.h_bad[0] == 0, "label value exceeds the class count");
        if (draws && picks) picks_to_host(g, g.h_jobs, n, picks);
        for (int i = 0; i < n; ++i)
            set_weights_table(g.h_hist + (size_t)i * kCropMaxClasses, g.h_first + (size_t)i * kCropMaxClasses, kCropMaxClasses, (long long)dim * dim, cw, iw,
                              g.h_table + (size_t)i * kCropMaxClasses);
        HIP_CHECK(hipMemcpyAsync(d_table.p, g.h_table, g.tab, hipMemcpyHostToDevice, st));
        launch_crop_weights(d_labels, d_table.as<float>(), n, dim, d_weights, st);
    }
};

namespace {
// [images | labels u16 | weights f32] of n samples in ONE block (a staging set, the crops of a batch): each part starts on a 256-byte boundary
struct BatchLayout {
    size_t img_bytes, lab_off, w_off, total;
    BatchLayout(size_t n, size_t plane, int channels)
        : img_bytes(n * plane * channels), lab_off((img_bytes + 255) / 256 * 256), w_off((lab_off + n * plane * 2 + 255) / 256 * 256), total(w_off + n * plane * 4) {}
    uint16_t* labels(void* base) const { return reinterpret_cast<uint16_t*>(static_cast<char*>(base) + lab_off); }
    float* weights(void* base) const { return reinterpret_cast<float*>(static_cast<char*>(base) + w_off); }
};

bool detection_requested(const double* detection_levels, int K) {
    bool any = false;
    if (detection_levels) for (int k = 0; k < K; ++k) { ANH_REQUIRE(detection_levels[k] >= 0.0, "detection levels must be >= 0"); if (detection_levels[k] > 0.0) any = true; }
    return any;
}
// detection-level filter (annonet_infer.cpp:187-239), on resident planes [K][h][w] and their label map of h x w.
// Seeds are looked up at (row, col): the reference stores (r, c) but reads (point.y(), point.x()) — transposed (:210 vs :222); see DESIGN.md.
// Its scratch, e.stage_out of detection_scratch_bytes, is the caller's to reserve (with the rest, before its first kernel).
size_t detection_scratch_bytes(size_t plane, int K) { return plane + (size_t)K * sizeof(double) + 64; }   // flags, levels, the change counter
// Returns run_detection_filter's host rounds.
int apply_detection_levels(Engine& e, const double* levels, int K, int h, int w, const float* d_blended, uint16_t* d_labels) {
    const size_t plane = (size_t)h * w;
    uint8_t* flags = e.stage_out.as<uint8_t>();
    double* d_det = reinterpret_cast<double*>(flags + ((plane + 15) / 16) * 16);
    int* d_changed = reinterpret_cast<int*>(d_det + K);
    HIP_CHECK(hipMemcpyAsync(d_det, levels, (size_t)K * sizeof(double), hipMemcpyHostToDevice, e.stream));
    return run_detection_filter(d_blended, d_labels, K, h, w, d_det, flags, d_changed, e.stream);
}
// stage_image / stage_result for n images of `plane` pixels, and stage_blended for their class planes where a path blends into them
void reserve_stage(Engine& e, size_t n, size_t plane, bool planes = true) {
    e.stage_image.reserve(n * plane * e.spec.cfg.in_channels);
    if (planes) e.stage_blended.reserve(n * plane * e.spec.cfg.classes * 4);
    e.stage_result.reserve(n * plane * 2);
}
}  // namespace

extern "C" {

const char* anh_last_error(void) { return g_error.c_str(); }
void anh_free(void* p) { std::free(p); }

int anh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int anh_set_device(int device) {
    return guarded([&] { HIP_CHECK(hipSetDevice(device)); });
}
int anh_set_devices(const int* devices, int n) {
    return guarded([&] { select_devices(devices, n); if (n >= 1) HIP_CHECK(hipSetDevice(devices[0])); });
}
int anh_handle_replicas(void* handle, int is_trainer) {
    if (!handle) return 0;
    return (int)(is_trainer ? ((anh_trainer*)handle)->reps : ((anh_runtime*)handle)->reps).size();
}
int anh_host_register(void* p, size_t bytes) {
    return guarded([&] { ANH_REQUIRE(p && bytes, "host register: null block"); HIP_CHECK(hipHostRegister(p, bytes, hipHostRegisterDefault)); });
}
int anh_host_unregister(void* p) {
    return guarded([&] { ANH_REQUIRE(p, "host unregister: null block"); HIP_CHECK(hipHostUnregister(p)); });
}
int anh_labels_rect_to_host(const uint16_t* d_labels, uint16_t* h_labels, int width, int height, int left, int top, int right, int bottom, void* stream) {
    return guarded([&] {
        ANH_REQUIRE(d_labels && h_labels && width >= 1 && height >= 1, "labels to host: null map");
        ANH_REQUIRE(left >= 0 && top >= 0 && right < width && bottom < height && left <= right && top <= bottom, "labels to host: rectangle outside the map");
        const size_t off = (size_t)top * width + left;
        if (left == 0 && right == width - 1)   // whole rows: one contiguous block
            HIP_CHECK(hipMemcpyAsync(h_labels + off, d_labels + off, (size_t)(bottom - top + 1) * width * 2, hipMemcpyDeviceToHost, (hipStream_t)stream));
        else
            HIP_CHECK(hipMemcpy2DAsync(h_labels + off, (size_t)width * 2, d_labels + off, (size_t)width * 2, (size_t)(right - left + 1) * 2, (size_t)(bottom - top + 1),
                                       hipMemcpyDeviceToHost, (hipStream_t)stream));
    });
}
int anh_shard_range(int64_t n, int world, int rank, int64_t* lo, int64_t* hi) {
    return guarded([&] { ANH_REQUIRE(lo && hi && world >= 1 && rank >= 0 && rank < world && n >= 0, "shard range: bad argument"); shard_range(n, world, rank, *lo, *hi); });
}
int anh_cross_replica_overlaps(const anh_tile* tiles, size_t n_tiles, int world, int width, int height, anh_rect** rects, size_t* count) {
    return guarded([&] {
        ANH_REQUIRE((tiles || n_tiles == 0) && rects && count && world >= 1, "null argument");
        const std::vector<anh_rect> r = cross_replica_overlaps(std::vector<anh_tile>(tiles, tiles + n_tiles), world, width, height);
        anh_rect* out = (anh_rect*)std::malloc(std::max<size_t>(1, r.size()) * sizeof(anh_rect));
        if (!out) fail(ANH_ERR_OOM, "host allocation failed");
        std::copy(r.begin(), r.end(), out);
        *rects = out; *count = r.size();
    });
}

// ---- dimension maths / spec ----
int anh_required_input_dim(const anh_net_config* cfg) {
    int r = -1;
    guarded([&] { ANH_REQUIRE(cfg, "null config"); r = Spec::build(*cfg).required_input_dim(); });
    return r;
}
int anh_recommended_input_dim(int levels, int n) {
    if (levels < 0 || levels > 3) { g_error = "level count must be 0..3"; return -1; }
    return Spec::recommended_input_dim(levels, n);
}
int anh_net_layer_count(const anh_net_config* cfg) {
    int r = -1;
    guarded([&] { ANH_REQUIRE(cfg, "null config"); r = (int)Spec::build(*cfg).layers.size(); });
    return r;
}
int anh_net_layer(const anh_net_config* cfg, int index, anh_layer_desc* out) {
    return guarded([&] {
        ANH_REQUIRE(cfg && out, "null argument");
        Spec s = Spec::build(*cfg);
        ANH_REQUIRE(index >= 0 && index < (int)s.layers.size(), "layer index out of range");
        *out = s.layers[index];
    });
}
int64_t anh_net_param_count(const anh_net_config* cfg) {
    int64_t r = -1;
    guarded([&] { ANH_REQUIRE(cfg, "null config"); r = Spec::build(*cfg).n_params; });
    return r;
}
int64_t anh_net_running_count(const anh_net_config* cfg) {
    int64_t r = -1;
    guarded([&] { ANH_REQUIRE(cfg, "null config"); r = Spec::build(*cfg).n_running; });
    return r;
}

// ---- RuntimeNet ----
int anh_runtime_create(const anh_net_config* cfg, anh_runtime** out) {
    return guarded([&] {
        ANH_REQUIRE(cfg && out, "null argument");
        auto h = std::make_unique<anh_runtime>();
        h->build(*cfg);
        *out = h.release();
    });
}
void anh_runtime_destroy(anh_runtime* h) { delete h; }
int anh_runtime_config(const anh_runtime* h, anh_net_config* out) {
    return guarded([&] { ANH_REQUIRE(h && out, "null argument"); *out = h->reps.engine(0).spec.cfg; });
}
int anh_runtime_set_params(anh_runtime* h, const float* params, int64_t n_params, const float* running, int64_t n_running) {
    return guarded([&] {
        ANH_REQUIRE(h && params && running, "null argument");
        ANH_REQUIRE(n_params == h->reps.engine(0).spec.n_params && n_running == h->reps.engine(0).spec.n_running, "parameter blob size mismatch");
        h->set_params_all(params, running);
    });
}
int anh_runtime_get_params(const anh_runtime* h, float* params, int64_t n_params, float* running, int64_t n_running) {
    return guarded([&] {
        ANH_REQUIRE(h, "null handle");
        ANH_REQUIRE((!params || n_params == h->reps.engine(0).spec.n_params) && (!running || n_running == h->reps.engine(0).spec.n_running), "parameter blob size mismatch");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).get_params(params, running);
    });
}
int anh_runtime_serialize(const anh_runtime* h, void** blob, size_t* size) {
    return guarded([&] {
        ANH_REQUIRE(h && blob && size, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        const Spec& s = h->reps.engine(0).spec;
        const size_t bytes = sizeof(BlobHeader) + (size_t)(s.n_params + s.n_running) * 4;
        char* p = (char*)std::malloc(bytes);
        if (!p) fail(ANH_ERR_OOM, "host allocation failed");
        BlobHeader hd{};
        std::memcpy(hd.magic, kRuntimeMagic, 8);
        hd.levels = s.cfg.levels; hd.in_channels = s.cfg.in_channels; hd.classes = s.cfg.classes; hd.min_filters = s.cfg.min_filters;
        hd.width_scaler = s.cfg.width_scaler; hd.n_params = s.n_params; hd.n_running = s.n_running;
        std::memcpy(p, &hd, sizeof hd);
        try { h->reps.engine(0).get_params((float*)(p + sizeof hd), (float*)(p + sizeof hd) + s.n_params); }
        catch (...) { std::free(p); throw; }
        *blob = p; *size = bytes;
    });
}
int anh_runtime_deserialize(const void* blob, size_t size, int precision, anh_runtime** out) {
    return guarded([&] {
        ANH_REQUIRE(blob && out, "null argument");
        if (size < sizeof(BlobHeader)) fail(ANH_ERR_IO, "runtime blob truncated");
        BlobHeader hd;
        std::memcpy(&hd, blob, sizeof hd);
        if (std::memcmp(hd.magic, kRuntimeMagic, 8) != 0) fail(ANH_ERR_IO, "not an annonet_hip runtime blob");
        anh_net_config cfg{hd.levels, hd.in_channels, hd.classes, hd.width_scaler, hd.min_filters, precision};
        Spec s = Spec::build(cfg);
        if (s.n_params != hd.n_params || s.n_running != hd.n_running || size != sizeof hd + (size_t)(hd.n_params + hd.n_running) * 4)
            fail(ANH_ERR_IO, "runtime blob does not match its header");
        auto h = std::make_unique<anh_runtime>();
        h->build(cfg);
        const float* f = (const float*)((const char*)blob + sizeof hd);
        h->set_params_all(f, f + hd.n_params);
        *out = h.release();
    });
}

int anh_runtime_forward_device(anh_runtime* h, const uint8_t* d_image, int n, int height, int width, float* d_out_nchw) {
    return guarded([&] {
        ANH_REQUIRE(h && d_image && d_out_nchw, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        Engine& e = h->reps.engine(0);
        e.forward_inference(image_source(d_image, height, width, e.spec.cfg.in_channels), n, height, width, d_out_nchw);
    });
}

int anh_runtime_forward(anh_runtime* h, const uint8_t* image, int n, int height, int width, const float** out, int* k, int* nr, int* nc) {
    return guarded([&] {
        ANH_REQUIRE(h && image && out, "null argument");
        ANH_REQUIRE(n >= 1 && height >= 1 && width >= 1, "empty input");
        DeviceScope scope(h->reps.device_of(0));
        Engine& e = h->reps.engine(0);
        const int K = e.spec.cfg.classes, C = e.spec.cfg.in_channels;
        const size_t in_bytes = (size_t)n * height * width * C, out_elems = (size_t)n * K * height * width;
        e.stage_image.reserve(in_bytes);
        e.stage_out.reserve(out_elems * 4);
        HIP_CHECK(hipMemcpyAsync(e.stage_image.p, image, in_bytes, hipMemcpyHostToDevice, e.stream));
        e.forward_inference(image_source(e.stage_image.as<uint8_t>(), height, width, C), n, height, width, e.stage_out.as<float>());
        e.host_out.resize(out_elems);
        HIP_CHECK(hipMemcpyAsync(e.host_out.data(), e.stage_out.p, out_elems * 4, hipMemcpyDeviceToHost, e.stream));
        e.synchronize();
        *out = e.host_out.data();
        if (k) *k = K;
        if (nr) *nr = height;
        if (nc) *nc = width;
    });
}

static std::vector<anh_tile> tiles_for(const anh_tiling_params* tiling, int width, int height) {
    if (tiling) return make_tiles(width, height, *tiling);
    anh_tile t;
    t.full_rect = {0, 0, width - 1, height - 1};
    t.unique_rect = t.full_rect;
    return {t};
}

int anh_infer_device(anh_runtime* h, const uint8_t* d_image, int height, int width, const double* gains, const anh_tiling_params* tiling,
                     const anh_tile* tiles, size_t n_tiles, uint16_t* d_result, float* d_blended) {
    return guarded([&] {
        ANH_REQUIRE(h && d_image && d_blended, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        std::vector<anh_tile> list = tiles ? std::vector<anh_tile>(tiles, tiles + n_tiles) : tiles_for(tiling, width, height);
        bool whole = tiles == nullptr;
        if (tiles && tiling) {   // a one-rank job hands over its "share": the complete tiling
            const std::vector<anh_tile> all = tiles_for(tiling, width, height);
            whole = all.size() == list.size() && std::memcmp(all.data(), list.data(), all.size() * sizeof(anh_tile)) == 0;
        }
        h->reps.engine(0).infer_device(d_image, height, width, gains, list, d_result, d_blended, whole);
    });
}

int anh_argmax_device(anh_runtime* h, const float* d_blended, int height, int width, int row0, int row1, const double* gains, uint16_t* d_result) {
    return guarded([&] {
        ANH_REQUIRE(h && d_blended && d_result, "null argument");
        ANH_REQUIRE(height >= 1 && width >= 1 && row0 >= 0 && row0 <= row1 && row1 <= height, "argmax: bad row range");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).argmax_rows(d_blended, height, width, row0, row1, gains, d_result);
    });
}

namespace {
void ring_reserve(anh_runtime::Pinned& b, size_t bytes) { b.done.ensure(); b.mem.reserve(bytes); }

// The streamed form of annonet_infer() for host buffers: the image is uploaded in row strips (host memcpy into a pinned ring
// -> async DMA on a copy stream), a tile starts as soon as the rows of its window are resident, and the label rows that no
// later tile can touch are arg-maxed and sent back (pinned ring -> host memcpy) while the next tile row computes.
void infer_streamed(anh_runtime* h, const uint8_t* image, int H, int W, const double* gains, const std::vector<anh_tile>& tiles, uint16_t* result) {
    Engine& e = h->reps.engine(0);
    const int K = e.spec.cfg.classes, C = e.spec.cfg.in_channels;
    const size_t plane = (size_t)H * W, row_bytes = (size_t)W * C;
    if (!h->copy_up.get()) { h->copy_up.create(hipStreamNonBlocking); h->copy_down.create(hipStreamNonBlocking); }
    const hipStream_t copy_up = h->copy_up.get(), copy_down = h->copy_down.get();
    const hipEvent_t labels_ready = h->labels_ready.ensure();
    const int strip_rows = std::max(1, (int)std::min<size_t>((size_t)H, ((size_t)4 << 20) / std::max<size_t>(row_bytes, 1)));   // ~4 MiB strips
    const int n_strips = (H + strip_rows - 1) / strip_rows;
    while ((int)h->strip_events.size() < n_strips) h->strip_events.emplace_back().ensure();
    for (int i = 0; i < anh_runtime::kRing; ++i) { h->up[i].busy = false; h->down[i].busy = false; }
    uint8_t* d_image = e.stage_image.as<uint8_t>();
    float* d_blended = e.stage_blended.as<float>();
    uint16_t* d_labels = e.stage_result.as<uint16_t>();
    launch_fill_zero(d_blended, plane * K * 4, e.stream);
    const double* d_gains = e.upload_gains(gains);

    int uploaded = 0, next_strip = 0;
    auto upload_until = [&](int rows) {   // rows [0, rows) resident (as far as the copy stream is concerned)
        rows = std::min(rows, H);
        while (uploaded < rows) {
            anh_runtime::Pinned& b = h->up[next_strip % anh_runtime::kRing];
            const int r0 = uploaded, r1 = std::min(H, r0 + strip_rows);
            const size_t bytes = (size_t)(r1 - r0) * row_bytes;
            if (b.busy) HIP_CHECK(hipEventSynchronize(b.done.get()));
            ring_reserve(b, (size_t)strip_rows * row_bytes);
            std::memcpy(b.mem.p, image + (size_t)r0 * row_bytes, bytes);
            HIP_CHECK(hipMemcpyAsync(d_image + (size_t)r0 * row_bytes, b.mem.p, bytes, hipMemcpyHostToDevice, copy_up));
            HIP_CHECK(hipEventRecord(b.done.get(), copy_up));
            HIP_CHECK(hipEventRecord(h->strip_events[next_strip].get(), copy_up));
            b.busy = true;
            uploaded = r1; ++next_strip;
        }
    };
    struct Down { int slot, r0, r1; };
    std::vector<Down> pending;
    auto drain = [&](size_t keep) {       // copy finished label strips out of the pinned ring
        while (pending.size() > keep) {
            const Down d = pending.front();
            pending.erase(pending.begin());
            anh_runtime::Pinned& b = h->down[d.slot];
            HIP_CHECK(hipEventSynchronize(b.done.get()));
            std::memcpy(result + (size_t)d.r0 * W, b.mem.p, (size_t)(d.r1 - d.r0) * W * 2);
            b.busy = false;
        }
    };
    int labels_done = 0, down_slot = 0;
    const size_t max_down_rows = std::min<size_t>((size_t)H, std::max<size_t>(1, ((size_t)16 << 20) / ((size_t)W * 2)));   // label strips of <= 16 MiB
    auto send_labels = [&](int until) {   // rows [labels_done, until) are final on the compute stream
        while (labels_done < until) {
            const int r0 = labels_done, r1 = (int)std::min<size_t>((size_t)until, (size_t)r0 + max_down_rows);
            launch_argmax_range(d_blended, K, (int64_t)plane, (int64_t)r0 * W, (int64_t)r1 * W, d_gains, d_labels, e.stream);
            HIP_CHECK(hipEventRecord(labels_ready, e.stream));
            drain(anh_runtime::kRing - 1);
            anh_runtime::Pinned& b = h->down[down_slot];   // free: at most kRing - 1 strips are pending
            ring_reserve(b, max_down_rows * W * 2);
            HIP_CHECK(hipStreamWaitEvent(copy_down, labels_ready, 0));
            HIP_CHECK(hipMemcpyAsync(b.mem.p, d_labels + (size_t)r0 * W, (size_t)(r1 - r0) * W * 2, hipMemcpyDeviceToHost, copy_down));
            HIP_CHECK(hipEventRecord(b.done.get(), copy_down));
            b.busy = true;
            pending.push_back(Down{down_slot, r0, r1});
            down_slot = (down_slot + 1) % anh_runtime::kRing;
            labels_done = r1;
        }
    };
    // rows below final_after[i] receive nothing from the tiles after i
    std::vector<int> final_after(tiles.size());
    int lowest_top = H;
    for (size_t i = tiles.size(); i-- > 0;) { final_after[i] = std::min(lowest_top, H); lowest_top = std::min(lowest_top, (int)std::max(0l, (long)tiles[i].full_rect.top)); }
    auto rows_needed = [&](const TileWindow& w) { return std::min(H, std::max(1, w.top + w.height)); };   // clamp-to-edge reads reach row 0 / row H-1 at most
    for (size_t i = 0; i < tiles.size();) {
        // the tiles of one tile row (equal windows, same image rows) run as batches (Engine::infer_tiles)
        const TileWindow win = tile_window(tiles[i], e.spec.cfg.levels);
        const int need = rows_needed(win), limit = e.tile_batch(win.height, win.width);
        size_t j = i + 1;
        while (j < tiles.size() && j - i < (size_t)limit) {
            const TileWindow wj = tile_window(tiles[j], e.spec.cfg.levels);
            if (wj.height != win.height || wj.width != win.width || rows_needed(wj) != need) break;
            ++j;
        }
        upload_until(need);
        HIP_CHECK(hipStreamWaitEvent(e.stream, h->strip_events[(need - 1) / strip_rows].get(), 0));
        e.infer_tiles(&tiles[i], (int)(j - i), d_image, H, W, d_blended);
        upload_until(uploaded + strip_rows * (int)(j - i));   // stay a few strips ahead of the tiles: one more strip per tile enqueued
        if (final_after[j - 1] > labels_done) send_labels(final_after[j - 1]);
        i = j;
    }
    upload_until(H);        // an image larger than its tiles' windows cannot occur, but keep the invariant
    send_labels(H);
    drain(0);
    e.synchronize();
}
}  // namespace

namespace {
// ---- one host-buffer inference call ----
// What anh_infer, anh_infer_batch, anh_infer_scaled, anh_infer_scaled_batch and the four anh_infer_regions forms ask for, as ONE value: the entry
// points check their arguments and fill it, run_host_infer decides who serves it, run_share is the body that runs it.
struct HostInfer {
    enum class Tail { none, filter, regions };
    const uint8_t* const* images = nullptr;   // n images of H x W, as the caller holds them
    int n = 1, H = 0, W = 0;
    bool batch = false;        // a batch form: the forward is infer_batch_device (a single-image form keeps infer_device's launches, engine.hip)
    double factor = 1.0;       // 1.0: no resize; else the images are shrunk to h x w, the net's resolution, and the maps blown up again
    int h = 0, w = 0;
    const double* gains = nullptr;
    const double* levels = nullptr;
    std::vector<anh_tile> tiles;   // at the net's resolution
    uint16_t* const* results = nullptr;   // per image: the map of H x W, ...
    uint16_t* const* scaled = nullptr;    // ... the map of h x w and the planes [K][h][w]; either list and any entry may be null
    float* const* planes = nullptr;
    Tail tail = Tail::none;    // after the forward, at the net's resolution: the detection-level filter (some level is positive), or the region table
    uint32_t* const* blobs = nullptr;     // Tail::regions: per image the blob map of h x w (the list and any entry may be null), ...
    anh_region** regions = nullptr;       // ... ONE malloc'd table for the images a share serves, the first image's rows first, ...
    size_t* n_regions = nullptr;          // ... and per image the number of its rows

    bool resized() const { return factor != 1.0; }
    uint16_t* scaled_of(int i) const { return scaled ? scaled[i] : nullptr; }
    float* planes_of(int i) const { return planes ? planes[i] : nullptr; }
    uint32_t* blobs_of(int i) const { return blobs ? blobs[i] : nullptr; }
    HostInfer single(int i) const {   // image i of a batch as the single-image call
        HostInfer c = *this;
        c.images += i; c.results += i;
        if (scaled) c.scaled += i;
        if (planes) c.planes += i;
        if (blobs) c.blobs += i;
        if (n_regions) c.n_regions += i;
        c.n = 1; c.batch = false;
        return c;
    }
    // from an entry point's (checked) arguments; sh x sw: the net's resolution.  Negative detection levels are refused here, before anything is enqueued.
    HostInfer(anh_runtime* rt, const uint8_t* const* images, int n, bool batch, int H, int W, double factor, int sh, int sw, const double* gains, const double* levels,
              const anh_tiling_params* tiling, uint16_t* const* results, uint16_t* const* scaled, float* const* planes)
        : images(images), n(n), H(H), W(W), batch(batch), factor(factor), h(sh), w(sw), gains(gains), levels(levels), tiles(tiles_for(tiling, sw, sh)),
          results(results), scaled(scaled), planes(planes),
          tail(detection_requested(levels, rt->reps.engine(0).spec.cfg.classes) ? Tail::filter : Tail::none) {}
};

// A single image on a handle with several replicas (anh_set_devices): the tile list is split into contiguous row-major chunks
// (tiles are independent, annonet_infer.cpp:46-165, except for the additive blended_output), every replica blends its chunk
// into planes of its own, ONE all-reduce sums the planes inside the rectangles where tiles of different replicas overlap
// (strips one receptive field wide), every replica labels the rows its tiles cover, and the host label map is assembled tile
// by tile from the owner of each tile (in an overlap both owners hold the same sums, hence the same labels).
// A resized call: every replica uploads the original image and shrinks it itself (the shrunk image is integer-valued and identical
// everywhere); the map assembled on the host is the one at the net's resolution, and replica 0 blows it up.
void infer_multi(anh_runtime* h, const HostInfer& c) {
    const size_t R = h->reps.size();
    const int K = h->reps.engine(0).spec.cfg.classes, C = h->reps.engine(0).spec.cfg.in_channels;
    const int H = c.h, W = c.w;
    const size_t plane = (size_t)H * W, full = (size_t)c.H * c.W;
    const double* gains = c.gains;
    const std::vector<anh_tile>& tiles = c.tiles;
    float* blended_out = c.planes_of(0);
    std::vector<uint16_t> merged_own;
    uint16_t* result = !c.resized() ? c.results[0] : c.scaled_of(0);
    if (!result) { merged_own.resize(plane); result = merged_own.data(); }
    const RectTable table = make_rect_table(cross_replica_overlaps(tiles, (int)R, W, H));
    const int64_t total = table.total();
    std::vector<float*> packed(R, nullptr);
    std::vector<hipStream_t> streams(R);
    std::vector<int64_t> lo(R), hi(R);
    h->reps.each([&](size_t r, Engine& e) {
        shard_range((int64_t)tiles.size(), (int)R, (int)r, lo[r], hi[r]);
        reserve_stage(e, 1, plane);
        if (c.resized()) {
            e.stage_original.reserve(full * C);
            if (r == 0) e.stage_upsampled.reserve(full * 2);
            HIP_CHECK(hipMemcpyAsync(e.stage_original.p, c.images[0], full * C, hipMemcpyHostToDevice, e.stream));
            e.resize_image(e.stage_original.as<uint8_t>(), c.H, c.W, e.stage_image.as<uint8_t>(), H, W);
        } else
            HIP_CHECK(hipMemcpyAsync(e.stage_image.p, c.images[0], plane * C, hipMemcpyHostToDevice, e.stream));
        const std::vector<anh_tile> mine(tiles.begin() + lo[r], tiles.begin() + hi[r]);
        e.infer_device(e.stage_image.as<uint8_t>(), H, W, gains, mine, nullptr, e.stage_blended.as<float>());
        streams[r] = e.stream;
        if (total > 0) {
            anh_runtime::Exchange& x = h->exchange[r];
            x.packed.reserve((size_t)K * total * 4);
            x.rects.reserve(table.rects.size() * sizeof(anh_rect));
            x.offsets.reserve(table.offset.size() * sizeof(int64_t));
            HIP_CHECK(hipMemcpyAsync(x.rects.p, table.rects.data(), table.rects.size() * sizeof(anh_rect), hipMemcpyHostToDevice, e.stream));
            HIP_CHECK(hipMemcpyAsync(x.offsets.p, table.offset.data(), table.offset.size() * sizeof(int64_t), hipMemcpyHostToDevice, e.stream));
            launch_pack_rects(e.stage_blended.as<float>(), K, H, W, x.rects.as<anh_rect>(), x.offsets.as<int64_t>(), (int)table.rects.size(), total, x.packed.as<float>(), e.stream);
            packed[r] = x.packed.as<float>();
        }
    });
    // the table's host vectors must outlive the async uploads: every replica's stream passes the uploads before the collective returns control below
    if (total > 0) h->reps.coll->all_reduce_sum(packed, (size_t)K * total, streams);   // the ONE exchange step of the path
    h->reps.each([&](size_t r, Engine& e) {
        if (hi[r] == lo[r]) return;
        if (total > 0) {
            anh_runtime::Exchange& x = h->exchange[r];
            launch_unpack_rects(e.stage_blended.as<float>(), K, H, W, x.rects.as<anh_rect>(), x.offsets.as<int64_t>(), (int)table.rects.size(), total, x.packed.as<float>(), e.stream);
        }
        long top = H, bottom = -1;
        for (int64_t i = lo[r]; i < hi[r]; ++i) { top = std::min(top, tiles[(size_t)i].full_rect.top); bottom = std::max(bottom, tiles[(size_t)i].full_rect.bottom); }
        const int row0 = (int)std::max(0L, top), row1 = (int)std::min((long)H, bottom + 1);
        const double* d_gains = e.upload_gains(gains);
        launch_argmax_range(e.stage_blended.as<float>(), K, (int64_t)plane, (int64_t)row0 * W, (int64_t)row1 * W, d_gains, e.stage_result.as<uint16_t>(), e.stream);
        for (int64_t i = lo[r]; i < hi[r]; ++i) {   // this replica's share of the host label map (and planes): its tiles' full rectangles
            const anh_rect& f = tiles[(size_t)i].full_rect;
            const long l = std::max(0L, f.left), t = std::max(0L, f.top), rt = std::min((long)W - 1, f.right), b = std::min((long)H - 1, f.bottom);
            if (l > rt || t > b) continue;
            const size_t off = (size_t)t * W + l;
            HIP_CHECK(hipMemcpy2DAsync(result + off, (size_t)W * 2, e.stage_result.as<uint16_t>() + off, (size_t)W * 2, (size_t)(rt - l + 1) * 2, (size_t)(b - t + 1),
                                       hipMemcpyDeviceToHost, e.stream));
            if (blended_out)
                for (int k = 0; k < K; ++k)
                    HIP_CHECK(hipMemcpy2DAsync(blended_out + k * plane + off, (size_t)W * 4, e.stage_blended.as<float>() + k * plane + off, (size_t)W * 4,
                                               (size_t)(rt - l + 1) * 4, (size_t)(b - t + 1), hipMemcpyDeviceToHost, e.stream));
        }
    });
    h->reps.for_all([](size_t, Engine& e) { e.synchronize(); });
    if (!c.resized()) return;
    Engine& e = h->reps.engine(0);   // (the caller holds replica 0's device)
    HIP_CHECK(hipMemcpyAsync(e.stage_result.p, result, plane * 2, hipMemcpyHostToDevice, e.stream));
    e.resize_labels(e.stage_result.as<uint16_t>(), H, W, e.stage_upsampled.as<uint16_t>(), c.H, c.W);
    HIP_CHECK(hipMemcpyAsync(c.results[0], e.stage_upsampled.p, full * 2, hipMemcpyDeviceToHost, e.stream));
    e.synchronize();
}

// THE body of a host-buffer call: images [lo, hi) of `c` on one engine, under its device and on its stream.  Reserve everything the
// share uses (a share that cannot fit fails with ANH_ERR_OOM before its first kernel), upload, shrink, forward, tail, blow up,
// download, synchronise.
void run_share(Engine& e, const HostInfer& c, int lo, int hi) {
    using Tail = HostInfer::Tail;
    const int m = hi - lo, K = e.spec.cfg.classes, C = e.spec.cfg.in_channels;
    const size_t plane = (size_t)c.h * c.w, full = (size_t)c.H * c.W;
    bool planes = !c.batch || c.tail != Tail::none;   // infer_device blends into planes whoever wants them; both tails read them
    for (int i = lo; i < hi; ++i) planes = planes || c.planes_of(i) != nullptr;
    reserve_stage(e, (size_t)m, plane, planes);
    if (c.resized()) { e.stage_original.reserve((size_t)m * full * C); e.stage_upsampled.reserve((size_t)m * full * 2); }
    if (c.tail == Tail::filter) e.stage_out.reserve(detection_scratch_bytes(plane, K));
    if (c.tail == Tail::regions) (void)e.reserve_blobs(m, c.h, c.w, K, true);
    if (c.batch) e.reserve_infer_batch(m, c.h, c.w, c.tiles, planes);   // the forward's own, ahead of the shrink
    uint8_t* d_image = e.stage_image.as<uint8_t>();
    float* d_planes = planes ? e.stage_blended.as<float>() : nullptr;
    uint16_t* d_labels = e.stage_result.as<uint16_t>();
    const uint16_t* d_results = d_labels;   // the maps of H x W
    uint8_t* d_upload = c.resized() ? e.stage_original.as<uint8_t>() : d_image;
    for (int i = 0; i < m; ++i) HIP_CHECK(hipMemcpyAsync(d_upload + (size_t)i * full * C, c.images[lo + i], full * C, hipMemcpyHostToDevice, e.stream));
    if (c.resized()) e.resize_image_batch(d_upload, m, c.H, c.W, d_image, c.h, c.w);
    if (c.batch) e.infer_batch_device(d_image, m, c.h, c.w, c.gains, c.tiles, d_labels, d_planes);
    else e.infer_device(d_image, c.h, c.w, c.gains, c.tiles, d_labels, d_planes, /*whole_image=*/true);
    // the tails run at the net's resolution, as the reference runs its filter before resize_label_image
    std::unique_ptr<anh_region, decltype(&std::free)> table(nullptr, &std::free);
    const uint32_t* d_blobs = nullptr;
    if (c.tail == Tail::filter)
        for (int i = 0; i < m; ++i) (void)apply_detection_levels(e, c.levels, K, c.h, c.w, d_planes + (size_t)i * K * plane, d_labels + (size_t)i * plane);
    if (c.tail == Tail::regions) {   // ONE call for the share's m maps
        anh_region* t = nullptr;
        d_blobs = e.regions(d_labels, d_planes, m, K, c.h, c.w, c.levels, /*filter=*/true, nullptr, &t, c.n_regions + lo, /*stacked=*/c.batch);
        table.reset(t);
    }
    if (c.resized()) {
        e.resize_labels_batch(d_labels, m, c.h, c.w, e.stage_upsampled.as<uint16_t>(), c.H, c.W);
        d_results = e.stage_upsampled.as<uint16_t>();
    }
    for (int i = 0; i < m; ++i) {
        HIP_CHECK(hipMemcpyAsync(c.results[lo + i], d_results + (size_t)i * full, full * 2, hipMemcpyDeviceToHost, e.stream));
        if (c.resized() && c.scaled_of(lo + i)) HIP_CHECK(hipMemcpyAsync(c.scaled_of(lo + i), d_labels + (size_t)i * plane, plane * 2, hipMemcpyDeviceToHost, e.stream));
        if (d_blobs && c.blobs_of(lo + i)) HIP_CHECK(hipMemcpyAsync(c.blobs_of(lo + i), d_blobs + (size_t)i * plane, plane * 4, hipMemcpyDeviceToHost, e.stream));
        if (c.planes_of(lo + i)) HIP_CHECK(hipMemcpyAsync(c.planes_of(lo + i), d_planes + (size_t)i * K * plane, plane * K * 4, hipMemcpyDeviceToHost, e.stream));
    }
    e.synchronize();
    if (c.tail == Tail::regions) *c.regions = table.release();
}

// A single image, on replica 0 unless its tiles can be shared out.
void run_single(anh_runtime* h, const HostInfer& c) {
    DeviceScope scope(h->reps.device_of(0));
    Engine& e = h->reps.engine(0);
    // several replicas: shard the tile list (the filter and the region table walk connected blobs of the WHOLE label map: they run on
    // replica 0 alone, as does an image with fewer tiles than replicas would gain nothing)
    if (h->reps.size() > 1 && c.tail == HostInfer::Tail::none && c.tiles.size() >= 2) { infer_multi(h, c); return; }
    static const bool streamed = read_switch("ANH_INFER_STREAMED", true);
    if (streamed && !c.resized() && c.tail == HostInfer::Tail::none && !c.planes_of(0)) {
        reserve_stage(e, 1, (size_t)c.h * c.w);
        infer_streamed(h, c.images[0], c.h, c.w, c.gains, c.tiles, c.results[0]);
        return;
    }
    run_share(e, c, 0, 1);
}

// Who serves a host-buffer call.  A single-image form: run_single.  A batch form: every replica takes a contiguous share of the images
// (an image is computed wholly on one replica, so nothing is exchanged); fewer images than replicas are served image by image, as
// the single-image form serves them.  Factor 1.0 is exactly the unscaled call (the host's bilinear returns early at scale 1, nearest
// neighbour at equal size is the identity): the map at the net's resolution is then a copy of the result.
void run_host_infer(anh_runtime* h, const HostInfer& c) {
    const size_t R = h->reps.size();
    if (!c.batch) run_single(h, c);
    else {
        // the shares in image order: image by image, or replica r's anh_shard_range
        const bool by_image = (size_t)c.n < R;
        std::vector<std::pair<int, int>> range(by_image ? (size_t)c.n : R);
        for (size_t s = 0; s < range.size(); ++s) {
            int64_t lo = (int64_t)s, hi = (int64_t)s + 1;
            if (!by_image) shard_range((int64_t)c.n, (int)R, (int)s, lo, hi);
            range[s] = {(int)lo, (int)hi};
        }
        // the region table: every share returns a table of its own; the call's ONE block is their concatenation in image order
        const bool regions = c.tail == HostInfer::Tail::regions;
        std::vector<anh_region*> part(range.size(), nullptr);
        struct Release { std::vector<anh_region*>& p; ~Release() { for (anh_region* t : p) std::free(t); } } release{part};
        auto share = [&](HostInfer s, size_t slot) { if (regions) s.regions = &part[slot]; return s; };
        if (by_image) for (int i = 0; i < c.n; ++i) run_single(h, share(c.single(i), (size_t)i));
        else
            h->reps.each([&](size_t r, Engine& e) {
                if (range[r].second > range[r].first) run_share(e, share(c, r), range[r].first, range[r].second);
            });
        if (regions && part.size() == 1) { *c.regions = part[0]; part[0] = nullptr; }
        else if (regions) {
            size_t rows = 0;
            for (int i = 0; i < c.n; ++i) rows += c.n_regions[i];
            anh_region* all = static_cast<anh_region*>(std::malloc(std::max<size_t>(1, rows * sizeof(anh_region))));
            if (!all) fail(ANH_ERR_OOM, "host allocation of the region table failed");
            size_t at = 0;
            for (size_t s = 0; s < range.size(); ++s) {
                size_t mine = 0;
                for (int i = range[s].first; i < range[s].second; ++i) mine += c.n_regions[i];
                if (mine) std::memcpy(all + at, part[s], mine * sizeof(anh_region));
                at += mine;
            }
            *c.regions = all;
        }
    }
    if (!c.resized())
        for (int i = 0; i < c.n; ++i) if (c.scaled_of(i)) std::memcpy(c.scaled_of(i), c.results[i], (size_t)c.H * c.W * 2);
}
}  // namespace

int anh_infer(anh_runtime* h, const uint8_t* image, int height, int width, const double* gains, const double* detection_levels,
              const anh_tiling_params* tiling, uint16_t* result, float* blended_out) {
    return guarded([&] {
        ANH_REQUIRE(h && image && result, "null argument");
        ANH_REQUIRE(height >= 1 && width >= 1, "empty image");
        run_host_infer(h, HostInfer(h, &image, 1, false, height, width, 1.0, height, width, gains, detection_levels, tiling, &result, nullptr, &blended_out));
    });
}

// ---- connected blobs and the region table (Engine::label_blobs / regions): a single-image entry point is the batch one with n = 1, behind
// its own size check ----
namespace {
void require_blob_map_size(int height, int width) {
    ANH_REQUIRE(height >= 1 && width >= 1, "empty label map");
    ANH_REQUIRE((int64_t)height * width < ((int64_t)1 << 31), "blob labelling is limited to height * width < 2^31 pixels");
}
void require_blob_batch_size(int n, int height, int width) {
    ANH_REQUIRE(n >= 1, "the batch needs at least one image");
    require_blob_map_size(height, width);
    ANH_REQUIRE(blob_batch_fits(n, height, width), "blob labelling of a batch is limited to n * height * width (sides rounded up to 32) < 2^32 pixels");
}
// what the entry points of either form do after their size check (first: a size beyond the limit is refused whatever else is wrong)
void label_blobs_device(anh_runtime* h, const uint16_t* d_labels, int n, bool batch, int height, int width, uint32_t* d_blobs, uint32_t* counts) {
    ANH_REQUIRE(h && d_labels && d_blobs && counts, "null argument");
    DeviceScope scope(h->reps.device_of(0));
    h->reps.engine(0).label_blobs(d_labels, n, height, width, d_blobs, counts, batch);
}
void regions_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int n, bool batch, int classes, int height, int width, const double* detection_levels,
                    int apply_filter, uint32_t* d_blobs, anh_region** regions, size_t* n_regions) {
    ANH_REQUIRE(classes >= 1 && classes <= 65535, "regions: the class count must be within 1..65535");
    if (detection_levels) for (int k = 0; k < classes; ++k) ANH_REQUIRE(detection_levels[k] >= 0.0, "detection levels must be >= 0");
    ANH_REQUIRE(h && d_labels && d_blended && regions && n_regions, "null argument");
    DeviceScope scope(h->reps.device_of(0));
    (void)h->reps.engine(0).regions(d_labels, d_blended, n, classes, height, width, detection_levels, apply_filter != 0, d_blobs, regions, n_regions, batch);
}
// what the four host-buffer forms share: the regions tail on a checked HostInfer
void run_regions(anh_runtime* h, HostInfer c, uint32_t* const* blobs, anh_region** regions, size_t* n_regions) {
    c.tail = HostInfer::Tail::regions;
    c.blobs = blobs; c.regions = regions; c.n_regions = n_regions;
    run_host_infer(h, c);
}
}  // namespace

int anh_label_blobs_device(anh_runtime* h, const uint16_t* d_labels, int height, int width, uint32_t* d_blobs, uint32_t* count) {
    return guarded([&] {
        require_blob_map_size(height, width);
        label_blobs_device(h, d_labels, 1, false, height, width, d_blobs, count);
    });
}

int anh_regions_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int classes, int height, int width, const double* detection_levels,
                       int apply_filter, uint32_t* d_blobs, anh_region** regions, size_t* n_regions) {
    return guarded([&] {
        require_blob_map_size(height, width);
        regions_device(h, d_labels, d_blended, 1, false, classes, height, width, detection_levels, apply_filter, d_blobs, regions, n_regions);
    });
}

// the detection-level filter of anh_infer alone, on a resident map: Tail::filter's rule and its apply_detection_levels
int anh_detection_filter_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int classes, int height, int width, const double* detection_levels,
                                int* rounds) {
    return guarded([&] {
        ANH_REQUIRE(h && d_labels && d_blended, "null argument");
        ANH_REQUIRE(classes >= 1 && classes <= 65535, "detection filter: the class count must be within 1..65535");
        ANH_REQUIRE(height >= 1 && width >= 1, "empty label map");
        if (rounds) *rounds = 0;
        if (!detection_requested(detection_levels, classes)) return;   // no positive level: nothing is ever removed
        DeviceScope scope(h->reps.device_of(0));
        Engine& e = h->reps.engine(0);
        e.stage_out.reserve(detection_scratch_bytes((size_t)height * width, classes));
        const int made = apply_detection_levels(e, detection_levels, classes, height, width, d_blended, d_labels);
        e.synchronize();   // the apply launch: the map is final when the call returns
        if (rounds) *rounds = made;
    });
}

int anh_infer_regions(anh_runtime* h, const uint8_t* image, int height, int width, const double* gains, const double* detection_levels,
                      const anh_tiling_params* tiling, uint16_t* result, uint32_t* blobs, float* blended_out, anh_region** regions, size_t* n_regions) {
    return guarded([&] {
        require_blob_map_size(height, width);
        ANH_REQUIRE(h && image && result && regions && n_regions, "null argument");
        // the blobs are those of the WHOLE label map: replica 0 alone, as anh_infer's filter
        run_regions(h, HostInfer(h, &image, 1, false, height, width, 1.0, height, width, gains, detection_levels, tiling, &result, nullptr, &blended_out), &blobs, regions,
                    n_regions);
    });
}

int anh_label_blobs_batch_device(anh_runtime* h, const uint16_t* d_labels, int n, int height, int width, uint32_t* d_blobs, uint32_t* counts) {
    return guarded([&] {
        require_blob_batch_size(n, height, width);
        label_blobs_device(h, d_labels, n, true, height, width, d_blobs, counts);
    });
}

int anh_regions_batch_device(anh_runtime* h, uint16_t* d_labels, const float* d_blended, int n, int classes, int height, int width, const double* detection_levels,
                             int apply_filter, uint32_t* d_blobs, anh_region** regions, size_t* n_regions) {
    return guarded([&] {
        require_blob_batch_size(n, height, width);
        regions_device(h, d_labels, d_blended, n, true, classes, height, width, detection_levels, apply_filter, d_blobs, regions, n_regions);
    });
}

int anh_infer_regions_batch(anh_runtime* h, const uint8_t* const* images, int n, int height, int width, const double* gains, const double* detection_levels,
                            const anh_tiling_params* tiling, uint16_t* const* results, uint32_t* const* blobs, float* const* blended_out, anh_region** regions,
                            size_t* n_regions) {
    return guarded([&] {
        require_blob_batch_size(n, height, width);
        ANH_REQUIRE(images && results, "infer_batch: null image or result list");
        ANH_REQUIRE(h && regions && n_regions, "null argument");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && results[i], "infer_batch: null image or result");
        run_regions(h, HostInfer(h, images, n, true, height, width, 1.0, height, width, gains, detection_levels, tiling, results, nullptr, blended_out), blobs, regions,
                    n_regions);
    });
}

// ---- scoring result maps against their ground truth (Engine::score_stacked) ----
namespace {
void require_score_sizes(int n, int classes, int height, int width) {
    ANH_REQUIRE(n >= 1, "score: the batch needs at least one image");
    ANH_REQUIRE(classes >= 1 && classes <= 65535, "score: the class count must be within 1..65535");
    require_blob_map_size(height, width);
    // truth and result maps are labelled together, as one stack of 2n maps
    ANH_REQUIRE(n < (1 << 30) && blob_batch_fits(2 * n, height, width), "scoring a batch is limited to 2 * n * height * width (sides rounded up to 32) < 2^32 pixels");
}
// the maps go into the engine's stack [truth maps ; result maps]: by n copies each from host pointers, by one copy each from resident stacks
void run_score(anh_runtime* h, const uint16_t* const* truth, const uint16_t* const* result, const uint16_t* d_truth, const uint16_t* d_result, int n, int classes,
               int height, int width, uint64_t* per_pixel, uint64_t* per_region, uint64_t* labelled) {
    DeviceScope scope(h->reps.device_of(0));
    Engine& e = h->reps.engine(0);
    uint16_t* stack = e.reserve_score(n, classes, height, width);   // everything but the vote table, before anything is enqueued
    const size_t plane = (size_t)height * width, bytes = plane * sizeof(uint16_t);
    if (d_truth) {
        HIP_CHECK(hipMemcpyAsync(stack, d_truth, bytes * n, hipMemcpyDeviceToDevice, e.stream));
        HIP_CHECK(hipMemcpyAsync(stack + plane * n, d_result, bytes * n, hipMemcpyDeviceToDevice, e.stream));
    } else {
        for (int i = 0; i < n; ++i) {
            HIP_CHECK(hipMemcpyAsync(stack + plane * i, truth[i], bytes, hipMemcpyHostToDevice, e.stream));
            HIP_CHECK(hipMemcpyAsync(stack + plane * ((size_t)n + i), result[i], bytes, hipMemcpyHostToDevice, e.stream));
        }
    }
    e.score_stacked(n, classes, height, width, per_pixel, per_region, labelled);
}
}  // namespace

int anh_score_batch_device(anh_runtime* h, const uint16_t* d_truth, const uint16_t* d_result, int n, int classes, int height, int width, uint64_t* per_pixel,
                           uint64_t* per_region, uint64_t* labelled) {
    return guarded([&] {
        require_score_sizes(n, classes, height, width);   // first: a size beyond the limit is refused whatever else is wrong
        ANH_REQUIRE(h && d_truth && d_result, "null argument");
        run_score(h, nullptr, nullptr, d_truth, d_result, n, classes, height, width, per_pixel, per_region, labelled);
    });
}

int anh_score_device(anh_runtime* h, const uint16_t* d_truth, const uint16_t* d_result, int classes, int height, int width, uint64_t* per_pixel, uint64_t* per_region,
                     uint64_t* labelled) {
    return anh_score_batch_device(h, d_truth, d_result, 1, classes, height, width, per_pixel, per_region, labelled);
}

int anh_score_batch(anh_runtime* h, const uint16_t* const* truth, const uint16_t* const* result, int n, int classes, int height, int width, uint64_t* per_pixel,
                    uint64_t* per_region, uint64_t* labelled) {
    return guarded([&] {
        require_score_sizes(n, classes, height, width);
        ANH_REQUIRE(h && truth && result, "null argument");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(truth[i] && result[i], "score: null map");
        run_score(h, truth, result, nullptr, nullptr, n, classes, height, width, per_pixel, per_region, labelled);
    });
}

int anh_score(anh_runtime* h, const uint16_t* truth, const uint16_t* result, int classes, int height, int width, uint64_t* per_pixel, uint64_t* per_region,
              uint64_t* labelled) {
    return anh_score_batch(h, &truth, &result, 1, classes, height, width, per_pixel, per_region, labelled);
}

// ---- held-out evaluation (Engine::evaluate_logits, Engine::evaluate_device) ----
namespace {
void require_eval_sizes(int n, int height, int width) {
    ANH_REQUIRE(n >= 1, "evaluate: the batch needs at least one image");
    ANH_REQUIRE(height >= 1 && width >= 1, "evaluate: empty window");
    if (anh_device_count() == 0) fail(ANH_ERR_DEVICE, "no MI355X / HIP device visible");   // no evaluation without a GPU, whatever else is passed
}
// host samples -> the engine's staging buffers [images | labels u16 | weights f32], then the device form; the predicted maps come back
// after the call's one wait
void run_host_evaluate(anh_runtime* h, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width, const double* gains,
                       anh_eval_image* per_image, uint64_t* confusion, uint16_t* predicted) {
    DeviceScope scope(h->reps.device_of(0));
    Engine& e = h->reps.engine(0);
    const size_t plane = (size_t)height * width, C = (size_t)e.spec.cfg.in_channels;
    e.stage_image.reserve((size_t)n * plane * C);
    e.stage_labels.reserve((size_t)n * plane * sizeof(uint16_t));
    e.stage_weights.reserve((size_t)n * plane * sizeof(float));
    if (predicted) e.stage_result.reserve((size_t)n * plane * sizeof(uint16_t));
    std::vector<uint16_t> lab((size_t)n * plane);
    std::vector<float> wgt((size_t)n * plane);
    for (int i = 0; i < n; ++i) {
        const anh_wlabel* src = labels[i];
        uint16_t* dl = lab.data() + (size_t)i * plane;
        float* dw = wgt.data() + (size_t)i * plane;
        for (size_t p = 0; p < plane; ++p) { dl[p] = src[p].label; dw[p] = src[p].weight; }
        HIP_CHECK(hipMemcpyAsync(e.stage_image.as<uint8_t>() + (size_t)i * plane * C, images[i], plane * C, hipMemcpyHostToDevice, e.stream));
    }
    HIP_CHECK(hipMemcpyAsync(e.stage_labels.p, lab.data(), lab.size() * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream));
    HIP_CHECK(hipMemcpyAsync(e.stage_weights.p, wgt.data(), wgt.size() * sizeof(float), hipMemcpyHostToDevice, e.stream));
    uint16_t* d_predicted = predicted ? e.stage_result.as<uint16_t>() : nullptr;
    e.evaluate_device(e.stage_image.as<uint8_t>(), e.stage_labels.as<uint16_t>(), e.stage_weights.as<float>(), n, height, width, gains, per_image, confusion,
                      d_predicted);
    if (predicted) HIP_CHECK(hipMemcpy(predicted, d_predicted, (size_t)n * plane * sizeof(uint16_t), hipMemcpyDeviceToHost));   // (the stream is idle)
}
// the inference net a trainer keeps for evaluation, with the trainer's parameters as they stand: what anh_trainer_snapshot_runtime
// builds, kept between calls
anh_runtime* refreshed_eval_net(anh_trainer* h, int precision) {
    ANH_REQUIRE(precision == ANH_FP32 || precision == ANH_BF16, "unknown precision");
    Engine& e = h->engine();
    std::vector<float> p((size_t)e.spec.n_params), r((size_t)e.spec.n_running);
    e.get_params(p.data(), r.data());   // synchronises: a step in flight finishes first
    if (!h->eval_net || h->eval_net->reps.engine(0).spec.cfg.precision != precision) {
        anh_net_config cfg = e.spec.cfg;
        cfg.precision = precision;
        auto rt = std::make_unique<anh_runtime>();
        rt->build(cfg, h->reps.size() > 1 ? h->reps.device_of(0) : -1);
        h->eval_net = std::move(rt);
    }
    h->eval_net->set_params_all(p.data(), r.data());
    return h->eval_net.get();
}
}  // namespace

int anh_eval_logits_device(anh_runtime* h, const float* d_logits, const uint16_t* d_labels, const float* d_weights, int n, int classes, int height, int width,
                           const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted) {
    return guarded([&] {
        require_eval_sizes(n, height, width);
        ANH_REQUIRE(classes >= 1 && classes <= kEvalMaxClasses, "evaluate: the class count must be within 1..64");
        ANH_REQUIRE(h && d_logits && d_labels && per_image, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).evaluate_logits(d_logits, d_labels, d_weights, n, classes, height, width, gains, per_image, confusion, d_predicted);
    });
}

int anh_runtime_evaluate_device(anh_runtime* h, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights, int n, int height, int width,
                                const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted) {
    return guarded([&] {
        require_eval_sizes(n, height, width);
        ANH_REQUIRE(h && d_images && d_labels && per_image, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).evaluate_device(d_images, d_labels, d_weights, n, height, width, gains, per_image, confusion, d_predicted);
    });
}

int anh_runtime_evaluate(anh_runtime* h, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width, const double* gains,
                         anh_eval_image* per_image, uint64_t* confusion, uint16_t* predicted) {
    return guarded([&] {
        require_eval_sizes(n, height, width);
        ANH_REQUIRE(h && images && labels && per_image, "null argument");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && labels[i], "evaluate: null sample");
        run_host_evaluate(h, images, labels, n, height, width, gains, per_image, confusion, predicted);
    });
}

// ---- annonet_infer() over several images of one size (Engine::infer_batch_device) ----
int anh_infer_batch_device(anh_runtime* h, const uint8_t* d_images, int n, int height, int width, const double* gains, const anh_tiling_params* tiling,
                           uint16_t* d_results, float* d_blended) {
    return guarded([&] {
        ANH_REQUIRE(n >= 1, "infer_batch: the batch needs at least one image");
        ANH_REQUIRE(h && d_images && d_results, "null argument");
        ANH_REQUIRE(height >= 1 && width >= 1, "empty image");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).infer_batch_device(d_images, n, height, width, gains, tiles_for(tiling, width, height), d_results, d_blended);
    });
}

int anh_infer_batch(anh_runtime* h, const uint8_t* const* images, int n, int height, int width, const double* gains, const double* detection_levels,
                    const anh_tiling_params* tiling, uint16_t* const* results, float* const* blended_out) {
    return guarded([&] {
        ANH_REQUIRE(n >= 1, "infer_batch: the batch needs at least one image");
        ANH_REQUIRE(images && results, "infer_batch: null image or result list");
        ANH_REQUIRE(h, "null handle");
        ANH_REQUIRE(height >= 1 && width >= 1, "empty image");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && results[i], "infer_batch: null image or result");
        run_host_infer(h, HostInfer(h, images, n, true, height, width, 1.0, height, width, gains, detection_levels, tiling, results, nullptr, blended_out));
    });
}

int anh_labels_from_logits_device(anh_runtime* h, const float* d_logits, int count, int classes, int win_height, int win_width, int top, int left,
                                  int height, int width, const double* gains, uint16_t* d_result) {
    return guarded([&] {
        ANH_REQUIRE(h && d_logits && d_result, "null argument");
        ANH_REQUIRE(count >= 1 && classes >= 1, "labels_from_logits: empty batch");
        DeviceScope scope(h->reps.device_of(0));
        Engine& e = h->reps.engine(0);
        e.labels_from_logits(d_logits, count, classes, win_height, win_width, top, left, height, width, e.upload_gains(gains, classes), d_result);
    });
}

int anh_infer_batch_plan(const anh_tile* tiles, size_t n_tiles, int n_images, int levels, int cap, int** pairs, int** batch_sizes, size_t* n_batches) {
    return guarded([&] {
        ANH_REQUIRE(tiles && n_tiles >= 1 && pairs && batch_sizes && n_batches, "null argument");
        ANH_REQUIRE(n_images >= 1 && cap >= 1 && levels >= 0 && levels <= 3, "infer_batch_plan: bad argument");
        const auto plan = infer_batch_plan(std::vector<anh_tile>(tiles, tiles + n_tiles), n_images, levels, [cap](int, int) { return cap; });
        const size_t total = n_tiles * (size_t)n_images;
        int* p = (int*)std::malloc(total * 2 * sizeof(int));
        int* b = (int*)std::malloc(std::max<size_t>(1, plan.size()) * sizeof(int));
        if (!p || !b) { std::free(p); std::free(b); fail(ANH_ERR_OOM, "host allocation failed"); }
        size_t k = 0;
        for (size_t i = 0; i < plan.size(); ++i) {
            b[i] = (int)plan[i].size();
            for (const TileSample& s : plan[i]) { p[2 * k] = s.image; p[2 * k + 1] = s.tile; ++k; }
        }
        *pairs = p; *batch_sizes = b; *n_batches = plan.size();
    });
}

// ---- downscaled inference: read_sample's resize (annonet.cpp:153) + annonet_infer() + resize_label_image (annonet.cpp:132-141) ----
namespace {
// std::round(size_scale * side) with size_scale = 1.0 / factor: the expression of annonet_host.h's resize_image_bilinear, which is
// dlib::resize_image(1.0 / factor, img) as read_sample calls it
void scaled_dims_checked(int height, int width, double factor, int& sh, int& sw) {
    ANH_REQUIRE(height >= 1 && width >= 1, "empty image");
    ANH_REQUIRE(std::isfinite(factor) && factor > 0.0, "the downscaling factor must be a positive finite number");
    const double scale = 1.0 / factor;
    const double nr = std::round(scale * height), nc = std::round(scale * width);
    ANH_REQUIRE(nr >= 1 && nc >= 1, "the image is too small for this downscaling factor: a scaled side would be below 1 pixel");
    ANH_REQUIRE(nr <= 32768 && nc <= 32768, "the downscaling factor enlarges the image beyond 32768 pixels per side");
    sh = (int)nr; sw = (int)nc;
}
void require_resize_sides(const char* what, int src_h, int src_w, int dst_h, int dst_w) {
    ANH_REQUIRE(src_h >= 1 && src_w >= 1 && dst_h >= 1 && dst_w >= 1 && src_h <= 32768 && src_w <= 32768 && dst_h <= 32768 && dst_w <= 32768,
                std::string(what) + ": sides must be within 1..32768");
}
}  // namespace

int anh_scaled_dims(int height, int width, double downscaling_factor, int* scaled_height, int* scaled_width) {
    return guarded([&] {
        ANH_REQUIRE(scaled_height && scaled_width, "null argument");
        scaled_dims_checked(height, width, downscaling_factor, *scaled_height, *scaled_width);
    });
}

int anh_resize_image_device(const uint8_t* d_src, int channels, int src_h, int src_w, uint8_t* d_dst, int dst_h, int dst_w, void* hip_stream) {
    return guarded([&] {
        ANH_REQUIRE(d_src && d_dst, "null argument");
        require_resize_sides("resize_image", src_h, src_w, dst_h, dst_w);
        launch_resize_image_bilinear(d_src, channels, src_h, src_w, d_dst, dst_h, dst_w, (hipStream_t)hip_stream);
    });
}

int anh_resize_labels_device(const uint16_t* d_src, int src_h, int src_w, uint16_t* d_dst, int dst_h, int dst_w, void* hip_stream) {
    return guarded([&] {
        ANH_REQUIRE(d_src && d_dst, "null argument");
        require_resize_sides("resize_labels", src_h, src_w, dst_h, dst_w);
        launch_resize_labels_nearest(d_src, src_h, src_w, d_dst, dst_h, dst_w, (hipStream_t)hip_stream);
    });
}

namespace {
// anh_infer_scaled_device (batch false, n = 1: the forward stays infer_device) and anh_infer_scaled_batch_device on resident buffers:
// enqueued on the handle's stream, not synchronised
void infer_scaled_on_device(anh_runtime* h, bool batch, const uint8_t* d_images, int n, int height, int width, double downscaling_factor, const double* gains,
                            const anh_tiling_params* tiling, uint16_t* d_results, uint16_t* d_scaled_labels, float* d_blended) {
    int sh = 0, sw = 0;
    scaled_dims_checked(height, width, downscaling_factor, sh, sw);
    DeviceScope scope(h->reps.device_of(0));
    Engine& e = h->reps.engine(0);
    const int K = e.spec.cfg.classes, C = e.spec.cfg.in_channels;
    const size_t plane = (size_t)sh * sw;
    const std::vector<anh_tile> tiles = tiles_for(tiling, sw, sh);
    if (!batch && !d_blended) { e.stage_blended.reserve(plane * K * 4); d_blended = e.stage_blended.as<float>(); }   // infer_device blends into planes
    auto forward = [&](const uint8_t* d_src, uint16_t* d_labels) {
        if (batch) e.infer_batch_device(d_src, n, sh, sw, gains, tiles, d_labels, d_blended);
        else e.infer_device(d_src, sh, sw, gains, tiles, d_labels, d_blended, /*whole_image=*/true);
    };
    if (downscaling_factor == 1.0) {   // the host's bilinear returns early at scale 1, nearest neighbour at equal size is the identity
        forward(d_images, d_results);
        if (d_scaled_labels) HIP_CHECK(hipMemcpyAsync(d_scaled_labels, d_results, (size_t)n * plane * 2, hipMemcpyDeviceToDevice, e.stream));
        return;
    }
    // reserved before the first kernel; infer_batch_device reserves its own (planes, logits) before its first kernel and writes nothing
    // the shrink does not own, so a batch that cannot fit has only shrunk images into a stage buffer
    e.stage_image.reserve((size_t)n * plane * C);
    if (!d_scaled_labels) { e.stage_result.reserve((size_t)n * plane * 2); d_scaled_labels = e.stage_result.as<uint16_t>(); }
    if (batch) e.reserve_infer_batch(n, sh, sw, tiles, d_blended != nullptr);
    e.resize_image_batch(d_images, n, height, width, e.stage_image.as<uint8_t>(), sh, sw);
    forward(e.stage_image.as<uint8_t>(), d_scaled_labels);
    e.resize_labels_batch(d_scaled_labels, n, sh, sw, d_results, height, width);
}
}  // namespace

int anh_infer_scaled_device(anh_runtime* h, const uint8_t* d_image, int height, int width, double downscaling_factor, const double* gains,
                            const anh_tiling_params* tiling, uint16_t* d_result, uint16_t* d_scaled_labels, float* d_blended) {
    return guarded([&] {
        ANH_REQUIRE(h && d_image && d_result, "null argument");
        infer_scaled_on_device(h, false, d_image, 1, height, width, downscaling_factor, gains, tiling, d_result, d_scaled_labels, d_blended);
    });
}

int anh_infer_scaled(anh_runtime* h, const uint8_t* image, int height, int width, double downscaling_factor, const double* gains,
                     const double* detection_levels, const anh_tiling_params* tiling, uint16_t* result, uint16_t* scaled_labels, float* blended_out) {
    return guarded([&] {
        ANH_REQUIRE(h && image && result, "null argument");
        int sh = 0, sw = 0;
        scaled_dims_checked(height, width, downscaling_factor, sh, sw);
        run_host_infer(h, HostInfer(h, &image, 1, false, height, width, downscaling_factor, sh, sw, gains, detection_levels, tiling, &result, &scaled_labels, &blended_out));
    });
}

// ---- downscaled inference over n images of one original size: anh_infer_scaled composed with anh_infer_batch ----
int anh_resize_image_batch_device(const uint8_t* d_src, int count, int channels, int src_h, int src_w, uint8_t* d_dst, int dst_h, int dst_w, void* hip_stream) {
    return guarded([&] {
        ANH_REQUIRE(count >= 1, "resize_image: the batch needs at least one image");
        ANH_REQUIRE(d_src && d_dst, "null argument");
        require_resize_sides("resize_image", src_h, src_w, dst_h, dst_w);
        launch_resize_image_bilinear_batch(d_src, count, channels, src_h, src_w, d_dst, dst_h, dst_w, (hipStream_t)hip_stream);
    });
}

int anh_resize_labels_batch_device(const uint16_t* d_src, int count, int src_h, int src_w, uint16_t* d_dst, int dst_h, int dst_w, void* hip_stream) {
    return guarded([&] {
        ANH_REQUIRE(count >= 1, "resize_labels: the batch needs at least one label image");
        ANH_REQUIRE(d_src && d_dst, "null argument");
        require_resize_sides("resize_labels", src_h, src_w, dst_h, dst_w);
        launch_resize_labels_nearest_batch(d_src, count, src_h, src_w, d_dst, dst_h, dst_w, (hipStream_t)hip_stream);
    });
}

int anh_infer_scaled_batch_device(anh_runtime* h, const uint8_t* d_images, int n, int height, int width, double downscaling_factor, const double* gains,
                                  const anh_tiling_params* tiling, uint16_t* d_results, uint16_t* d_scaled_labels, float* d_blended) {
    return guarded([&] {
        ANH_REQUIRE(n >= 1, "infer_batch: the batch needs at least one image");
        ANH_REQUIRE(h && d_images && d_results, "null argument");
        infer_scaled_on_device(h, true, d_images, n, height, width, downscaling_factor, gains, tiling, d_results, d_scaled_labels, d_blended);
    });
}

int anh_infer_scaled_batch(anh_runtime* h, const uint8_t* const* images, int n, int height, int width, double downscaling_factor, const double* gains,
                           const double* detection_levels, const anh_tiling_params* tiling, uint16_t* const* results, uint16_t* const* scaled_labels,
                           float* const* blended_out) {
    return guarded([&] {
        ANH_REQUIRE(n >= 1, "infer_batch: the batch needs at least one image");
        ANH_REQUIRE(images && results, "infer_batch: null image or result list");
        ANH_REQUIRE(h, "null handle");
        ANH_REQUIRE(height >= 1 && width >= 1, "empty image");
        int sh = 0, sw = 0;
        scaled_dims_checked(height, width, downscaling_factor, sh, sw);
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && results[i], "infer_batch: null image or result");
        run_host_infer(h, HostInfer(h, images, n, true, height, width, downscaling_factor, sh, sw, gains, detection_levels, tiling, results, scaled_labels, blended_out));
    });
}

// ---- regions of a downscaled call: the table and the blob map belong to the map at the net's resolution, the result map is blown up afterwards ----
int anh_infer_regions_scaled(anh_runtime* h, const uint8_t* image, int height, int width, double downscaling_factor, const double* gains,
                             const double* detection_levels, const anh_tiling_params* tiling, uint16_t* result, uint16_t* scaled_labels, uint32_t* blobs,
                             float* blended_out, anh_region** regions, size_t* n_regions) {
    return guarded([&] {
        int sh = 0, sw = 0;
        scaled_dims_checked(height, width, downscaling_factor, sh, sw);
        require_blob_map_size(sh, sw);
        ANH_REQUIRE(h && image && result && regions && n_regions, "null argument");
        run_regions(h, HostInfer(h, &image, 1, false, height, width, downscaling_factor, sh, sw, gains, detection_levels, tiling, &result, &scaled_labels, &blended_out),
                    &blobs, regions, n_regions);
    });
}

int anh_infer_regions_scaled_batch(anh_runtime* h, const uint8_t* const* images, int n, int height, int width, double downscaling_factor, const double* gains,
                                   const double* detection_levels, const anh_tiling_params* tiling, uint16_t* const* results, uint16_t* const* scaled_labels,
                                   uint32_t* const* blobs, float* const* blended_out, anh_region** regions, size_t* n_regions) {
    return guarded([&] {
        ANH_REQUIRE(n >= 1, "infer_batch: the batch needs at least one image");
        int sh = 0, sw = 0;
        scaled_dims_checked(height, width, downscaling_factor, sh, sw);
        require_blob_batch_size(n, sh, sw);
        ANH_REQUIRE(images && results, "infer_batch: null image or result list");
        ANH_REQUIRE(h && regions && n_regions, "null argument");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && results[i], "infer_batch: null image or result");
        run_regions(h, HostInfer(h, images, n, true, height, width, downscaling_factor, sh, sw, gains, detection_levels, tiling, results, scaled_labels, blended_out),
                    blobs, regions, n_regions);
    });
}

int anh_runtime_set_stream(anh_runtime* h, void* s) { return guarded([&] { ANH_REQUIRE(h, "null handle"); ANH_REQUIRE(h->reps.size() == 1, "a handle that drives several devices keeps its own streams"); h->reps.engine(0).set_stream((hipStream_t)s); }); }
int anh_runtime_get_stream(anh_runtime* h, void** s) { return guarded([&] { ANH_REQUIRE(h && s, "null argument"); *s = (void*)h->reps.engine(0).stream; }); }
int anh_runtime_stores_activations(anh_runtime* h, int* yes) { return guarded([&] { ANH_REQUIRE(h && yes, "null argument"); *yes = h->reps.engine(0).infer_post ? 1 : 0; }); }
int anh_runtime_layer_tensor(anh_runtime* h, int layer, float* out, int64_t capacity, int dims4[4]) {
    return guarded([&] {
        ANH_REQUIRE(h && dims4, "null argument");
        DeviceScope scope(h->reps.device_of(0));
        h->reps.engine(0).layer_tensor(layer, 0, out, capacity, dims4);
    });
}
int anh_runtime_synchronize(anh_runtime* h) {
    return guarded([&] { ANH_REQUIRE(h, "null handle"); h->reps.for_all([](size_t, Engine& e) { e.synchronize(); }); });
}

// ---- TrainingNet ----
int anh_trainer_create(anh_trainer** out) {
    return guarded([&] {
        ANH_REQUIRE(out, "null argument");
        auto h = std::make_unique<anh_trainer>();
        h->reps.devices = selected_devices();
        h->stage = std::vector<std::array<anh_trainer::StageSet, 2>>(h->reps.size());
        h->copy_stream = std::vector<Stream>(h->reps.size());
        *out = h.release();
    });
}
void anh_trainer_destroy(anh_trainer* h) { delete h; }

#define TRAINER_SETTER(name, body) \
    return guarded([&] { ANH_REQUIRE(h, "null handle"); body; })

int anh_trainer_set_net_width(anh_trainer* h, double scaler, int min_filters) {
    TRAINER_SETTER(net_width, { ANH_REQUIRE(scaler > 0 && min_filters >= 1, "bad net width");
        if (scaler != h->cfg.width_scaler || min_filters != h->cfg.min_filters) h->structural_change();
        h->cfg.width_scaler = scaler; h->cfg.min_filters = min_filters; });
}
int anh_trainer_set_class_count(anh_trainer* h, size_t classes) {
    TRAINER_SETTER(class_count, { ANH_REQUIRE(classes >= 1 && classes <= 64, "class count must be 1..64");
        if ((int)classes != h->cfg.classes) h->structural_change();
        h->cfg.classes = (int)classes; });
}
int anh_trainer_set_levels(anh_trainer* h, int levels) { TRAINER_SETTER(levels, { ANH_REQUIRE(levels >= 0 && levels <= 3, "level count must be 0..3"); if (levels != h->cfg.levels) h->structural_change(); h->cfg.levels = levels; }); }
int anh_trainer_set_input_channels(anh_trainer* h, int c) { TRAINER_SETTER(channels, { ANH_REQUIRE(c == 1 || c == 3, "input channels must be 1 or 3"); if (c != h->cfg.in_channels) h->structural_change(); h->cfg.in_channels = c; }); }
int anh_trainer_set_precision(anh_trainer* h, int p) { TRAINER_SETTER(precision, { ANH_REQUIRE(p == ANH_FP32 || p == ANH_BF16, "unknown precision"); if (p != h->cfg.precision) h->structural_change(); h->cfg.precision = p; }); }
int anh_trainer_set_seed(anh_trainer* h, uint64_t seed) { TRAINER_SETTER(seed, { if (seed != h->seed) h->structural_change(); h->seed = seed; }); }

int anh_trainer_initialize(anh_trainer* h) {
    return guarded([&] {
        ANH_REQUIRE(h, "null handle");
        if (anh_device_count() == 0) fail(ANH_ERR_DEVICE, "no MI355X / HIP device visible");
        (void)Spec::build(h->cfg);  // validates the configuration
        h->initialized = true;
        h->dirty = true;
        if (!h->loss_ring.p) {
            // portable + mapped: the update kernel of replica 0 writes it, whichever device that replica lives on (anh_set_devices may come later)
            h->loss_ring.reserve(256 * sizeof(unsigned long long), hipHostMallocPortable | hipHostMallocMapped);
            std::memset(h->loss_ring.p, 0, h->loss_ring.bytes);
            HIP_CHECK(hipHostGetDevicePointer((void**)&h->loss_ring_dev, h->loss_ring.p, 0));
        }
    });
}
int anh_trainer_set_learning_rate(anh_trainer* h, double lr) { TRAINER_SETTER(lr, { ANH_REQUIRE(lr > 0, "learning rate must be positive"); h->sched.lr = lr; }); }
int anh_trainer_set_learning_rate_shrink_factor(anh_trainer* h, double f) { TRAINER_SETTER(shrink, { ANH_REQUIRE(f > 0 && f <= 1, "shrink factor must be in (0,1]"); h->sched.shrink = f; }); }
int anh_trainer_set_iterations_without_progress_threshold(anh_trainer* h, unsigned long n) { TRAINER_SETTER(thresh, { h->sched.threshold = n; }); }
int anh_trainer_set_previous_loss_values_dump_amount(anh_trainer* h, unsigned long n) { TRAINER_SETTER(dump, { h->sched.dump_amount = n; }); }
int anh_trainer_set_all_bn_running_stats_window_sizes(anh_trainer* h, unsigned long n) { TRAINER_SETTER(window, { ANH_REQUIRE(n >= 1, "window must be >= 1"); h->bn_window = n; }); }
int anh_trainer_set_sgd(anh_trainer* h, double wd, double mom) { TRAINER_SETTER(sgd, { ANH_REQUIRE(wd >= 0 && mom >= 0 && mom < 1, "bad sgd parameters"); h->weight_decay = wd; h->momentum = mom; }); }
int anh_trainer_be_verbose(anh_trainer* h) { TRAINER_SETTER(verbose, { h->verbose = true; }); }
int anh_trainer_set_synchronization_file(anh_trainer* h, const char* path, double seconds) {
    return guarded([&] {
        ANH_REQUIRE(h && path, "null argument");
        h->sync_path = path; h->sync_seconds = seconds;
        h->last_sync = std::chrono::steady_clock::now();
        // dlib's trainer resumes from an existing synchronization file.  The reference calls this BEFORE SetClassCount
        // (annonet_train_main.cpp:400-405), so the file is read on the first use of the net, once every structural setter ran.
        h->resume_pending = h->steps == 0;
    });
}
double anh_trainer_get_learning_rate(const anh_trainer* h) {
    if (!h) return 0;
    // a pending resume may change the rate: the host polls this in its loop condition before the first step (annonet_train_main.cpp:583).
    // This getter has no status to return: a resume that fails here leaves resume_pending set and the message in anh_last_error(), and
    // the next call with a status (StartTraining) fails with the same error.
    if (h->resume_pending && h->initialized) (void)guarded([&] { (void)const_cast<anh_trainer*>(h)->engine(); });
    return h->sched.lr;   // changes only inside apply_update, at the fixed loss lag: no timing-dependent polling
}
double anh_trainer_get_last_loss(anh_trainer* h) {
    double v = NAN;
    guarded([&] { ANH_REQUIRE(h, "null handle"); h->engine().synchronize(); h->fetch_all(); v = h->steps ? h->last_loss : h->engine().read_loss(); });
    return v;
}
unsigned long anh_trainer_get_step_count(const anh_trainer* h) { return h ? h->steps : 0; }
int anh_trainer_config(const anh_trainer* h, anh_net_config* out) { return guarded([&] { ANH_REQUIRE(h && out, "null argument"); *out = h->cfg; }); }

int anh_trainer_forward_backward_device(anh_trainer* h, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights,
                                        int n, int height, int width, double loss_scale_n) {
    return guarded([&] {
        ANH_REQUIRE(h && d_images && d_labels && d_weights, "null argument");
        ANH_REQUIRE(loss_scale_n > 0, "loss scale batch must be positive");
        ANH_REQUIRE(h->reps.size() == 1, "device-resident steps drive ONE device: a handle over several devices takes host mini-batches (anh_trainer_step)");
        DeviceScope scope(h->reps.device_of(0));
        Engine& e = h->engine();
        e.bn_window = h->bn_window;
        e.forward_training(image_source(d_images, height, width, e.spec.cfg.in_channels), n, height, width);
        e.backward(d_labels, d_weights, loss_scale_n);
    });
}

int anh_trainer_apply_update(anh_trainer* h, double grad_scale) {
    return guarded([&] {
        ANH_REQUIRE(h, "null handle");
        Engine& e = h->engine();
        // this is step h->steps + 1: its rate is decided by the losses of steps <= h->steps + 1 - kLossLag (deterministic lag)
        if (h->steps + 1 > anh_trainer::kLossLag) h->record_until(h->steps + 1 - anh_trainer::kLossLag);
        for (size_t r = 1; r < h->reps.size(); ++r) { DeviceScope scope(h->reps.device_of(r)); h->reps.engine(r).apply_update(h->sched.lr, h->weight_decay, h->momentum, grad_scale, h->bn_window); }
        DeviceScope scope0(h->reps.device_of(0));
        // the update kernel also ships this step's loss (gradient bucket's trailing slot: already all-reduced under data parallelism)
        const int slot = h->next_slot;
        h->next_slot = (h->next_slot + 1) % 256;
        e.apply_update(h->sched.lr, h->weight_decay, h->momentum, grad_scale, h->bn_window, h->loss_ring_dev + slot, anh_trainer::loss_tag(h->steps + 1));
        ++h->steps;
        h->pending.push_back({slot, h->steps, false, 0.0});
        if (h->verbose && h->steps % 100 == 0) {
            if (!h->pending.empty()) { h->arrive(h->pending.front()); h->last_loss = h->pending.front().value; }   // the oldest loss in flight
            std::printf("step#: %lu  learning rate: %g  loss: %g  steps without apparent progress: %lu\n", h->steps, h->sched.lr, h->last_loss,
                        h->sched.steps_without_progress);
            std::fflush(stdout);
        }
        if (!h->sync_path.empty() && h->sync_seconds > 0) {
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double>(now - h->last_sync).count() >= h->sync_seconds) {
                h->last_sync = now;
                const int rc = anh_trainer_save_state(h, h->sync_path.c_str());
                if (rc != ANH_OK) fail(rc, g_error);
            }
        }
    });
}

extern "C++" {
namespace {
// Packs samples of a host mini-batch into one of a replica's two pinned staging sets, uploads them on the replica's copy stream
// and enqueues forward + backward behind the upload.  Returns once the inputs are packed (the host refills its vectors right
// after StartTraining returns, annonet_train_main.cpp:585-586); packing step k+1 overlaps the GPU work of step k.
anh_trainer::StageSet& stage_and_run(anh_trainer* h, size_t r, Engine& e, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height,
                                     int width, double loss_scale_n) {
    const int C = e.spec.cfg.in_channels, K = e.spec.cfg.classes;
    const size_t plane = (size_t)height * width;
    const BatchLayout lay((size_t)n, plane, C);
    anh_trainer::StageSet& st = h->stage[r][h->host_steps & 1];
    if (!h->copy_stream[r].get()) h->copy_stream[r].create(hipStreamNonBlocking);
    const hipStream_t copy_stream = h->copy_stream[r].get();
    const hipEvent_t uploaded = st.uploaded.ensure(), consumed = st.consumed.ensure();
    if (st.in_flight) {   // the pinned block is free again once the upload of step k-2 is done: the one place a call blocks on the GPU
        const auto w0 = std::chrono::steady_clock::now();
        wait_event(uploaded, h->reps.size() > 1);
        st.wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
    } else st.wait_us = 0;
    if (lay.total > st.pinned.bytes) {
        if (st.in_flight) wait_event(consumed, h->reps.size() > 1);
        st.pinned.reserve(lay.total);
        st.dev.reserve(lay.total);
    }
    // ---- pack: images as they are, weighted labels split into a u16 and an f32 plane; labels validated on the way ----
    uint8_t* base = st.pinned.as<uint8_t>();
    uint16_t* plab = lay.labels(base);
    float* pw = lay.weights(base);
    bool bad_label = false;
    for (int i = 0; i < n; ++i) {
        std::memcpy(base + (size_t)i * plane * C, images[i], plane * C);
        const anh_wlabel* src = labels[i];
        uint16_t* dl = plab + (size_t)i * plane;
        float* dw = pw + (size_t)i * plane;
        unsigned worst = 0;
        for (size_t p = 0; p < plane; ++p) {
            const uint16_t l = src[p].label;
            dl[p] = l; dw[p] = src[p].weight;
            worst |= (unsigned)(l != ANH_LABEL_IGNORE && l >= K);
        }
        bad_label = bad_label || worst != 0;
    }
    ANH_REQUIRE(!bad_label, "label value exceeds the class count");
    // ---- upload behind the step that last read this device block, compute behind the upload ----
    if (st.in_flight) HIP_CHECK(hipStreamWaitEvent(copy_stream, consumed, 0));
    HIP_CHECK(hipMemcpyAsync(st.dev.p, st.pinned.p, lay.total, hipMemcpyHostToDevice, copy_stream));
    HIP_CHECK(hipEventRecord(uploaded, copy_stream));
    HIP_CHECK(hipStreamWaitEvent(e.stream, uploaded, 0));
    uint8_t* dbase = st.dev.as<uint8_t>();
    e.bn_window = h->bn_window;
    e.forward_training(image_source(dbase, height, width, C), n, height, width);
    e.backward(lay.labels(dbase), lay.weights(dbase), loss_scale_n);
    return st;
}
}  // namespace
}  // extern "C++"

int anh_trainer_step(anh_trainer* h, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width) {
    return guarded([&] {
        ANH_REQUIRE(h && images && labels, "null argument");
        ANH_REQUIRE(n >= 1 && height >= 1 && width >= 1, "empty mini-batch");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && labels[i], "null sample");
        (void)h->engine();   // builds every replica on first use
        const size_t R = h->reps.size();
        ANH_REQUIRE((size_t)n >= R, "mini-batch smaller than the number of devices");
        // data parallel (annonet_train_main.cpp:583-614): replica r takes samples [n r / R, n (r+1) / R); the loss
        // scale 1/(N nr nc) uses the WHOLE batch, so the exchange step is a plain sum of the gradient buckets
        std::vector<anh_trainer::StageSet*> used(R, nullptr);
        const auto host_t0 = std::chrono::steady_clock::now();
        h->reps.each([&](size_t r, Engine& e) {   // packing, upload and the step's launches of every replica in parallel (persistent worker threads)
            int64_t lo, hi;
            shard_range(n, (int)R, (int)r, lo, hi);
            used[r] = &stage_and_run(h, r, e, images + lo, labels + lo, (int)(hi - lo), height, width, (double)n);
        });
        if (R > 1) {
            std::vector<float*> buckets(R);
            std::vector<hipStream_t> streams(R);
            for (size_t r = 0; r < R; ++r) { buckets[r] = h->reps.engine(r).grad_bucket(); streams[r] = h->reps.engine(r).stream; }
            const int64_t count = (int64_t)h->reps.engine(0).spec.n_params + 1, first = h->reps.engine(0).early_grad_first();   // the trailing slot carries the loss
            static const bool early_on = read_switch("ANH_EARLY_REDUCE", true);
            static const int xs_every = getenv("ANH_EXCHANGE_SAMPLE") ? atoi(getenv("ANH_EXCHANGE_SAMPLE")) : 8;
            anh_trainer::ExchangeStats& xs = h->xs;
            const bool split = early_on && first > 0 && first < count - 1;
            bool sample = false;
            if (xs_every > 0 && h->host_steps % (unsigned long)xs_every == (unsigned long)xs_every - 1) {
                h->collect_exchange_sample();   // (the previous sampled step ended long ago)
                DeviceScope scope(h->reps.device_of(0));
                for (Event* ev : {&xs.tail0, &xs.tail1, &xs.head0, &xs.head1}) ev->ensure(hipEventDefault);
                sample = true;
                xs.split = split;
            }
            if (split) {
                // the tail of the bucket (every layer but the first two, head, loss) is final while backward still runs
                // (Engine::ev_early_grads): reduce it on side streams now, the short head on the replicas' own streams afterwards
                std::vector<float*> tails(R);
                std::vector<hipStream_t> side(R);
                h->reps.for_all([&](size_t r, Engine& e) {
                    side[r] = e.early_reduce_stream();
                    HIP_CHECK(hipStreamWaitEvent(side[r], e.ev_early_grads.get(), 0));
                    tails[r] = buckets[r] + first;
                });
                if (sample) { DeviceScope scope(h->reps.device_of(0)); HIP_CHECK(hipEventRecord(xs.tail0.get(), side[0])); }
                h->reps.coll->all_reduce_sum(tails, (size_t)(count - first), side);
                if (sample) { DeviceScope scope(h->reps.device_of(0)); HIP_CHECK(hipEventRecord(xs.tail1.get(), side[0])); HIP_CHECK(hipEventRecord(xs.head0.get(), streams[0])); }
                h->reps.coll->all_reduce_sum(buckets, (size_t)first, streams);
                if (sample) { DeviceScope scope(h->reps.device_of(0)); HIP_CHECK(hipEventRecord(xs.head1.get(), streams[0])); xs.pending = true; }
                h->reps.for_all([&](size_t r, Engine& e) {   // the update reads the whole bucket
                    HIP_CHECK(hipEventRecord(e.ev_early_reduced.get(), side[r]));
                    HIP_CHECK(hipStreamWaitEvent(e.stream, e.ev_early_reduced.get(), 0));
                });
            } else {
                if (sample) { DeviceScope scope(h->reps.device_of(0)); HIP_CHECK(hipEventRecord(xs.head0.get(), streams[0])); }
                h->reps.coll->all_reduce_sum(buckets, (size_t)count, streams);
                if (sample) { DeviceScope scope(h->reps.device_of(0)); HIP_CHECK(hipEventRecord(xs.head1.get(), streams[0])); xs.pending = true; }
            }
        }
        const int rc = anh_trainer_apply_update(h, 1.0);
        if (rc != ANH_OK) fail(rc, g_error);
        h->reps.for_all([&](size_t r, Engine& e) {
            HIP_CHECK(hipEventRecord(used[r]->consumed.get(), e.stream));
            used[r]->in_flight = true;
        });
        ++h->host_steps;
        h->xs.host_us_last = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - host_t0).count();
        h->xs.host_us_sum += h->xs.host_us_last;
        h->xs.wait_us_sum += used[0]->wait_us;   // replica 0 packs on the calling thread: its wait is wall time of the call
        ++h->xs.calls;
    });
}

int anh_trainer_exchange_stats(anh_trainer* h, anh_exchange_stats* out) {
    return guarded([&] {
        ANH_REQUIRE(h && out, "null argument");
        h->collect_exchange_sample();
        const anh_trainer::ExchangeStats& xs = h->xs;
        *out = anh_exchange_stats{};
        out->replicas = (int)h->reps.size();
        out->steps = xs.calls;
        out->host_us_mean = xs.calls ? xs.host_us_sum / (double)xs.calls : 0.0;
        out->host_us_last = xs.host_us_last;
        out->host_wait_us_mean = xs.calls ? xs.wait_us_sum / (double)xs.calls : 0.0;
        out->samples = xs.samples;
        out->allreduce_tail_us_mean = xs.samples ? xs.tail_us_sum / (double)xs.samples : 0.0;
        out->allreduce_head_us_mean = xs.samples ? xs.head_us_sum / (double)xs.samples : 0.0;
        out->allreduce_tail_us_last = xs.tail_us_last;
        out->allreduce_head_us_last = xs.head_us_last;
        out->early_reduce = xs.split ? 1 : 0;
        out->uses_rccl = h->reps.coll ? h->reps.coll->transport() : 0;
        out->rccl_version = Collective::rccl_version();
        out->worker_calls = h->reps.workers ? (int64_t)(h->reps.workers->calls() - xs.worker_calls_base) : 0;
        out->bucket_bytes = h->reps.built() ? ((int64_t)h->reps.engine(0).spec.n_params + 1) * 4 : 0;
    });
}
void anh_trainer_reset_exchange_stats(anh_trainer* h) {
    if (!h) return;
    try { h->collect_exchange_sample(); } catch (...) {}
    anh_trainer::ExchangeStats& xs = h->xs;
    xs.calls = 0; xs.host_us_sum = 0; xs.wait_us_sum = 0; xs.samples = 0; xs.tail_us_sum = 0; xs.head_us_sum = 0;
    xs.worker_calls_base = h->reps.workers ? h->reps.workers->calls() : 0;
}

int anh_trainer_grad_buffer(anh_trainer* h, void** d_ptr, int64_t* count) {
    return guarded([&] { ANH_REQUIRE(h && d_ptr && count, "null argument"); *d_ptr = h->engine().grad_bucket(); *count = h->engine().spec.n_params + 1; });
}
int anh_trainer_get_params(anh_trainer* h, float* params, int64_t n_params, float* running, int64_t n_running) {
    return guarded([&] {
        ANH_REQUIRE(h, "null handle");
        Engine& e = h->engine();
        ANH_REQUIRE((!params || n_params == e.spec.n_params) && (!running || n_running == e.spec.n_running), "parameter blob size mismatch");
        e.get_params(params, running);
    });
}
int anh_trainer_set_params(anh_trainer* h, const float* params, int64_t n_params, const float* running, int64_t n_running) {
    return guarded([&] {
        ANH_REQUIRE(h && params && running, "null argument");
        Engine& e = h->engine();
        ANH_REQUIRE(n_params == e.spec.n_params && n_running == e.spec.n_running, "parameter blob size mismatch");
        h->reps.for_all([&](size_t, Engine& er) { er.synchronize(); er.set_params(params, running); });
    });
}
int anh_trainer_replica_params(anh_trainer* h, int replica, float* params, int64_t n_params) {
    return guarded([&] {
        ANH_REQUIRE(h && params, "null argument");
        (void)h->engine();
        ANH_REQUIRE(replica >= 0 && (size_t)replica < h->reps.size(), "replica index out of range");
        ANH_REQUIRE(n_params == h->reps.engine(0).spec.n_params, "size mismatch");
        DeviceScope scope(h->reps.device_of((size_t)replica));
        h->reps.engine((size_t)replica).get_params(params, nullptr);
    });
}
int anh_trainer_get_grads(anh_trainer* h, float* grads, int64_t n_params) {
    return guarded([&] { ANH_REQUIRE(h && grads, "null argument"); ANH_REQUIRE(n_params == h->engine().spec.n_params, "size mismatch"); h->engine().get_grads_canonical(grads); });
}
int anh_trainer_get_momentum(anh_trainer* h, float* m, int64_t n_params) {
    return guarded([&] { ANH_REQUIRE(h && m, "null argument"); ANH_REQUIRE(n_params == h->engine().spec.n_params, "size mismatch"); h->engine().get_momentum(m); });
}
int anh_trainer_set_momentum(anh_trainer* h, const float* m, int64_t n_params) {
    return guarded([&] {
        ANH_REQUIRE(h && m, "null argument");
        ANH_REQUIRE(n_params == h->engine().spec.n_params, "size mismatch");
        h->reps.for_all([&](size_t, Engine& e) { e.set_momentum(m); });
    });
}

int anh_trainer_snapshot_runtime(anh_trainer* h, int precision, anh_runtime** out) {
    return guarded([&] {
        ANH_REQUIRE(h && out, "null argument");
        Engine& e = h->engine();
        std::vector<float> p((size_t)e.spec.n_params), r((size_t)e.spec.n_running);
        e.get_params(p.data(), r.data());  // synchronises: a step in flight finishes first (annonet_train_main.cpp:558)
        anh_net_config cfg = e.spec.cfg;
        cfg.precision = precision;
        // A snapshot is ONE replica on the trainer's first device: the host serializes it (annonet_train_main.cpp:557-565, at step 0,
        // every save interval and at the end) while the trainer's own communicator may have collectives in flight — no second set of
        // engines, no second ncclCommInitAll.  Handles the caller creates for inference (anh_runtime_create / _deserialize) span the
        // selected devices.
        auto rt = std::make_unique<anh_runtime>();
        rt->build(cfg, h->reps.size() > 1 ? h->reps.device_of(0) : -1);
        rt->set_params_all(p.data(), r.data());
        *out = rt.release();
    });
}

int anh_trainer_evaluate(anh_trainer* h, int precision, const uint8_t* const* images, const anh_wlabel* const* labels, int n, int height, int width,
                         const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* predicted) {
    return guarded([&] {
        require_eval_sizes(n, height, width);
        ANH_REQUIRE(h && images && labels && per_image, "null argument");
        for (int i = 0; i < n; ++i) ANH_REQUIRE(images[i] && labels[i], "evaluate: null sample");
        run_host_evaluate(refreshed_eval_net(h, precision), images, labels, n, height, width, gains, per_image, confusion, predicted);
    });
}

int anh_trainer_evaluate_device(anh_trainer* h, int precision, const uint8_t* d_images, const uint16_t* d_labels, const float* d_weights, int n, int height,
                                int width, const double* gains, anh_eval_image* per_image, uint64_t* confusion, uint16_t* d_predicted) {
    return guarded([&] {
        require_eval_sizes(n, height, width);
        ANH_REQUIRE(h && d_images && d_labels && per_image, "null argument");
        anh_runtime* rt = refreshed_eval_net(h, precision);
        DeviceScope scope(rt->reps.device_of(0));
        rt->reps.engine(0).evaluate_device(d_images, d_labels, d_weights, n, height, width, gains, per_image, confusion, d_predicted);
    });
}

int anh_trainer_save_state(anh_trainer* h, const char* path) {
    return guarded([&] {
        ANH_REQUIRE(h && path, "null argument");
        Engine& e = h->engine();
        e.synchronize();
        h->fetch_all();   // the losses still ahead of the schedule's lag are stored as such: a resumed run records them when an uninterrupted one would
        const Spec& s = e.spec;
        std::vector<float> p((size_t)s.n_params), m((size_t)s.n_params), r((size_t)s.n_running);
        e.get_params(p.data(), r.data());
        e.get_momentum(m.data());
        const std::vector<double> updates = e.get_running_updates();
        const std::string tmp = std::string(path) + ".tmp";
        {
            std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
            if (!f) fail(ANH_ERR_IO, "cannot write " + tmp);
            BlobHeader hd{};
            std::memcpy(hd.magic, kStateMagic, 8);
            hd.levels = s.cfg.levels; hd.in_channels = s.cfg.in_channels; hd.classes = s.cfg.classes; hd.min_filters = s.cfg.min_filters;
            hd.width_scaler = s.cfg.width_scaler; hd.n_params = s.n_params; hd.n_running = s.n_running;
            f.write((const char*)&hd, sizeof hd);
            const uint64_t steps = h->steps, nh = h->sched.history.size(), budget = h->sched.check_budget, swp = h->sched.steps_without_progress;
            const uint64_t n_unrec = h->pending.size(), n_bn = updates.size();
            f.write((const char*)&steps, 8); f.write((const char*)&h->sched.lr, 8); f.write((const char*)&budget, 8); f.write((const char*)&swp, 8);
            f.write((const char*)&h->last_loss, 8);
            f.write((const char*)&nh, 8);
            for (double v : h->sched.history) f.write((const char*)&v, 8);
            f.write((const char*)&n_unrec, 8);
            for (const auto& pl : h->pending) { const uint64_t st = pl.step; f.write((const char*)&st, 8); f.write((const char*)&pl.value, 8); }
            f.write((const char*)&n_bn, 8);
            for (double v : updates) f.write((const char*)&v, 8);
            f.write((const char*)p.data(), p.size() * 4); f.write((const char*)m.data(), m.size() * 4); f.write((const char*)r.data(), r.size() * 4);
            if (!f) fail(ANH_ERR_IO, "short write to " + tmp);
        }
        if (std::rename(tmp.c_str(), path) != 0) fail(ANH_ERR_IO, std::string("cannot move state file into place: ") + path);
    });
}

namespace {
void load_state_into(anh_trainer* h, Engine& e, const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) fail(ANH_ERR_IO, std::string("cannot read ") + path);
    BlobHeader hd;
    f.read((char*)&hd, sizeof hd);
    if (!f || std::memcmp(hd.magic, kStateMagic, 8) != 0) fail(ANH_ERR_IO, "not an annonet_hip trainer state file (or one of an older format)");
    const Spec& s = e.spec;
    if (hd.levels != s.cfg.levels || hd.in_channels != s.cfg.in_channels || hd.classes != s.cfg.classes || hd.n_params != s.n_params || hd.n_running != s.n_running)
        fail(ANH_ERR_IO, "trainer state file was written for a different net");
    uint64_t steps = 0, nh = 0, budget = 0, swp = 0, n_unrec = 0, n_bn = 0;
    double lr = 0, last_loss = 0;
    f.read((char*)&steps, 8); f.read((char*)&lr, 8); f.read((char*)&budget, 8); f.read((char*)&swp, 8); f.read((char*)&last_loss, 8); f.read((char*)&nh, 8);
    if (!f || nh > (1u << 26)) fail(ANH_ERR_IO, "trainer state file is corrupt");
    std::deque<double> hist;
    for (uint64_t i = 0; i < nh; ++i) { double v; f.read((char*)&v, 8); hist.push_back(v); }
    f.read((char*)&n_unrec, 8);
    if (!f || n_unrec > 4096) fail(ANH_ERR_IO, "trainer state file is corrupt");
    std::deque<anh_trainer::PendingLoss> unrec;
    for (uint64_t i = 0; i < n_unrec; ++i) { uint64_t st; double v; f.read((char*)&st, 8); f.read((char*)&v, 8); unrec.push_back({0, (unsigned long)st, true, v}); }
    f.read((char*)&n_bn, 8);
    if (!f || n_bn > 4096) fail(ANH_ERR_IO, "trainer state file is corrupt");
    std::vector<double> updates((size_t)n_bn);
    for (auto& v : updates) f.read((char*)&v, 8);
    std::vector<float> p((size_t)s.n_params), m((size_t)s.n_params), r((size_t)s.n_running);
    f.read((char*)p.data(), p.size() * 4); f.read((char*)m.data(), m.size() * 4); f.read((char*)r.data(), r.size() * 4);
    if (!f) fail(ANH_ERR_IO, "trainer state file is truncated");
    h->reps.for_all([&](size_t, Engine& er) {   // every replica resumes from the same state
        er.synchronize();
        er.set_params(p.data(), r.data());
        er.set_momentum(m.data());
        er.set_running_updates(updates);
    });
    h->pending = unrec;
    h->steps = (unsigned long)steps; h->last_loss = last_loss;
    h->sched.lr = lr; h->sched.check_budget = (unsigned long)budget; h->sched.steps_without_progress = (unsigned long)swp; h->sched.history = hist;
}
}  // namespace

void anh_trainer::resume() { load_state_into(this, reps.engine(0), sync_path.c_str()); }

int anh_trainer_load_state(anh_trainer* h, const char* path) {
    return guarded([&] {
        ANH_REQUIRE(h && path, "null argument");
        h->resume_pending = false;   // an explicit load wins over the synchronization file
        load_state_into(h, h->engine(), path);
    });
}

int anh_trainer_set_stream(anh_trainer* h, void* s) {
    return guarded([&] { ANH_REQUIRE(h, "null handle"); ANH_REQUIRE(h->reps.size() == 1, "a handle that drives several devices keeps its own streams"); h->engine().set_stream((hipStream_t)s); });
}
int anh_trainer_get_stream(anh_trainer* h, void** s) { return guarded([&] { ANH_REQUIRE(h && s, "null argument"); *s = (void*)h->engine().stream; }); }
int anh_trainer_early_grads(anh_trainer* h, int64_t* first) {
    return guarded([&] {
        ANH_REQUIRE(h && first, "null argument");
        Engine& e = h->engine();
        *first = h->reps.size() > 1 ? (int64_t)e.spec.n_params + 1 : e.early_grad_first();   // (several replicas: the library reduces the buckets itself)
    });
}
int anh_trainer_step_graph_stats(anh_trainer* h, int64_t* captures, int64_t* launches) {
    return guarded([&] {
        ANH_REQUIRE(h && captures && launches, "null argument");
        Engine& e = h->engine();
        *captures = (int64_t)e.step_graph_captures; *launches = (int64_t)e.step_graph_launches;
    });
}
int anh_trainer_wait_early_grads(anh_trainer* h, void* hip_stream) {
    return guarded([&] {
        ANH_REQUIRE(h && hip_stream, "null argument");
        Engine& e = h->engine();
        ANH_REQUIRE(e.early_grad_first() <= e.spec.n_params, "this net has no early gradient part");
        HIP_CHECK(hipStreamWaitEvent((hipStream_t)hip_stream, e.ev_early_grads.get(), 0));
    });
}
int anh_trainer_synchronize(anh_trainer* h) {
    return guarded([&] {
        ANH_REQUIRE(h, "null handle");
        (void)h->engine();
        bool bad = false;
        h->reps.for_all([&](size_t, Engine& e) {
            e.synchronize();
            bad = e.read_error_flag_and_clear() || bad;
        });
        if (bad) fail(ANH_ERR_INVALID, "a label value exceeds the class count");
    });
}
int anh_trainer_layer_tensor(anh_trainer* h, int layer, int which, float* out, int64_t capacity, int dims4[4]) {
    return guarded([&] { ANH_REQUIRE(h && dims4, "null argument"); h->engine().layer_tensor(layer, which, out, capacity, dims4); });
}

// ---- profiling ----
static Engine* engine_of(void* handle, int is_trainer) {
    ANH_REQUIRE(handle, "null handle");
    return is_trainer ? &((anh_trainer*)handle)->engine() : &((anh_runtime*)handle)->reps.engine(0);
}
int anh_profile_enable(void* handle, int is_trainer, int enable) {
    return guarded([&] { Engine* e = engine_of(handle, is_trainer); e->synchronize(); e->prof.enabled = enable != 0; });
}
int anh_profile_set_filter(void* handle, int is_trainer, const char* substring) {
    return guarded([&] { Engine* e = engine_of(handle, is_trainer); e->synchronize(); e->prof.filter = substring ? substring : ""; });
}
int anh_profile_set_sampling(void* handle, int is_trainer, int every) {
    return guarded([&] { ANH_REQUIRE(every >= 1, "sampling interval must be >= 1"); Engine* e = engine_of(handle, is_trainer); e->synchronize(); e->prof.sample_every = every; e->prof.pass_index = 0; });
}
int anh_profile_reset(void* handle, int is_trainer) {
    return guarded([&] { Engine* e = engine_of(handle, is_trainer); e->synchronize(); e->prof.reset(); });
}
int anh_profile_count(void* handle, int is_trainer) {
    int n = -1;
    guarded([&] { Engine* e = engine_of(handle, is_trainer); e->synchronize(); n = (int)e->prof.entries.size(); });
    return n;
}
int anh_profile_entry(void* handle, int is_trainer, int index, char* name, size_t name_cap, double* total_ms, int64_t* launches, double* flops, double* bytes) {
    return guarded([&] {
        Engine* e = engine_of(handle, is_trainer);
        ANH_REQUIRE(index >= 0 && index < (int)e->prof.entries.size(), "profile index out of range");
        const Profiler::Entry& en = e->prof.entries[index];
        if (name && name_cap) { std::strncpy(name, en.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
        if (total_ms) *total_ms = en.total_ms;
        if (launches) *launches = en.launches;
        if (flops) *flops = en.flops;
        if (bytes) *bytes = en.bytes;
    });
}
int anh_profile_launch_order(void* handle, int is_trainer, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        Engine* e = engine_of(handle, is_trainer);
        std::string joined;
        for (const std::string& n : e->prof.order) { joined += n; joined += '\n'; }
        if (needed) *needed = joined.size() + 1;
        if (buf && cap) { std::strncpy(buf, joined.c_str(), cap - 1); buf[cap - 1] = 0; }
    });
}

// ---- host logic ----
int anh_get_tiles(int width, int height, const anh_tiling_params* params, anh_tile** tiles, size_t* count) {
    return guarded([&] {
        ANH_REQUIRE(tiles && count, "null argument");
        std::vector<anh_tile> t = tiles_for(params, width, height);
        anh_tile* out = (anh_tile*)std::malloc(std::max<size_t>(1, t.size()) * sizeof(anh_tile));
        if (!out) fail(ANH_ERR_OOM, "host allocation failed");
        std::memcpy(out, t.data(), t.size() * sizeof(anh_tile));
        *tiles = out; *count = t.size();
    });
}
int anh_set_weights(const uint16_t* labels, int nr, int nc, double cw, double iw, anh_wlabel* out) {
    return guarded([&] { ANH_REQUIRE(labels && out, "null argument"); set_weights(labels, nr, nc, cw, iw, out); });
}
int anh_random_rect_containing_point(uint32_t dx, uint32_t dy, long px, long py, long w, long hgt, anh_rect* out) {
    return guarded([&] { ANH_REQUIRE(out, "null argument"); *out = random_rect_containing_point(dx, dy, px, py, w, hgt); });
}
int anh_outpaint(uint8_t* image, int nr, int nc, int channels, const anh_rect* inside) {
    return guarded([&] { ANH_REQUIRE(image && inside, "null argument"); outpaint(image, nr, nc, channels, *inside); });
}
int anh_dataset_create(int channels, anh_dataset** out) {
    return guarded([&] {
        ANH_REQUIRE(out, "null argument");
        ANH_REQUIRE(channels == 1 || channels == 3, "input channels must be 1 or 3");
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); fail(ANH_ERR_DEVICE, "no MI355X / HIP device visible"); }
        auto d = std::make_unique<anh_dataset>();
        d->channels = channels;
        d->stream.create(hipStreamNonBlocking);
        *out = d.release();
    });
}
void anh_dataset_destroy(anh_dataset* d) { delete d; }
int anh_dataset_add(anh_dataset* d, const uint8_t* image_hwc, const uint16_t* labels, int height, int width, int* index) {
    return guarded([&] {
        ANH_REQUIRE(d && image_hwc && labels, "null argument");
        ANH_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width < ((int64_t)1 << 31), "bad image size");
        anh_dataset::Item it;
        const size_t px = (size_t)height * width;
        it.image.reserve(px * d->channels); it.labels.reserve(px * 2);
        it.height = height; it.width = width;
        HIP_CHECK(hipMemcpy(it.image.p, image_hwc, px * d->channels, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(it.labels.p, labels, px * 2, hipMemcpyHostToDevice));
        d->resident_bytes += px * d->channels + px * 2;
        int slot;
        if (!d->free_slots.empty()) { slot = d->free_slots.back(); d->free_slots.pop_back(); d->items[(size_t)slot] = std::move(it); }
        else { d->items.push_back(std::move(it)); slot = (int)d->items.size() - 1; }
        if (index) *index = slot;
    });
}
int anh_dataset_remove(anh_dataset* d, int index) {
    return guarded([&] {
        ANH_REQUIRE(d, "null dataset");
        ANH_REQUIRE(index >= 0 && (size_t)index < d->items.size() && d->items[(size_t)index].height > 0, "dataset remove: no such image");
        HIP_CHECK(hipStreamSynchronize(d->stream.get()));   // the crop kernels that read the image have finished
        anh_dataset::Item& it = d->items[(size_t)index];
        d->drop_index(it);
        d->resident_bytes -= (uint64_t)it.height * it.width * (d->channels + 2);
        it.image.release(); it.labels.release(); it.height = it.width = 0;
        d->free_slots.push_back(index);
    });
}
int anh_dataset_resident_bytes(const anh_dataset* d, uint64_t* bytes) {
    return guarded([&] { ANH_REQUIRE(d && bytes, "null argument"); *bytes = d->resident_bytes; });
}
int anh_dataset_prepare(anh_dataset* d, int index, const uint16_t* classes_to_ignore, int n_ignore, double by_area, double by_width, double by_height,
                        int receptive_field_side, anh_dataset_info* info) {
    return guarded([&] {
        ANH_REQUIRE(d && info, "null argument");
        ANH_REQUIRE(n_ignore >= 0 && n_ignore <= 64 && (classes_to_ignore || n_ignore == 0), "dataset prepare: 0..64 classes to ignore");
        ANH_REQUIRE(receptive_field_side > 0, "dataset prepare: the receptive-field side must be positive");
        ANH_REQUIRE(!(by_area < 0) && !(by_width < 0) && !(by_height < 0) && by_area == by_area && by_width == by_width && by_height == by_height,
                    "dataset prepare: negative threshold");
        anh_dataset::Item& it = d->item(index, "dataset prepare");
        const hipStream_t st = d->stream.get();
        HIP_CHECK(hipStreamSynchronize(st));   // the crop kernels that read the labels have finished
        d->drop_index(it);
        const int H = it.height, W = it.width;
        const int64_t pixels = (int64_t)H * W;
        const size_t blocks = dataset_index_blocks(pixels);
        const bool by_size = std::isfinite(by_area) || std::isfinite(by_width) || std::isfinite(by_height);
        // words: [0] pixels relabelled by class, [1] by size, [2] the one table's row offset (0), [3..67) class totals, [67] bad label | blob count
        constexpr size_t kWords = 3 + kCropMaxClasses + 1;
        d->prep_words.reserve(kWords * 8); d->prep_counts.reserve((size_t)kCropMaxClasses * blocks * 4);
        if (kWords * 8 > d->pinned.bytes) d->pinned.reserve(kWords * 8);
        if (by_size) {
            d->blob_parent.reserve((size_t)pixels * 4); d->blob_map.reserve((size_t)pixels * 4); d->blob_sums.reserve(blob_scan_blocks(pixels) * 4);
        }
        unsigned long long* words = d->prep_words.as<unsigned long long>();
        unsigned long long* h_words = d->pinned.as<unsigned long long>();
        int* bad = reinterpret_cast<int*>(words + 3 + kCropMaxClasses);
        unsigned* blob_count = reinterpret_cast<unsigned*>(bad + 1);
        uint16_t* labels = it.labels.as<uint16_t>();
        HIP_CHECK(hipMemsetAsync(words, 0, kWords * 8, st));
        if (n_ignore > 0) {
            DatasetIgnoreList list{};
            list.n = n_ignore;
            for (int i = 0; i < n_ignore; ++i) list.values[i] = classes_to_ignore[i];
            launch_dataset_relabel(labels, pixels, list, words, st);
        }
        if (by_size) {
            launch_blob_label(labels, 1, H, W, d->blob_parent.as<int>(), d->blob_map.as<uint32_t>(), d->blob_sums.as<unsigned>(), blob_count, st);
            HIP_CHECK(hipMemcpyAsync(h_words, blob_count, 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            const uint32_t rows = *reinterpret_cast<const unsigned*>(h_words) - 1u;   // "labels including the background one"
            d->blob_table.reserve(((size_t)rows + 1) * sizeof(anh_region));   // the labelling does not need the table: sized once the count is back
            const double rf = (double)receptive_field_side;
            launch_blob_number(d->blob_parent.as<int>(), d->blob_map.as<uint32_t>(), labels, 1, H, W, d->blob_table.as<anh_region>(), words + 2, st);
            launch_dataset_ignore_large(labels, d->blob_map.as<uint32_t>(), d->blob_table.as<anh_region>(), rows, H, W, by_area * rf * rf, by_width * rf, by_height * rf,
                                        words + 1, st);
        }
        launch_dataset_index(labels, pixels, d->prep_counts.as<unsigned>(), words + 3, bad, st);
        HIP_CHECK(hipMemcpyAsync(h_words, words, kWords * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        anh_dataset_info got{};
        got.ignored_by_class = (int64_t)h_words[0]; got.ignored_by_size = (int64_t)h_words[1];
        ANH_REQUIRE(*reinterpret_cast<const int*>(h_words + 3 + kCropMaxClasses) == 0, "dataset prepare: a label value is 64 or more (and not the ignore label)");
        for (int c = 0; c < kCropMaxClasses; ++c)
            if (h_words[3 + c]) { got.classes[got.present] = (uint16_t)c; got.counts[got.present] = h_words[3 + c]; ++got.present; }
        if (got.present) {
            it.index.reserve((size_t)got.present * blocks * 4);
            for (int i = 0; i < got.present; ++i)
                HIP_CHECK(hipMemcpyAsync(it.index.as<unsigned>() + (size_t)i * blocks, d->prep_counts.as<unsigned>() + (size_t)got.classes[i] * blocks, blocks * 4,
                                         hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        it.index_bytes = (uint64_t)got.present * blocks * 4;
        d->resident_bytes += it.index_bytes;
        it.info = got; it.prepared = true;
        *info = got;
    });
}
int anh_dataset_scratch_bytes(const anh_dataset* d, uint64_t* bytes) {
    return guarded([&] {
        ANH_REQUIRE(d && bytes, "null argument");
        *bytes = d->prep_counts.bytes + d->prep_words.bytes + d->blob_parent.bytes + d->blob_map.bytes + d->blob_sums.bytes + d->blob_table.bytes;
    });
}
int anh_dataset_labels(anh_dataset* d, int index, uint16_t* labels) {
    return guarded([&] {
        ANH_REQUIRE(d && labels, "null argument");
        const anh_dataset::Item& it = d->item(index, "dataset labels");
        HIP_CHECK(hipStreamSynchronize(d->stream.get()));
        HIP_CHECK(hipMemcpy(labels, it.labels.p, (size_t)it.height * it.width * 2, hipMemcpyDeviceToHost));
    });
}
int anh_resolve_pick(const anh_dataset_info* info, uint32_t class_draw, uint64_t point_draw, uint16_t* label, uint64_t* k) {
    return guarded([&] { ANH_REQUIRE(info && label && k, "null argument"); resolve_pick(*info, class_draw, point_draw, label, k); });
}
int anh_dataset_pick(anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, anh_crop_pick* out) {
    return guarded([&] {
        ANH_REQUIRE(d && specs && draws && out, "null argument");
        const anh_dataset::Staged g = d->stage_specs(specs, draws, n, dim);
        const hipStream_t st = d->stream.get();
        HIP_CHECK(hipMemcpyAsync(g.h_bad, d->d_bad.p, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(g.h_picks, d->d_picks.p, (size_t)n * sizeof(DatasetPick), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ANH_REQUIRE(g.h_bad[1] == 0, "picked crops: the point index does not match the resident labels");
        anh_dataset::picks_to_host(g, g.h_jobs, n, out);
    });
}
namespace {
void crop_batch_to_host(anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, int classes, double class_weight, double image_weight,
                        uint8_t* images, anh_wlabel* labels, anh_crop_pick* picks) {
    ANH_REQUIRE(d && specs && images && labels && n >= 1 && dim >= 1, "crop batch: bad argument");
    const size_t plane = (size_t)dim * dim;
    const BatchLayout lay((size_t)n, plane, d->channels);
    const hipStream_t stream = d->stream.get();
    d->out.reserve(lay.total);
    uint8_t* base = d->out.as<uint8_t>();
    d->crop_batch(specs, draws, n, dim, classes, class_weight, image_weight, base, lay.labels(base), lay.weights(base), picks);
    std::vector<uint16_t> hl((size_t)n * plane);
    std::vector<float> hw((size_t)n * plane);
    HIP_CHECK(hipMemcpyAsync(images, base, lay.img_bytes, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(hl.data(), lay.labels(base), hl.size() * 2, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(hw.data(), lay.weights(base), hw.size() * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t i = 0; i < hl.size(); ++i) { labels[i].label = hl[i]; labels[i].weight = hw[i]; }
}
// the crops of step k are cut on the dataset's stream while the trainer's stream still runs step k-1
void step_on_crops(anh_trainer* h, anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, double class_weight, double image_weight) {
    ANH_REQUIRE(n >= 1 && dim >= 1, "empty mini-batch");
    ANH_REQUIRE(h->reps.size() == 1, "device-cut crops live on ONE device: a handle over several devices takes host mini-batches (anh_trainer_step)");
    Engine& e = h->engine();
    const int C = e.spec.cfg.in_channels, K = e.spec.cfg.classes;
    ANH_REQUIRE(C == d->channels, "the dataset's channel count differs from the net's");
    const BatchLayout lay((size_t)n, (size_t)dim * dim, C);
    anh_trainer::StageSet& st = h->stage[0][h->host_steps & 1];
    const hipEvent_t uploaded = st.uploaded.ensure(), consumed = st.consumed.ensure();
    if (lay.total > st.dev.bytes) {
        if (st.in_flight) wait_event(consumed, h->reps.size() > 1);
        st.dev.reserve(lay.total);
    }
    if (st.in_flight) HIP_CHECK(hipStreamWaitEvent(d->stream.get(), consumed, 0));
    uint8_t* dbase = st.dev.as<uint8_t>();
    d->crop_batch(specs, draws, n, dim, K, class_weight, image_weight, dbase, lay.labels(dbase), lay.weights(dbase), nullptr);
    HIP_CHECK(hipEventRecord(uploaded, d->stream.get()));
    HIP_CHECK(hipStreamWaitEvent(e.stream, uploaded, 0));
    int rc = anh_trainer_forward_backward_device(h, dbase, lay.labels(dbase), lay.weights(dbase), n, dim, dim, (double)n);
    if (rc != ANH_OK) fail(rc, g_error);
    rc = anh_trainer_apply_update(h, 1.0);
    if (rc != ANH_OK) fail(rc, g_error);
    HIP_CHECK(hipEventRecord(consumed, e.stream));
    st.in_flight = true;
    ++h->host_steps;
}
}  // namespace
int anh_dataset_crop_batch(anh_dataset* d, const anh_crop_spec* specs, int n, int dim, int classes, double class_weight, double image_weight,
                           uint8_t* images, anh_wlabel* labels) {
    return guarded([&] { crop_batch_to_host(d, specs, nullptr, n, dim, classes, class_weight, image_weight, images, labels, nullptr); });
}
int anh_dataset_crop_batch_picked(anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, int classes, double class_weight,
                                  double image_weight, uint8_t* images, anh_wlabel* labels, anh_crop_pick* picks) {
    return guarded([&] {
        ANH_REQUIRE(draws, "null argument");
        crop_batch_to_host(d, specs, draws, n, dim, classes, class_weight, image_weight, images, labels, picks);
    });
}
int anh_trainer_step_crops(anh_trainer* h, anh_dataset* d, const anh_crop_spec* specs, int n, int dim, double class_weight, double image_weight) {
    return guarded([&] {
        ANH_REQUIRE(h && d && specs, "null argument");
        step_on_crops(h, d, specs, nullptr, n, dim, class_weight, image_weight);
    });
}
int anh_trainer_step_crops_picked(anh_trainer* h, anh_dataset* d, const anh_crop_spec* specs, const anh_crop_draw* draws, int n, int dim, double class_weight,
                                  double image_weight) {
    return guarded([&] {
        ANH_REQUIRE(h && d && specs && draws, "null argument");
        step_on_crops(h, d, specs, draws, n, dim, class_weight, image_weight);
    });
}
int anh_ignore_large_nonzero_regions(uint16_t* labels, int nr, int nc, double by_area, double by_width, double by_height, int rf, int64_t* ignored) {
    return guarded([&] {
        ANH_REQUIRE(labels && nr > 0 && nc > 0 && rf > 0, "ignore_large_nonzero_regions: bad argument");
        ANH_REQUIRE((int64_t)nr * nc < (int64_t)1 << 31, "ignore_large_nonzero_regions: image too large");
        ANH_REQUIRE(!(by_area < 0) && !(by_width < 0) && !(by_height < 0), "ignore_large_nonzero_regions: negative threshold");
        const int64_t n = ignore_large_nonzero_regions(labels, nr, nc, by_area, by_width, by_height, rf);
        if (ignored) *ignored = n;
    });
}
static void* host_copy(const std::string& s) {
    void* p = std::malloc(s.size() ? s.size() : 1);
    if (!p) fail(ANH_ERR_OOM, "host allocation failed");
    std::memcpy(p, s.data(), s.size());
    return p;
}
int anh_dnn_envelope_pack(const char* classes_json, size_t json_size, double downscaling_factor, const void* net_blob, size_t net_size,
                          void** file, size_t* file_size) {
    return guarded([&] {
        ANH_REQUIRE(file && file_size && (classes_json || json_size == 0) && (net_blob || net_size == 0), "null argument");
        const std::string out = dnn_envelope_pack(std::string(classes_json ? classes_json : "", json_size), downscaling_factor,
                                                  std::string(net_blob ? (const char*)net_blob : "", net_size));
        *file = host_copy(out); *file_size = out.size();
    });
}
int anh_dnn_envelope_unpack(const void* file, size_t file_size, char** classes_json, size_t* json_size, double* downscaling_factor,
                            void** net_blob, size_t* net_size) {
    return guarded([&] {
        ANH_REQUIRE(file && classes_json && json_size && downscaling_factor && net_blob && net_size, "null argument");
        std::string json, net;
        double factor = 0;
        dnn_envelope_unpack(std::string((const char*)file, file_size), json, factor, net);
        void* j = host_copy(json);
        void* n = nullptr;
        try { n = host_copy(net); } catch (...) { std::free(j); throw; }
        *classes_json = (char*)j; *json_size = json.size(); *downscaling_factor = factor; *net_blob = n; *net_size = net.size();
    });
}
int64_t anh_count_steps_without_decrease(const double* values, int64_t n, double p) {
    if (!values && n > 0) return -1;
    return count_steps_without_decrease(values, n, p);
}

}  // extern "C"
