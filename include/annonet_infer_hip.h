// annonet_infer_hip.h — annonet_infer() (annonet_infer.h:34-42) with the whole per-image loop on the GPU: the image is
// uploaded once, tiles are cut with a clamp-to-edge window inside the first conv kernel, logits are blended into
// resident class planes and the argmax runs on the device (annonet_infer.cpp:42-214); only the u16 label map comes
// back.  Same signature as the reference's function, so annonet_infer_main.cpp:468 compiles unchanged against it.
#ifndef ANNONET_INFER_HIP_H
#define ANNONET_INFER_HIP_H

#include <cstdlib>
#include <string>

#include "NetPimpl.h"
#include "tiling/dlib-wrapper.h"

// The reference leaves the blended class planes in temp.blended_output after every call (annonet_infer.cpp:80-85, annonet_infer.h:31).
// Here they live in HBM and travel back (K x H x W floats over PCIe) only when temp.keep_blended_output is set.  A drop-in host that
// READS temp.blended_output after the call keeps the reference's behaviour without touching its code: compile with
// -DANNONET_HIP_KEEP_BLENDED_OUTPUT=1, or run with ANH_KEEP_BLENDED_OUTPUT=1 in the environment — either makes the flag default to true.
#ifndef ANNONET_HIP_KEEP_BLENDED_OUTPUT
#define ANNONET_HIP_KEEP_BLENDED_OUTPUT 0
#endif
inline bool annonet_hip_keep_blended_default() {
    static const bool from_env = [] { const char* e = std::getenv("ANH_KEEP_BLENDED_OUTPUT"); return e && std::atoi(e) != 0; }();
    return ANNONET_HIP_KEEP_BLENDED_OUTPUT != 0 || from_env;
}

struct annonet_infer_temp {  // annonet_infer.h:26-32; the GPU path keeps its scratch inside the net handle
    NetPimpl::input_type input_tile;
    std::vector<dlib::point> detection_seeds;
    dlib::matrix<unsigned int> connected_blobs;
    std::vector<dlib::matrix<float>> blended_output;  // filled when keep_blended_output is set (see above for its default)
    bool keep_blended_output = annonet_hip_keep_blended_default();
    dlib::matrix<uint16_t> scaled_result_image;       // annonet_infer_scaled: the label map at the net's resolution, filled on every scaled call
    std::vector<dlib::matrix<uint16_t>> scaled_result_images;   // annonet_infer_scaled_batch: one such map per image, filled on every call
    // annonet_infer_regions: one row per connected blob of the UNFILTERED label map, in blob-number order (anh_region, annonet_hip.h);
    // connected_blobs (the reference fills it on every call, annonet_infer.cpp:217) travels back only when keep_connected_blobs is set.
    // detection_seeds stays empty: it can be as long as the image, and regions[i].seeds carries the count per blob.
    std::vector<anh_region> regions;
    bool keep_connected_blobs = false;
    // annonet_infer_regions_batch / _scaled_batch: image i's table (blob numbers restart at 1 per image) and, under keep_connected_blobs, its blob map
    std::vector<std::vector<anh_region>> regions_per_image;
    std::vector<dlib::matrix<unsigned int>> connected_blobs_per_image;
};

namespace annonet_infer_hip_detail {
// the net's class count, once the sizes of the per-class arguments (and of a batch) are checked; `fn` names the calling function in the message
inline int classes_checked(NetPimpl::RuntimeNet& net, const char* fn, const std::vector<double>& gains, const std::vector<double>& detection_levels,
                           const std::vector<NetPimpl::input_type>* batch = nullptr) {
    anh_net_config cfg;
    NetPimpl::check(anh_runtime_config(net.handle(), &cfg));
    if (batch && batch->empty()) throw std::runtime_error(std::string(fn) + ": the batch needs at least one image");
    if (!gains.empty() && (int)gains.size() != cfg.classes) throw std::runtime_error(std::string(fn) + ": one gain per class expected");
    if (!detection_levels.empty() && (int)detection_levels.size() != cfg.classes) throw std::runtime_error(std::string(fn) + ": one detection level per class expected");
    return cfg.classes;
}
inline const double* data_or_null(const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); }
inline anh_tiling_params to_params(const tiling::parameters& p) { return anh_tiling_params{p.max_tile_width, p.max_tile_height, p.overlap_x, p.overlap_y}; }
inline const uint8_t* pixels(const NetPimpl::input_type& image) { return reinterpret_cast<const uint8_t*>(&*image.begin()); }
// planes [K][h][w] as they came back -> temp.blended_output
inline void store_planes(annonet_infer_temp& temp, const std::vector<float>& planes, int K, int h, int w) {
    temp.blended_output.resize(K);
    for (int k = 0; k < K; ++k) {
        temp.blended_output[k].set_size(h, w);
        std::copy(planes.begin() + (size_t)k * h * w, planes.begin() + (size_t)(k + 1) * h * w, temp.blended_output[k].begin());
    }
}
// the image and result pointers of a (non-empty) batch of ONE size; the results are sized here
struct batch_pointers {
    int n, H, W;
    std::vector<const uint8_t*> images;
    std::vector<uint16_t*> results;
    std::vector<float*> planes_of;   // all null but the last image's, when the planes are kept
    batch_pointers(const char* fn, const std::vector<NetPimpl::input_type>& input_images, std::vector<dlib::matrix<uint16_t>>& result_images) {
        n = (int)input_images.size(); H = (int)input_images[0].nr(); W = (int)input_images[0].nc();
        images.resize((size_t)n); results.resize((size_t)n); planes_of.assign((size_t)n, nullptr);
        result_images.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            if ((int)input_images[i].nr() != H || (int)input_images[i].nc() != W) throw std::runtime_error(std::string(fn) + ": the images of a batch must have one size");
            images[i] = pixels(input_images[i]);
            result_images[i].set_size(H, W);
            results[i] = &*result_images[i].begin();
        }
    }
};
}  // namespace annonet_infer_hip_detail

inline void annonet_infer(NetPimpl::RuntimeNet& net, const NetPimpl::input_type& input_image, dlib::matrix<uint16_t>& result_image,
                          annonet_infer_temp& temp, const std::vector<double>& gains = std::vector<double>(),
                          const std::vector<double>& detection_levels = std::vector<double>(),
                          const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer", gains, detection_levels), H = (int)input_image.nr(), W = (int)input_image.nc();
    result_image.set_size(H, W);
    std::vector<float> planes;
    if (temp.keep_blended_output) planes.resize((size_t)K * H * W);
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    NetPimpl::check(anh_infer(net.handle(), d::pixels(input_image), H, W, d::data_or_null(gains), d::data_or_null(detection_levels), &tp, &*result_image.begin(),
                              temp.keep_blended_output ? planes.data() : nullptr));
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, H, W);
}

// annonet_infer() that also leaves what the reference computes on the way to its detection-level filter (annonet_infer.cpp:194-223): the
// connected blobs of the label map BEFORE the filter and, per blob, class, bounding box, area, seed count and peak margin over "clean"
// (anh_infer_regions; labelled on the device).  result_image is bit-identical to annonet_infer()'s on one device.  Always fills
// temp.regions; temp.connected_blobs when temp.keep_connected_blobs is set; temp.blended_output keeps its keep_blended_output rule.
inline void annonet_infer_regions(NetPimpl::RuntimeNet& net, const NetPimpl::input_type& input_image, dlib::matrix<uint16_t>& result_image,
                                  annonet_infer_temp& temp, const std::vector<double>& gains = std::vector<double>(),
                                  const std::vector<double>& detection_levels = std::vector<double>(),
                                  const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_regions", gains, detection_levels), H = (int)input_image.nr(), W = (int)input_image.nc();
    result_image.set_size(H, W);
    std::vector<float> planes;
    if (temp.keep_blended_output) planes.resize((size_t)K * H * W);
    if (temp.keep_connected_blobs) temp.connected_blobs.set_size(H, W);
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "connected_blobs receives the u32 blob map as it is");
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    anh_region* table = nullptr;
    size_t rows = 0;
    NetPimpl::check(anh_infer_regions(net.handle(), d::pixels(input_image), H, W, d::data_or_null(gains), d::data_or_null(detection_levels), &tp, &*result_image.begin(),
                                      temp.keep_connected_blobs ? reinterpret_cast<uint32_t*>(&*temp.connected_blobs.begin()) : nullptr,
                                      temp.keep_blended_output ? planes.data() : nullptr, &table, &rows));
    try { temp.regions.assign(table, table + rows); } catch (...) { anh_free(table); throw; }
    anh_free(table);
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, H, W);
}

// annonet_infer() over several images of ONE size in one call (anh_infer_batch): a folder of camera frames that are one tile each runs the
// net with several frames per launch, and every result equals annonet_infer() of that image alone, bit for bit.  result_images[i]
// belongs to input_images[i].  temp.blended_output keeps its keep_blended_output rule and holds the planes of the LAST image, as it
// would after a loop of annonet_infer() calls.
inline void annonet_infer_batch(NetPimpl::RuntimeNet& net, const std::vector<NetPimpl::input_type>& input_images, std::vector<dlib::matrix<uint16_t>>& result_images,
                                annonet_infer_temp& temp, const std::vector<double>& gains = std::vector<double>(),
                                const std::vector<double>& detection_levels = std::vector<double>(),
                                const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_batch", gains, detection_levels, &input_images);
    d::batch_pointers b("annonet_infer_batch", input_images, result_images);
    std::vector<float> planes;
    if (temp.keep_blended_output) { planes.resize((size_t)K * b.H * b.W); b.planes_of[b.n - 1] = planes.data(); }
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    NetPimpl::check(anh_infer_batch(net.handle(), b.images.data(), b.n, b.H, b.W, d::data_or_null(gains), d::data_or_null(detection_levels), &tp, b.results.data(),
                                    temp.keep_blended_output ? b.planes_of.data() : nullptr));
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, b.H, b.W);
}

// What the reference's inference program does around annonet_infer() for a net trained with a downscaling factor, in one call on the
// GPU: read_sample's dlib::resize_image(1.0 / factor, image) (annonet.cpp:153, bilinear), annonet_infer() on the shrunk image
// (annonet_infer_main.cpp:468) and resize_label_image back to the original size (annonet_infer_main.cpp:413, annonet.cpp:132-141, nearest
// neighbour).  input_image comes at its ORIGINAL size; result_image has that size; temp.scaled_result_image is the map at the net's
// resolution, which the program scores its confusion matrices on (annonet_infer_main.cpp:482-492).  temp.blended_output keeps its
// keep_blended_output rule and holds the planes at the net's resolution.
inline void annonet_infer_scaled(NetPimpl::RuntimeNet& net, const NetPimpl::input_type& input_image, double downscaling_factor,
                                 dlib::matrix<uint16_t>& result_image, annonet_infer_temp& temp, const std::vector<double>& gains = std::vector<double>(),
                                 const std::vector<double>& detection_levels = std::vector<double>(),
                                 const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_scaled", gains, detection_levels), H = (int)input_image.nr(), W = (int)input_image.nc();
    int sh = 0, sw = 0;
    NetPimpl::check(anh_scaled_dims(H, W, downscaling_factor, &sh, &sw));
    result_image.set_size(H, W);
    temp.scaled_result_image.set_size(sh, sw);
    std::vector<float> planes;
    if (temp.keep_blended_output) planes.resize((size_t)K * sh * sw);
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    NetPimpl::check(anh_infer_scaled(net.handle(), d::pixels(input_image), H, W, downscaling_factor, d::data_or_null(gains), d::data_or_null(detection_levels), &tp,
                                     &*result_image.begin(), &*temp.scaled_result_image.begin(), temp.keep_blended_output ? planes.data() : nullptr));
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, sh, sw);
}

// annonet_infer_scaled() over several images of ONE original size in one call (anh_infer_scaled_batch): one batched shrink, the forward
// batches of annonet_infer_batch() at the net's resolution, one batched blow-up.  result_images[i] (original size) and
// temp.scaled_result_images[i] (the net's resolution) belong to input_images[i] and equal, bit for bit, what annonet_infer_scaled() gives
// for that image alone.  temp.blended_output keeps its keep_blended_output rule and holds the planes of the LAST image at the net's
// resolution, as it would after a loop of annonet_infer_scaled() calls.
inline void annonet_infer_scaled_batch(NetPimpl::RuntimeNet& net, const std::vector<NetPimpl::input_type>& input_images, double downscaling_factor,
                                       std::vector<dlib::matrix<uint16_t>>& result_images, annonet_infer_temp& temp,
                                       const std::vector<double>& gains = std::vector<double>(), const std::vector<double>& detection_levels = std::vector<double>(),
                                       const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_scaled_batch", gains, detection_levels, &input_images);
    int sh = 0, sw = 0;
    NetPimpl::check(anh_scaled_dims((int)input_images[0].nr(), (int)input_images[0].nc(), downscaling_factor, &sh, &sw));
    d::batch_pointers b("annonet_infer_scaled_batch", input_images, result_images);
    std::vector<uint16_t*> scaled((size_t)b.n);
    temp.scaled_result_images.resize((size_t)b.n);
    for (int i = 0; i < b.n; ++i) {
        temp.scaled_result_images[i].set_size(sh, sw);
        scaled[i] = &*temp.scaled_result_images[i].begin();
    }
    std::vector<float> planes;
    if (temp.keep_blended_output) { planes.resize((size_t)K * sh * sw); b.planes_of[b.n - 1] = planes.data(); }
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    NetPimpl::check(anh_infer_scaled_batch(net.handle(), b.images.data(), b.n, b.H, b.W, downscaling_factor, d::data_or_null(gains), d::data_or_null(detection_levels), &tp,
                                           b.results.data(), scaled.data(), temp.keep_blended_output ? b.planes_of.data() : nullptr));
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, sh, sw);
}

namespace annonet_infer_hip_detail {
// what the batched regions forms share: the blob maps (when kept) sized to h x w, and the call's ONE table cut into temp.regions_per_image
inline std::vector<uint32_t*> blob_pointers(annonet_infer_temp& temp, int n, int h, int w) {
    static_assert(sizeof(unsigned int) == sizeof(uint32_t), "connected_blobs receives the u32 blob map as it is");
    std::vector<uint32_t*> blobs((size_t)n, nullptr);
    temp.connected_blobs_per_image.resize(temp.keep_connected_blobs ? (size_t)n : 0);
    for (int i = 0; i < n && temp.keep_connected_blobs; ++i) {
        temp.connected_blobs_per_image[i].set_size(h, w);
        blobs[i] = reinterpret_cast<uint32_t*>(&*temp.connected_blobs_per_image[i].begin());
    }
    return blobs;
}
inline void store_regions_per_image(annonet_infer_temp& temp, anh_region* table, const std::vector<size_t>& rows) {
    try {
        temp.regions_per_image.resize(rows.size());
        const anh_region* at = table;
        for (size_t i = 0; i < rows.size(); ++i) { temp.regions_per_image[i].assign(at, at + rows[i]); at += rows[i]; }
    } catch (...) { anh_free(table); throw; }
    anh_free(table);
}
}  // namespace annonet_infer_hip_detail

// annonet_infer_regions() over several images of ONE size in one call (anh_infer_regions_batch): the forward batches of
// annonet_infer_batch(), then ONE batched labelling of all the maps.  result_images[i], temp.regions_per_image[i] and (under
// keep_connected_blobs) temp.connected_blobs_per_image[i] belong to input_images[i] and equal, bit for bit, what annonet_infer_regions()
// gives for that image alone.  temp.blended_output holds the planes of the LAST image, as after annonet_infer_batch().
inline void annonet_infer_regions_batch(NetPimpl::RuntimeNet& net, const std::vector<NetPimpl::input_type>& input_images,
                                        std::vector<dlib::matrix<uint16_t>>& result_images, annonet_infer_temp& temp,
                                        const std::vector<double>& gains = std::vector<double>(), const std::vector<double>& detection_levels = std::vector<double>(),
                                        const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_regions_batch", gains, detection_levels, &input_images);
    d::batch_pointers b("annonet_infer_regions_batch", input_images, result_images);
    std::vector<uint32_t*> blobs = d::blob_pointers(temp, b.n, b.H, b.W);
    std::vector<float> planes;
    if (temp.keep_blended_output) { planes.resize((size_t)K * b.H * b.W); b.planes_of[b.n - 1] = planes.data(); }
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    anh_region* table = nullptr;
    std::vector<size_t> rows((size_t)b.n, 0);
    NetPimpl::check(anh_infer_regions_batch(net.handle(), b.images.data(), b.n, b.H, b.W, d::data_or_null(gains), d::data_or_null(detection_levels), &tp, b.results.data(),
                                            temp.keep_connected_blobs ? blobs.data() : nullptr, temp.keep_blended_output ? b.planes_of.data() : nullptr, &table,
                                            rows.data()));
    d::store_regions_per_image(temp, table, rows);
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, b.H, b.W);
}

// annonet_infer_scaled() plus the region table (anh_infer_regions_scaled): temp.regions and (under keep_connected_blobs)
// temp.connected_blobs belong to temp.scaled_result_image's unfiltered map, at the net's resolution, where the reference runs its filter;
// result_image is that map, filtered, blown up to the original size.
inline void annonet_infer_regions_scaled(NetPimpl::RuntimeNet& net, const NetPimpl::input_type& input_image, double downscaling_factor,
                                         dlib::matrix<uint16_t>& result_image, annonet_infer_temp& temp, const std::vector<double>& gains = std::vector<double>(),
                                         const std::vector<double>& detection_levels = std::vector<double>(),
                                         const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_regions_scaled", gains, detection_levels), H = (int)input_image.nr(), W = (int)input_image.nc();
    int sh = 0, sw = 0;
    NetPimpl::check(anh_scaled_dims(H, W, downscaling_factor, &sh, &sw));
    result_image.set_size(H, W);
    temp.scaled_result_image.set_size(sh, sw);
    if (temp.keep_connected_blobs) temp.connected_blobs.set_size(sh, sw);
    std::vector<float> planes;
    if (temp.keep_blended_output) planes.resize((size_t)K * sh * sw);
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    anh_region* table = nullptr;
    size_t rows = 0;
    NetPimpl::check(anh_infer_regions_scaled(net.handle(), d::pixels(input_image), H, W, downscaling_factor, d::data_or_null(gains), d::data_or_null(detection_levels), &tp,
                                             &*result_image.begin(), &*temp.scaled_result_image.begin(),
                                             temp.keep_connected_blobs ? reinterpret_cast<uint32_t*>(&*temp.connected_blobs.begin()) : nullptr,
                                             temp.keep_blended_output ? planes.data() : nullptr, &table, &rows));
    try { temp.regions.assign(table, table + rows); } catch (...) { anh_free(table); throw; }
    anh_free(table);
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, sh, sw);
}

// annonet_infer_regions_scaled() over several images of ONE original size in one call (anh_infer_regions_scaled_batch): one batched
// shrink, the forward batches, ONE batched labelling at the net's resolution, one batched blow-up.  Fills result_images,
// temp.scaled_result_images, temp.regions_per_image and (under keep_connected_blobs) temp.connected_blobs_per_image, image by image as
// annonet_infer_regions_scaled() gives them.
inline void annonet_infer_regions_scaled_batch(NetPimpl::RuntimeNet& net, const std::vector<NetPimpl::input_type>& input_images, double downscaling_factor,
                                               std::vector<dlib::matrix<uint16_t>>& result_images, annonet_infer_temp& temp,
                                               const std::vector<double>& gains = std::vector<double>(),
                                               const std::vector<double>& detection_levels = std::vector<double>(),
                                               const tiling::parameters& tiling_parameters = tiling::parameters()) {
    namespace d = annonet_infer_hip_detail;
    const int K = d::classes_checked(net, "annonet_infer_regions_scaled_batch", gains, detection_levels, &input_images);
    int sh = 0, sw = 0;
    NetPimpl::check(anh_scaled_dims((int)input_images[0].nr(), (int)input_images[0].nc(), downscaling_factor, &sh, &sw));
    d::batch_pointers b("annonet_infer_regions_scaled_batch", input_images, result_images);
    std::vector<uint16_t*> scaled((size_t)b.n);
    temp.scaled_result_images.resize((size_t)b.n);
    for (int i = 0; i < b.n; ++i) {
        temp.scaled_result_images[i].set_size(sh, sw);
        scaled[i] = &*temp.scaled_result_images[i].begin();
    }
    std::vector<uint32_t*> blobs = d::blob_pointers(temp, b.n, sh, sw);
    std::vector<float> planes;
    if (temp.keep_blended_output) { planes.resize((size_t)K * sh * sw); b.planes_of[b.n - 1] = planes.data(); }
    const anh_tiling_params tp = d::to_params(tiling_parameters);
    anh_region* table = nullptr;
    std::vector<size_t> rows((size_t)b.n, 0);
    NetPimpl::check(anh_infer_regions_scaled_batch(net.handle(), b.images.data(), b.n, b.H, b.W, downscaling_factor, d::data_or_null(gains),
                                                   d::data_or_null(detection_levels), &tp, b.results.data(), scaled.data(),
                                                   temp.keep_connected_blobs ? blobs.data() : nullptr, temp.keep_blended_output ? b.planes_of.data() : nullptr, &table,
                                                   rows.data()));
    d::store_regions_per_image(temp, table, rows);
    if (temp.keep_blended_output) d::store_planes(temp, planes, K, sh, sw);
}

// What the reference's inference program does with a result after annonet_infer() (annonet_infer_main.cpp:482-491, :202-272), on the GPU
// (anh_score_batch): per image the labelled pixels, the per-pixel counts and the two-way per-region votes, [classes][classes] each with the
// ground truth as the first index.  The rule is written out in annonet_hip.h.  The maps of one call have ONE size; truth_maps[i] belongs
// to result_maps[i]; a truth value >= classes (65535 = ignore) is unlabelled, a result value >= classes casts no vote.
struct annonet_score_counts {
    std::vector<uint64_t> labelled;      // [n]
    std::vector<uint64_t> per_pixel;     // [n][classes][classes]
    std::vector<uint64_t> per_region;    // [n][classes][classes]
};

inline void annonet_score(NetPimpl::RuntimeNet& net, const std::vector<const dlib::matrix<uint16_t>*>& truth_maps,
                          const std::vector<const dlib::matrix<uint16_t>*>& result_maps, int classes, annonet_score_counts& counts) {
    if (truth_maps.empty() || truth_maps.size() != result_maps.size()) throw std::runtime_error("annonet_score: one result map per truth map, at least one pair");
    if (classes < 1) throw std::runtime_error("annonet_score: the class count must be at least 1");
    const int n = (int)truth_maps.size(), H = (int)truth_maps[0]->nr(), W = (int)truth_maps[0]->nc();
    std::vector<const uint16_t*> truth((size_t)n), result((size_t)n);
    for (int i = 0; i < n; ++i) {
        if ((int)truth_maps[i]->nr() != H || (int)truth_maps[i]->nc() != W || (int)result_maps[i]->nr() != H || (int)result_maps[i]->nc() != W)
            throw std::runtime_error("annonet_score: the maps of a call must have one size");
        if (H < 1 || W < 1) throw std::runtime_error("annonet_score: empty maps");
        truth[i] = &*truth_maps[i]->begin();
        result[i] = &*result_maps[i]->begin();
    }
    const size_t cells = (size_t)n * classes * classes;
    counts.labelled.assign((size_t)n, 0);
    counts.per_pixel.assign(cells, 0);
    counts.per_region.assign(cells, 0);
    NetPimpl::check(anh_score_batch(net.handle(), truth.data(), result.data(), n, classes, H, W, counts.per_pixel.data(), counts.per_region.data(),
                                    counts.labelled.data()));
}

// one pair of maps
inline void annonet_score(NetPimpl::RuntimeNet& net, const dlib::matrix<uint16_t>& truth_map, const dlib::matrix<uint16_t>& result_map, int classes,
                          annonet_score_counts& counts) {
    annonet_score(net, std::vector<const dlib::matrix<uint16_t>*>{&truth_map}, std::vector<const dlib::matrix<uint16_t>*>{&result_map}, classes, counts);
}

#endif  // ANNONET_INFER_HIP_H
