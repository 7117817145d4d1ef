// infer_tool.cpp -> annonet_amd/lib/annonet_infer_hip: the job of the reference's inference tool (annonet_infer_main.cpp:283-538) on the
// drop-in headers, as a three-stage pipeline built from this repository's own parts:
//
//     ImageReaders (N threads: read_sample)  ->  Segmenter (this thread: annonet_infer() on the GPU(s))  ->  ResultWriters (M threads: PNG)
//
// Kept from the reference because they are its observable behaviour: the option names and defaults (:308-316), the lines it prints
// (input directory, gains / detection levels, scan summary, "All N images processed in ... (actual inference: ...)", "Processing time
// excluding the first image: average = ... ms, max = ... ms", both confusion matrices), the files it reads (annonet.dnn,
// <image>_mask.png) and writes (<image>_result.png), and its exit codes (2 for option errors, 1 otherwise).
// Extensions: --precision fp32|bf16, --devices 0,1,... (tile lists sharded over several GPUs from this one process), --dnn <file>,
// --host-resize, --image-batch N (consecutive images of one size go through annonet_infer_batch() together, or through
// annonet_infer_scaled_batch() where the GPU resizes).  A net with a downscaling factor other than 1: the image goes to the GPU at its original size and annonet_infer_scaled()
// shrinks it, infers and blows the label map back up there (the reference does both resizes on the CPU: annonet.cpp:153 in the readers,
// annonet_infer_main.cpp:413 in the writers); --host-resize keeps them on this program's reader / writer threads.  Same files, same matrices.
// --write-regions: annonet_infer_regions() instead of annonet_infer(), and <image>_result_regions.csv beside every result PNG.
// --gpu-score: both confusion matrices are counted on the GPU by annonet_score(), not on this thread; the printed matrices are the same.
#define ANNONET_HIP_NO_DLIB
#include "../../include/annonet_infer_hip.h"
#include "annonet_host.h"

#include <functional>
#include <map>

namespace {

// ---- command line ---------------------------------------------------------------------------------------------------
struct Settings {
    std::string directory, dnn_file = "annonet.dnn", precision = "bf16";
    std::vector<std::string> gain_args, detection_args;
    std::vector<int> devices;
    int max_tile_w = 1024, max_tile_h = 1024;   // the reference's GPU-build defaults (:300-303)
    bool host_resize = false;
    bool write_regions = false;
    bool gpu_score = false;
    int image_batch = 1;
    int readers = (int)std::max(1u, std::thread::hardware_concurrency()), writers = (int)std::max(1u, std::thread::hardware_concurrency());
};

const char* usage_text() {
    return "Do inference using trained semantic-segmentation networks\nUsage:\n  annonet_infer_hip [OPTION...] <input-directory>\n\n"
           "  -i, --input-directory arg            Input image directory\n"
           "  -g, --gain arg                       Supply a class-specific gain, for example: 1:-0.5\n"
           "  -d, --detection arg                  Supply a class-specific detection level that _comes on top of gain_, for example: 1:1.5\n"
           "  -w, --tile-max-width arg             Set max tile width (default: 1024)\n"
           "  -h, --tile-max-height arg            Set max tile height (default: 1024)\n"
           "      --full-image-reader-thread-count arg\n"
           "      --result-image-writer-thread-count arg\n"
           "      --precision fp32|bf16            fp32 = bit-exact parity mode, bf16 = MFMA throughput mode (default)\n"
           "      --devices 0,1,...                GPUs this process drives (tile lists are sharded over them)\n"
           "      --dnn file                       trained net (default: annonet.dnn)\n"
           "      --host-resize                    downscaled nets: resize image and label map on the CPU threads, not on the GPU\n"
           "      --write-regions                  also write <image>_result_regions.csv: one line per DETECTED connected blob of the label map\n"
           "                                       (class_index,class_name,left,top,right,bottom,area,seeds,peak; boxes in pixels of the net's\n"
           "                                       resolution).  Works with --image-batch and with the GPU resize of a downscaled net: the\n"
           "                                       blobs of a whole batch are labelled together, at the net's resolution\n"
           "      --gpu-score                      score the results against the masks on the GPU (annonet_score(): the blobs of truth and result\n"
           "                                       maps are labelled there, a group of --image-batch images by one call); same matrices\n"
           "      --image-batch N                  up to N consecutive images of one size run as one batch (default: 1, image by image);\n"
           "                                       with a downscaled net whose resizes run on the GPU the batch forms on the ORIGINAL size and is\n"
           "                                       shrunk and blown up there by one launch each; with --devices the\n"
           "                                       images of a batch are dealt out to the GPUs.  A batch's time is charged in equal parts\n"
           "                                       to its images, and \"excluding the first image\" then excludes the first batch\n";
}

Settings read_command_line(int argc, char** argv) {
    Settings s;
    std::map<std::string, std::function<void(const std::string&)>> with_value = {
        {"-i", [&](const std::string& v) { s.directory = v; }}, {"--input-directory", [&](const std::string& v) { s.directory = v; }},
        {"-g", [&](const std::string& v) { s.gain_args.push_back(v); }}, {"--gain", [&](const std::string& v) { s.gain_args.push_back(v); }},
        {"-d", [&](const std::string& v) { s.detection_args.push_back(v); }}, {"--detection", [&](const std::string& v) { s.detection_args.push_back(v); }},
        {"-w", [&](const std::string& v) { s.max_tile_w = std::stoi(v); }}, {"--tile-max-width", [&](const std::string& v) { s.max_tile_w = std::stoi(v); }},
        {"-h", [&](const std::string& v) { s.max_tile_h = std::stoi(v); }}, {"--tile-max-height", [&](const std::string& v) { s.max_tile_h = std::stoi(v); }},
        {"--full-image-reader-thread-count", [&](const std::string& v) { s.readers = std::stoi(v); }},
        {"--result-image-writer-thread-count", [&](const std::string& v) { s.writers = std::stoi(v); }},
        {"--precision", [&](const std::string& v) { s.precision = v; }}, {"--dnn", [&](const std::string& v) { s.dnn_file = v; }},
        {"--image-batch", [&](const std::string& v) { s.image_batch = std::stoi(v); }},
        {"--devices", [&](const std::string& v) { std::stringstream list(v); std::string item; while (std::getline(list, item, ',')) s.devices.push_back(std::stoi(item)); }},
    };
    for (int i = 1; i < argc; ++i) {
        const std::string word = argv[i];
        auto option = with_value.find(word);
        if (option != with_value.end()) {
            if (i + 1 >= argc) throw std::runtime_error("Option '" + word + "' is missing an argument");
            option->second(argv[++i]);
        } else if (word == "--host-resize") s.host_resize = true;
        else if (word == "--write-regions") s.write_regions = true;
        else if (word == "--gpu-score") s.gpu_score = true;
        else if (!word.empty() && word[0] == '-') throw std::runtime_error("Option '" + word + "' does not exist");
        else if (s.directory.empty()) s.directory = word;
        else throw std::runtime_error("Unexpected argument " + word);
    }
    if (s.directory.empty()) throw std::runtime_error("Option 'input-directory' is required but not present");
    if (s.precision != "bf16" && s.precision != "fp32") throw std::runtime_error("--precision must be fp32 or bf16");
    if (s.image_batch < 1) throw std::runtime_error("--image-batch must be at least 1");
    return s;
}

// "index:value" pairs (-g 1:-0.5) -> one value per class, 0 where nothing was given (annonet_infer_main.cpp:36-63)
std::vector<double> per_class_values(const std::vector<std::string>& args, size_t class_count) {
    std::vector<double> values(class_count, 0.0);
    for (const std::string& arg : args) {
        const size_t colon = arg.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 >= arg.size()) throw std::runtime_error("The gains must be supplied in the format index:gain (e.g., 1:-0.5)");
        const unsigned long index = std::stoul(arg.substr(0, colon));
        if (index >= class_count) {
            std::ostringstream message;
            message << "Can't define class-specific value for index " << index << " when there are only " << class_count << " classes";
            throw std::runtime_error(message.str());
        }
        values[index] = std::stod(arg.substr(colon + 1));
    }
    return values;
}

void echo_per_class(const char* caption, const std::vector<double>& values) {
    std::cout << caption;
    for (size_t k = 0; k < values.size(); ++k) std::cout << " " << k << ":" << values[k];
    std::cout << std::endl;
}

// ---- --write-regions: the table annonet_infer_regions() leaves, as <image>_result_regions.csv ------------------------------------------
// One header line, then one line per DETECTED blob in blob-number order.  The header's last field names the downscaling factor the
// boxes have to be multiplied by to reach the original image; the lines carry the nine fields before it.
std::string csv_field(const std::string& text) {
    if (text.find_first_of(",\"\n") == std::string::npos) return text;
    std::string quoted = "\"";
    for (const char c : text) { if (c == '"') quoted += '"'; quoted += c; }
    return quoted + "\"";
}
void write_regions_csv(const std::string& path, const std::vector<anh_region>& regions, const std::vector<AnnoClass>& classes, double downscaling) {
    std::ofstream out(path);
    out << "class_index,class_name,left,top,right,bottom,area,seeds,peak,downscaling_factor=" << downscaling << "\n";
    out << std::setprecision(9);   // a float survives the round trip
    for (const anh_region& r : regions) {
        if (!r.detected) continue;
        out << r.label << ',' << csv_field(r.label < classes.size() ? classes[r.label].classlabel : std::string()) << ',' << r.left << ',' << r.top << ','
            << r.right << ',' << r.bottom << ',' << r.area << ',' << r.seeds << ',' << r.peak << "\n";
    }
    if (!out.flush()) throw std::runtime_error("could not write " + path);
}

// ---- the trained net: annonet.dnn = (anno classes json, downscaling factor, serialized RuntimeNet) ---------------------------------
struct TrainedNet {
    NetPimpl::RuntimeNet net;
    std::vector<AnnoClass> classes;
    double downscaling = 1.0;

    static TrainedNet load(const std::string& path, bool fp32) {
        TrainedNet t;
        const std::string bytes = annonet_io::slurp(path);
        char* json = nullptr; void* blob = nullptr; size_t json_size = 0, blob_size = 0;
        NetPimpl::check(anh_dnn_envelope_unpack(bytes.data(), bytes.size(), &json, &json_size, &t.downscaling, &blob, &blob_size));
        const std::string classes_json(json, json_size), net_bytes(static_cast<const char*>(blob), blob_size);
        anh_free(json); anh_free(blob);
        std::cout << "Deserializing annonet, downscaling factor = " << t.downscaling << std::endl;
        std::istringstream stream(net_bytes);
        t.net.Deserialize(stream, fp32 ? ANH_FP32 : ANH_BF16);
        t.classes = parse_anno_classes(classes_json);
        if (t.classes.size() < 2) throw std::runtime_error("at least two classes are needed");
        anh_net_config cfg;
        NetPimpl::check(anh_runtime_config(t.net.handle(), &cfg));
        if ((size_t)cfg.classes != t.classes.size()) throw std::runtime_error("the net's class count differs from the anno classes of the .dnn file");
        return t;
    }
};

// ---- stage 1: readers ----------------------------------------------------------------------------------------------------
class ImageReaders {
  public:
    // resize_images = false: the images stay at their original size (annonet_infer_scaled shrinks them on the GPU)
    ImageReaders(const std::vector<image_filenames_type>& files, int threads, const std::vector<AnnoClass>& classes, double downscaling, bool resize_images)
        : todo_(std::max<size_t>(files.size(), 1)), done_((size_t)std::max(threads, 1)) {
        for (const auto& f : files) todo_.enqueue(f);
        for (int i = 0; i < std::max(threads, 1); ++i)
            pool_.emplace_back([this, &classes, downscaling, resize_images] {
                image_filenames_type names;
                while (todo_.dequeue(names)) if (!done_.enqueue(read_sample(names, classes, false, downscaling, resize_images))) break;
            });
    }
    ~ImageReaders() { todo_.disable(); done_.disable(); for (auto& t : pool_) if (t.joinable()) t.join(); }
    sample_type next() {   // samples arrive in completion order; each carries its own file names
        sample_type s;
        if (!done_.dequeue(s)) throw std::runtime_error("the image readers stopped");
        if (!s.error.empty()) throw std::runtime_error(s.error);
        return s;
    }

  private:
    anh_host::pipe<image_filenames_type> todo_;
    anh_host::pipe<sample_type> done_;
    std::vector<std::thread> pool_;
};

// ---- stage 3: writers ----------------------------------------------------------------------------------------------------
struct LabelMapToWrite {
    std::string path;
    int width = 0, height = 0;          // of the ORIGINAL image: the map is resized back before it is painted (:409-411)
    dlib::matrix<uint16_t> labels;
};

class ResultWriters {
  public:
    ResultWriters(int threads, size_t expected, const std::vector<AnnoClass>& classes) : jobs_((size_t)std::max(threads, 1)), outcomes_(std::max<size_t>(expected, 1)) {
        for (int i = 0; i < std::max(threads, 1); ++i)
            pool_.emplace_back([this, &classes] {
                LabelMapToWrite job;
                dlib::matrix<dlib::rgb_alpha_pixel> painted;
                while (jobs_.dequeue(job)) {
                    bool ok = true;
                    try {
                        if (job.labels.nc() != job.width || job.labels.nr() != job.height) resize_label_image(job.labels, job.width, job.height);   // (a map that annonet_infer_scaled blew up already has the size)
                        painted.set_size(job.labels.nr(), job.labels.nc());
                        auto out = painted.begin();
                        for (const uint16_t label : job.labels) *out++ = label < classes.size() ? classes[label].rgba_label : rgba_ignore_label;   // (65535: an all-NaN pixel)
                        save_png(painted, job.path);
                    } catch (std::exception& e) { std::cerr << e.what() << std::endl; ok = false; }
                    outcomes_.enqueue(ok);
                }
            });
    }
    ~ResultWriters() { jobs_.disable(); outcomes_.disable(); for (auto& t : pool_) if (t.joinable()) t.join(); }
    void submit(LabelMapToWrite job) { jobs_.enqueue(std::move(job)); ++submitted_; }
    void wait_for_all() {
        bool all_ok = true;
        for (size_t i = 0; i < submitted_; ++i) { bool ok = true; outcomes_.dequeue(ok); all_ok = all_ok && ok; }
        if (!all_ok) throw std::runtime_error("some result images could not be written");
    }

  private:
    anh_host::pipe<LabelMapToWrite> jobs_;
    anh_host::pipe<bool> outcomes_;
    std::vector<std::thread> pool_;
    size_t submitted_ = 0;
};

// ---- the tool's own clock (annonet_infer_main.cpp:442-444,466-480,498-507) -----------------------------------------------------------
struct InferenceClock {
    using us = std::chrono::microseconds;
    us all{0}, after_first{0}, slowest_after_first{0};
    size_t images = 0;
    void record(us d) {
        all += d;
        if (images++ > 0) { after_first += d; slowest_after_first = std::max(slowest_after_first, d); }   // the first image pays the warm-up
    }
    // a batch of `count` images (--image-batch): its duration in equal parts to its images; the first BATCH pays the warm-up
    void record_batch(us d, size_t count) {
        all += d;
        if (images > 0) { after_first += d; slowest_after_first = std::max(slowest_after_first, us(d.count() / (long long)count)); }
        else first_batch_images = count;
        images += count;
    }
    size_t first_batch_images = 1;
    void report(double wall_seconds) const {
        std::cout << "\nAll " << images << " images processed in " << wall_seconds << " seconds! (actual inference: " << all.count() / 1000000.0 << " seconds)" << std::endl;
        if (images > first_batch_images)
            std::cout << "Processing time excluding the first image: average = " << after_first.count() / 1000.0 / (images - first_batch_images) << " ms, max = " << slowest_after_first.count() / 1000.0
                      << " ms" << std::endl;
    }
};

int run(const Settings& settings) {
    if (!settings.devices.empty()) NetPimpl::SetDevices(settings.devices);
    TrainedNet trained = TrainedNet::load(settings.dnn_file, settings.precision == "fp32");
    const std::vector<double> gains = per_class_values(settings.gain_args, trained.classes.size());
    const std::vector<double> detection_levels = per_class_values(settings.detection_args, trained.classes.size());
    echo_per_class("Using gains:", gains);
    echo_per_class("Using detection levels:", detection_levels);

    const std::vector<image_filenames_type> files = find_image_files(settings.directory, false);
    const int overlap = NetPimpl::TrainingNet::GetRequiredInputDimension();   // tiles overlap by one receptive field (:421-427)
    tiling::parameters tiles;
    tiles.max_tile_width = settings.max_tile_w; tiles.max_tile_height = settings.max_tile_h;
    tiles.overlap_x = tiles.overlap_y = overlap;
    if (tiles.max_tile_width < overlap || tiles.max_tile_height < overlap) throw std::runtime_error("the maximum tile size must not be smaller than the net's required input dimension");

    ConfusionMatrix per_pixel(trained.classes.size()), per_region(trained.classes.size());
    RegionScorer region_scorer;
    size_t labelled_pixels = 0;
    InferenceClock clock;
    annonet_infer_temp scratch;
    // --write-regions: the table belongs to the map at the net's resolution, whoever shrinks the image: the readers (--host-resize, then
    // annonet_infer_regions() sees the shrunk image) or the GPU (annonet_infer_regions_scaled(), which labels before it blows the map up)
    const bool resize_on_gpu = trained.downscaling != 1.0 && !settings.host_resize;
    {
        ImageReaders readers(files, settings.readers, trained.classes, trained.downscaling, !resize_on_gpu);
        ResultWriters writers(settings.writers, files.size(), trained.classes);
        const auto started = std::chrono::steady_clock::now();
        // both matrices are scored at the net's resolution (the ground truth was resized to it, annonet.cpp:160-166)
        auto score = [&](const sample_type& sample, const dlib::matrix<uint16_t>& scored) {
            for (const auto& cls_points : sample.labeled_points_by_class) {   // per-pixel score on the annotated pixels (:482-490)
                for (const dlib::point& p : cls_points.second) per_pixel.add(cls_points.first, scored(p.y(), p.x()));
                labelled_pixels += cls_points.second.size();
            }
            region_scorer.score(per_region, sample, scored);
        };
        // --gpu-score: the same counts by ONE annonet_score() call over the samples that have a mask (the host scorer returns early for the
        // others); truth = the sample's label_image, result = the map `score` would be handed, both at the net's resolution
        const int class_count = (int)trained.classes.size();
        annonet_score_counts counted;
        auto score_on_gpu = [&](const std::vector<const sample_type*>& samples, const std::vector<const dlib::matrix<uint16_t>*>& scored) {
            std::vector<const dlib::matrix<uint16_t>*> truth_maps, result_maps;
            for (size_t j = 0; j < samples.size(); ++j) {
                if (samples[j]->labeled_points_by_class.empty()) continue;
                if (samples[j]->label_image.nr() != scored[j]->nr() || samples[j]->label_image.nc() != scored[j]->nc()) throw std::runtime_error("ground truth and result sizes differ");
                truth_maps.push_back(&samples[j]->label_image);
                result_maps.push_back(scored[j]);
            }
            if (truth_maps.empty()) return;
            annonet_score(trained.net, truth_maps, result_maps, class_count, counted);
            const size_t k = (size_t)class_count;
            for (size_t i = 0; i < truth_maps.size(); ++i) {
                for (size_t t = 0; t < k; ++t)
                    for (size_t p = 0; p < k; ++p) {
                        per_pixel.add(t, p, (size_t)counted.per_pixel[(i * k + t) * k + p]);
                        per_region.add(t, p, (size_t)counted.per_region[(i * k + t) * k + p]);
                    }
                labelled_pixels += (size_t)counted.labelled[i];
            }
        };
        auto result_for = [](const sample_type& sample) {
            LabelMapToWrite result;
            result.path = sample.image_filenames.image_filename + "_result.png";
            result.width = sample.original_width; result.height = sample.original_height;
            return result;
        };
        // --image-batch N > 1: up to N consecutive samples of one size wait here and go through annonet_infer_batch() together; a sample
        // of another size flushes them first.  Where the GPU resizes (a factor other than 1 without --host-resize) the samples come at
        // their ORIGINAL size, the groups form on it and go through annonet_infer_scaled_batch().  --write-regions takes the same groups
        // through the matching regions form, which labels the blobs of the whole group by one batched call.
        const bool batched = settings.image_batch > 1;
        std::vector<sample_type> pending;
        auto flush = [&] {
            if (pending.empty()) return;
            std::vector<NetPimpl::input_type> images;
            for (sample_type& s : pending) images.push_back(std::move(s.input_image));
            std::vector<dlib::matrix<uint16_t>> maps;
            const auto t0 = std::chrono::steady_clock::now();
            if (resize_on_gpu && settings.write_regions) annonet_infer_regions_scaled_batch(trained.net, images, trained.downscaling, maps, scratch, gains, detection_levels, tiles);
            else if (resize_on_gpu) annonet_infer_scaled_batch(trained.net, images, trained.downscaling, maps, scratch, gains, detection_levels, tiles);
            else if (settings.write_regions) annonet_infer_regions_batch(trained.net, images, maps, scratch, gains, detection_levels, tiles);
            else annonet_infer_batch(trained.net, images, maps, scratch, gains, detection_levels, tiles);
            clock.record_batch(std::chrono::duration_cast<InferenceClock::us>(std::chrono::steady_clock::now() - t0), pending.size());
            if (settings.gpu_score) {
                std::vector<const sample_type*> samples;
                std::vector<const dlib::matrix<uint16_t>*> scored;
                for (size_t j = 0; j < pending.size(); ++j) { samples.push_back(&pending[j]); scored.push_back(resize_on_gpu ? &scratch.scaled_result_images[j] : &maps[j]); }
                score_on_gpu(samples, scored);
            }
            for (size_t j = 0; j < pending.size(); ++j) {
                LabelMapToWrite result = result_for(pending[j]);
                result.labels = std::move(maps[j]);
                if (!settings.gpu_score) score(pending[j], resize_on_gpu ? scratch.scaled_result_images[j] : result.labels);
                if (settings.write_regions)
                    write_regions_csv(pending[j].image_filenames.image_filename + "_result_regions.csv", scratch.regions_per_image[j], trained.classes, trained.downscaling);
                writers.submit(std::move(result));
            }
            pending.clear();
        };
        for (size_t i = 0; i < files.size(); ++i) {
            std::cout << "\rProcessing image " << (i + 1) << " of " << files.size() << "...";
            sample_type sample = readers.next();
            if (batched) {
                if (!pending.empty() && (sample.input_image.nr() != pending[0].input_image.nr() || sample.input_image.nc() != pending[0].input_image.nc())) flush();
                pending.push_back(std::move(sample));
                if ((int)pending.size() == settings.image_batch) flush();
                continue;
            }
            LabelMapToWrite result = result_for(sample);

            const auto t0 = std::chrono::steady_clock::now();
            if (resize_on_gpu && settings.write_regions) annonet_infer_regions_scaled(trained.net, sample.input_image, trained.downscaling, result.labels, scratch, gains, detection_levels, tiles);
            else if (resize_on_gpu) annonet_infer_scaled(trained.net, sample.input_image, trained.downscaling, result.labels, scratch, gains, detection_levels, tiles);
            else if (settings.write_regions) annonet_infer_regions(trained.net, sample.input_image, result.labels, scratch, gains, detection_levels, tiles);
            else annonet_infer(trained.net, sample.input_image, result.labels, scratch, gains, detection_levels, tiles);
            clock.record(std::chrono::duration_cast<InferenceClock::us>(std::chrono::steady_clock::now() - t0));
            if (settings.gpu_score) score_on_gpu({&sample}, {resize_on_gpu ? &scratch.scaled_result_image : &result.labels});
            else score(sample, resize_on_gpu ? scratch.scaled_result_image : result.labels);
            if (settings.write_regions) write_regions_csv(sample.image_filenames.image_filename + "_result_regions.csv", scratch.regions, trained.classes, trained.downscaling);
            writers.submit(std::move(result));
        }
        flush();
        clock.report(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - started).count() / 1000.0);
        writers.wait_for_all();
        std::cout << "All result images written!" << std::endl;
    }
    if (labelled_pixels) {
        std::cout << std::endl << "Confusion matrix per pixel:" << std::endl;
        per_pixel.print(std::cout, trained.classes);
        std::cout << std::endl << "Confusion matrix per region (two-way):" << std::endl;
        per_region.print(std::cout, trained.classes);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 1) {
        std::cout << "You call this program like this: " << std::endl << "./annonet_infer_hip /path/to/image/data" << std::endl << std::endl
                  << "You will also need a trained 'annonet.dnn' file. " << std::endl << std::endl;
        return 1;
    }
    Settings settings;
    try {
        settings = read_command_line(argc, argv);
        std::cout << "Input directory = " << settings.directory << std::endl;
    } catch (std::exception& e) {
        std::cerr << e.what() << std::endl << std::endl << usage_text() << std::endl;
        return 2;
    }
    try { return run(settings); }
    catch (std::exception& e) { std::cout << e.what() << std::endl; return 1; }
}
