// annonet_infer_regions_batch(), annonet_infer_regions_scaled() and annonet_infer_regions_scaled_batch() of the drop-in header
// (include/annonet_infer_hip.h) as a host program would call them.  tests/test_regions_batch_host.py compiles this;
// tests/test_gpu_infer_regions_batch.py compares the files it writes with the Python mirrors' results.
//   regions_batch_shim net.bin images.raw n height width factor tile_w tile_h det0,det1,...|- out-prefix
// writes, for form in batch (all images, unscaled), scaled (image 0) and sbatch (all images): <prefix>.<form>.labels.raw, .scaled.raw (the
// scaled forms), .blobs.raw, .regions.raw, and prints one line per form: the form, the images, the size of the blob maps and every image's rows
#define ANNONET_HIP_NO_DLIB
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "annonet_infer_hip.h"

namespace {
template <class Matrix>
void append(std::ofstream& out, const Matrix& m) { out.write(reinterpret_cast<const char*>(&*m.begin()), (std::streamsize)(m.size() * sizeof(*m.begin()))); }

void write_form(const std::string& prefix, const char* form, const std::vector<dlib::matrix<uint16_t>>& labels, const std::vector<dlib::matrix<uint16_t>>& scaled,
                const std::vector<dlib::matrix<unsigned int>>& blobs, const std::vector<std::vector<anh_region>>& regions) {
    const std::string base = prefix + "." + form;
    std::ofstream l(base + ".labels.raw", std::ios::binary), s(base + ".scaled.raw", std::ios::binary), b(base + ".blobs.raw", std::ios::binary),
        r(base + ".regions.raw", std::ios::binary);
    for (const auto& m : labels) append(l, m);
    for (const auto& m : scaled) append(s, m);
    for (const auto& m : blobs) append(b, m);
    std::cout << form << ' ' << labels.size() << ' ' << blobs.at(0).nr() << ' ' << blobs.at(0).nc();
    for (const auto& rows : regions) {
        r.write(reinterpret_cast<const char*>(rows.data()), (std::streamsize)(rows.size() * sizeof(anh_region)));
        std::cout << ' ' << rows.size();
    }
    std::cout << std::endl;
}
}  // namespace

int main(int argc, char** argv) try {
    if (argc != 11) throw std::runtime_error("usage: regions_batch_shim net.bin images.raw n height width factor tile_w tile_h det0,det1,...|- out-prefix");
    std::ifstream net_file(argv[1], std::ios::binary);
    NetPimpl::RuntimeNet net;
    net.Deserialize(net_file, ANH_FP32);
    const int n = std::atoi(argv[3]), height = std::atoi(argv[4]), width = std::atoi(argv[5]);
    const double factor = std::atof(argv[6]);
    std::vector<double> detection_levels;
    if (std::strcmp(argv[9], "-") != 0) {
        std::stringstream list(argv[9]);
        for (std::string item; std::getline(list, item, ',');) detection_levels.push_back(std::atof(item.c_str()));
    }
    std::ifstream image_file(argv[2], std::ios::binary);
    const std::string pixels((std::istreambuf_iterator<char>(image_file)), std::istreambuf_iterator<char>());
    const size_t one = (size_t)height * width * NetPimpl::kInputChannels;
    if (n < 1 || pixels.size() != one * (size_t)n) throw std::runtime_error("raw image file has the wrong size");
    std::vector<NetPimpl::input_type> images((size_t)n);
    for (int i = 0; i < n; ++i) {
        images[i].set_size(height, width);
        std::memcpy(&*images[i].begin(), pixels.data() + one * (size_t)i, one);
    }
    tiling::parameters tiles;
    tiles.max_tile_width = std::atoi(argv[7]); tiles.max_tile_height = std::atoi(argv[8]);
    tiles.overlap_x = tiles.overlap_y = 10;
    const std::string prefix = argv[10];

    annonet_infer_temp temp;
    temp.keep_connected_blobs = true;
    std::vector<dlib::matrix<uint16_t>> results;
    annonet_infer_regions_batch(net, images, results, temp, {}, detection_levels, tiles);
    write_form(prefix, "batch", results, {}, temp.connected_blobs_per_image, temp.regions_per_image);

    dlib::matrix<uint16_t> result;
    annonet_infer_regions_scaled(net, images[0], factor, result, temp, {}, detection_levels, tiles);
    write_form(prefix, "scaled", {result}, {temp.scaled_result_image}, {temp.connected_blobs}, {temp.regions});

    annonet_infer_regions_scaled_batch(net, images, factor, results, temp, {}, detection_levels, tiles);
    write_form(prefix, "sbatch", results, temp.scaled_result_images, temp.connected_blobs_per_image, temp.regions_per_image);
    if (!temp.detection_seeds.empty()) throw std::runtime_error("detection_seeds is documented to stay empty");
    return 0;
} catch (std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
}
