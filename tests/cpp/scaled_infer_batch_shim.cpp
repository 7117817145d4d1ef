// annonet_infer_scaled_batch() of the drop-in header (include/annonet_infer_hip.h) as a host program would call it for a folder of
// frames of one size and a net trained with a downscaling factor.  tests/test_gpu_scaled_infer_batch.py compares the files this writes
// with the Python mirror's result.
//   scaled_infer_batch_shim net.bin images.raw n height width factor tile out-prefix  ->  <prefix>.labels.raw ([n][height][width] u16),
//   <prefix>.scaled.raw ([n][sh][sw] u16, annonet_infer_temp::scaled_result_images), <prefix>.planes.raw (the planes of the last image
//   at the net's resolution, annonet_infer_temp::blended_output)
#define ANNONET_HIP_NO_DLIB
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "annonet_infer_hip.h"

int main(int argc, char** argv) try {
    if (argc != 9) throw std::runtime_error("usage: scaled_infer_batch_shim net.bin images.raw n height width factor tile out-prefix");
    std::ifstream net_file(argv[1], std::ios::binary);
    NetPimpl::RuntimeNet net;
    net.Deserialize(net_file, ANH_FP32);
    const int n = std::atoi(argv[3]), height = std::atoi(argv[4]), width = std::atoi(argv[5]), tile = std::atoi(argv[7]);
    const double factor = std::atof(argv[6]);
    std::ifstream image_file(argv[2], std::ios::binary);
    const std::string pixels((std::istreambuf_iterator<char>(image_file)), std::istreambuf_iterator<char>());
    const size_t one = (size_t)height * width * NetPimpl::kInputChannels;
    if (n < 1 || pixels.size() != one * n) throw std::runtime_error("raw image file has the wrong size");
    std::vector<NetPimpl::input_type> images((size_t)n);
    for (int i = 0; i < n; ++i) {
        images[i].set_size(height, width);
        std::memcpy(&*images[i].begin(), pixels.data() + one * i, one);
    }

    tiling::parameters tiles;
    tiles.max_tile_width = tiles.max_tile_height = tile;
    tiles.overlap_x = tiles.overlap_y = 10;
    std::vector<dlib::matrix<uint16_t>> results;
    annonet_infer_temp temp;
    temp.keep_blended_output = true;
    annonet_infer_scaled_batch(net, images, factor, results, temp, {}, {}, tiles);

    const std::string prefix = argv[8];
    std::ofstream labels(prefix + ".labels.raw", std::ios::binary), scaled(prefix + ".scaled.raw", std::ios::binary), planes(prefix + ".planes.raw", std::ios::binary);
    for (const auto& map : results) labels.write(reinterpret_cast<const char*>(&*map.begin()), (std::streamsize)(map.size() * 2));
    for (const auto& map : temp.scaled_result_images) scaled.write(reinterpret_cast<const char*>(&*map.begin()), (std::streamsize)(map.size() * 2));
    for (const auto& plane : temp.blended_output) planes.write(reinterpret_cast<const char*>(&*plane.begin()), (std::streamsize)(plane.size() * 4));
    std::cout << results.size() << ' ' << results[0].nr() << ' ' << results[0].nc() << ' ' << temp.scaled_result_images.size() << ' '
              << temp.scaled_result_images[0].nr() << ' ' << temp.scaled_result_images[0].nc() << ' ' << temp.blended_output.size() << std::endl;
    return 0;
} catch (std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
}
