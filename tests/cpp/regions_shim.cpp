// annonet_infer_regions() of the drop-in header (include/annonet_infer_hip.h) as a host program would call it: annonet_infer() plus the
// connected blobs of its unfiltered label map and one table row per blob (annonet_infer.cpp:194-223).  tests/test_regions_host.py compiles
// this; tests/test_gpu_infer_regions.py compares the files it writes with the Python mirror's result.
//   regions_shim net.bin image.raw height width det0,det1,... out-prefix  ->  <prefix>.labels.raw, <prefix>.blobs.raw, <prefix>.regions.raw, <prefix>.planes.raw
#define ANNONET_HIP_NO_DLIB
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "annonet_infer_hip.h"

int main(int argc, char** argv) try {
    if (argc != 7) throw std::runtime_error("usage: regions_shim net.bin image.raw height width det0,det1,...|- out-prefix");
    std::ifstream net_file(argv[1], std::ios::binary);
    NetPimpl::RuntimeNet net;
    net.Deserialize(net_file, ANH_FP32);
    const int height = std::atoi(argv[3]), width = std::atoi(argv[4]);
    std::vector<double> detection_levels;
    if (std::strcmp(argv[5], "-") != 0) {
        std::stringstream list(argv[5]);
        for (std::string item; std::getline(list, item, ',');) detection_levels.push_back(std::atof(item.c_str()));
    }
    std::ifstream image_file(argv[2], std::ios::binary);
    const std::string pixels((std::istreambuf_iterator<char>(image_file)), std::istreambuf_iterator<char>());
    if (pixels.size() != (size_t)height * width * NetPimpl::kInputChannels) throw std::runtime_error("raw image file has the wrong size");
    NetPimpl::input_type image;
    image.set_size(height, width);
    std::memcpy(&*image.begin(), pixels.data(), pixels.size());

    tiling::parameters tiles;
    tiles.max_tile_width = tiles.max_tile_height = 96;
    tiles.overlap_x = tiles.overlap_y = NetPimpl::TrainingNet::GetRequiredInputDimension();
    dlib::matrix<uint16_t> result;
    annonet_infer_temp temp;
    temp.keep_blended_output = true;
    temp.keep_connected_blobs = true;
    annonet_infer_regions(net, image, result, temp, {}, detection_levels, tiles);
    if (!temp.detection_seeds.empty()) throw std::runtime_error("detection_seeds is documented to stay empty");

    const std::string prefix = argv[6];
    std::ofstream labels(prefix + ".labels.raw", std::ios::binary), blobs(prefix + ".blobs.raw", std::ios::binary),
        regions(prefix + ".regions.raw", std::ios::binary), planes(prefix + ".planes.raw", std::ios::binary);
    labels.write(reinterpret_cast<const char*>(&*result.begin()), (std::streamsize)(result.size() * 2));
    blobs.write(reinterpret_cast<const char*>(&*temp.connected_blobs.begin()), (std::streamsize)(temp.connected_blobs.size() * sizeof(unsigned int)));
    regions.write(reinterpret_cast<const char*>(temp.regions.data()), (std::streamsize)(temp.regions.size() * sizeof(anh_region)));
    for (const auto& plane : temp.blended_output) planes.write(reinterpret_cast<const char*>(&*plane.begin()), (std::streamsize)(plane.size() * 4));
    std::cout << result.nr() << ' ' << result.nc() << ' ' << temp.connected_blobs.nr() << ' ' << temp.connected_blobs.nc() << ' ' << temp.regions.size() << ' '
              << sizeof(anh_region) << std::endl;
    return 0;
} catch (std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
}
