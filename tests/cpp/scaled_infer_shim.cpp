// annonet_infer_scaled() of the drop-in header (include/annonet_infer_hip.h) as a host program would call it for a net trained with a
// downscaling factor: what annonet_infer_main.cpp does with read_sample's resize (annonet.cpp:153), annonet_infer() (:468) and
// resize_label_image (:413), in one call.  tests/test_gpu_scaled_infer.py compares the files this writes with the Python mirror's result.
//   scaled_infer_shim net.bin image.raw height width factor out-prefix  ->  <prefix>.labels.raw, <prefix>.scaled.raw, <prefix>.planes.raw
#define ANNONET_HIP_NO_DLIB
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>

#include "annonet_infer_hip.h"

int main(int argc, char** argv) try {
    if (argc != 7) throw std::runtime_error("usage: scaled_infer_shim net.bin image.raw height width factor out-prefix");
    std::ifstream net_file(argv[1], std::ios::binary);
    NetPimpl::RuntimeNet net;
    net.Deserialize(net_file, ANH_FP32);
    const int height = std::atoi(argv[3]), width = std::atoi(argv[4]);
    const double factor = std::atof(argv[5]);
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
    annonet_infer_scaled(net, image, factor, result, temp, {}, {}, tiles);

    const std::string prefix = argv[6];
    std::ofstream labels(prefix + ".labels.raw", std::ios::binary), scaled(prefix + ".scaled.raw", std::ios::binary), planes(prefix + ".planes.raw", std::ios::binary);
    labels.write(reinterpret_cast<const char*>(&*result.begin()), (std::streamsize)(result.size() * 2));
    scaled.write(reinterpret_cast<const char*>(&*temp.scaled_result_image.begin()), (std::streamsize)(temp.scaled_result_image.size() * 2));
    for (const auto& plane : temp.blended_output) planes.write(reinterpret_cast<const char*>(&*plane.begin()), (std::streamsize)(plane.size() * 4));
    std::cout << result.nr() << ' ' << result.nc() << ' ' << temp.scaled_result_image.nr() << ' ' << temp.scaled_result_image.nc() << ' ' << temp.blended_output.size() << std::endl;
    return 0;
} catch (std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
}
