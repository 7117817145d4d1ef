// scaled_infer_rate.cpp — the per-image wall time of inference with a downscaled net, as a caller of the C++ headers gets it, in two
// builds of the same loop (tools/scaled_infer_rate.py compiles and runs both):
//   default         the form the tree had before annonet_infer_scaled(): resize_image_bilinear on the host (annonet_host.h), annonet_infer(),
//                   resize_label_image on the host — one thread.  Uses nothing newer, so it links against an older build of the library.
//   -DSCALED_ON_GPU annonet_infer_scaled(): the original image goes up, the original-size map comes down.
// Same seeded image, same net (2 levels, width 1.0, 3 classes, bf16: bench.py's flagship), same tiling, same allocations per image
// (a fresh input copy and fresh result matrices, as a reader thread and annonet_infer() produce them).
//   scaled_infer_rate side factor warmups images  ->  one JSON line
#define ANNONET_HIP_NO_DLIB
#include "annonet_infer_hip.h"   // -I <tree>/include, -I <tree>/annonet_amd/host: the tree the library was built from
#include "annonet_host.h"

#include <algorithm>
#include <chrono>
#include <cstdio>

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char** argv) try {
    if (argc != 5) throw std::runtime_error("usage: scaled_infer_rate side factor warmups images");
    const int side = std::atoi(argv[1]), warmups = std::atoi(argv[3]), images = std::atoi(argv[4]);
    const double factor = std::atof(argv[2]);
    NetPimpl::TrainingNet training_net;
    training_net.Initialize();
    training_net.SetNetWidth(1.0, 1);
    training_net.SetClassCount(3);
    NetPimpl::RuntimeNet net = training_net.GetRuntimeNet();

    NetPimpl::input_type original;
    original.set_size(side, side);
    unsigned seed = 3;
    for (auto& p : original) { seed = seed * 1664525u + 1013904223u; p = dlib::rgb_pixel{(unsigned char)(seed >> 8), (unsigned char)(seed >> 16), (unsigned char)(seed >> 24)}; }
    tiling::parameters tiles;
    tiles.max_tile_width = tiles.max_tile_height = 1024;
    tiles.overlap_x = tiles.overlap_y = NetPimpl::TrainingNet::GetRequiredInputDimension();

    using clock = std::chrono::steady_clock;
    auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::vector<double> total, shrink, infer, enlarge;
    unsigned long long checksum = 0;
    annonet_infer_temp temp;
    for (int i = 0; i < warmups + images; ++i) {
        NetPimpl::input_type image = original;   // what a reader hands over (not timed)
        dlib::matrix<uint16_t> result;
        const auto t0 = clock::now();
#ifdef SCALED_ON_GPU
        annonet_infer_scaled(net, image, factor, result, temp, {}, {}, tiles);
        const auto t1 = t0, t2 = clock::now(), t3 = t2;
#else
        resize_image_bilinear(1.0 / factor, image);                         // read_sample, annonet.cpp:153
        const auto t1 = clock::now();
        annonet_infer(net, image, result, temp, {}, {}, tiles);             // annonet_infer_main.cpp:468
        const auto t2 = clock::now();
        resize_label_image(result, side, side);                             // annonet_infer_main.cpp:409-411
        const auto t3 = clock::now();
#endif
        if (result.nr() != side || result.nc() != side) throw std::runtime_error("the result does not have the original size");
        if (i >= warmups) { total.push_back(ms(t0, t3)); shrink.push_back(ms(t0, t1)); infer.push_back(ms(t1, t2)); enlarge.push_back(ms(t2, t3)); }
        if (i == warmups + images - 1) for (const uint16_t v : result) checksum = checksum * 1099511628211ull + v;
    }
    std::printf("{\"side\": %d, \"factor\": %g, \"warmups\": %d, \"images\": %d, \"median_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f, "
                "\"shrink_ms\": %.3f, \"infer_ms\": %.3f, \"enlarge_ms\": %.3f, \"label_checksum\": \"%016llx\"}\n",
                side, factor, warmups, images, median(total), *std::min_element(total.begin(), total.end()), *std::max_element(total.begin(), total.end()),
                median(shrink), median(infer), median(enlarge), checksum);
    return 0;
} catch (std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
}
