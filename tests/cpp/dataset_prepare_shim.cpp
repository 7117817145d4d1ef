// dataset_prepare_shim.cpp — NetPimpl::Dataset::Prepare and TrainingNet::StartTrainingOnPickedCrops against the headers alone: one image,
// both label filters, one optimiser step on crops whose centres the device picks.  Without a GPU the calls must fail the reference's
// way: an exception.
#define ANNONET_HIP_NO_DLIB
#include <cmath>
#include <cstdio>
#include <limits>

#include "NetPimpl.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    anh_dataset_info two{};   // anh_resolve_pick is host logic: it answers with or without a GPU
    two.present = 2; two.classes[0] = 1; two.classes[1] = 4; two.counts[0] = 10; two.counts[1] = 3;
    uint16_t label = 0; uint64_t k = 0;
    NetPimpl::check(anh_resolve_pick(&two, 5u, 11u, &label, &k));
    CHECK(label == 4 && k == 2);

    if (anh_device_count() == 0) {
        bool threw = false;
        try { NetPimpl::Dataset d; }
        catch (const std::exception& ex) { threw = true; std::printf("no GPU: %s\n", ex.what()); }
        CHECK(threw);
        std::printf("dataset prepare shim ok (host logic only)\n");
        return 0;
    }
    const int rf = NetPimpl::TrainingNet::GetRequiredInputDimension();
    const int dim = NetPimpl::RuntimeNet::GetRecommendedInputDimension(rf);
    const long H = 3 * dim, W = 4 * dim + 3;
    NetPimpl::input_type image;
    dlib::matrix<uint16_t> labels;
    image.set_size(H, W);
    labels.set_size(H, W);
    long ones = 0;
    for (long r = 0; r < H; ++r)
        for (long c = 0; c < W; ++c) {
            image(r, c) = dlib::rgb_pixel{(unsigned char)(r * 7 + c), (unsigned char)(c * 3), (unsigned char)(r + c)};
            labels(r, c) = (uint16_t)((r + c) % 11 == 0 ? 65535 : (r / 9 + c / 9) % 3);
            ones += labels(r, c) == 1;
        }
    NetPimpl::Dataset data;
    const int index = data.Add(image, labels);
    const uint64_t before = data.ResidentBytes();
    const double inf = std::numeric_limits<double>::infinity();
    const anh_dataset_info info = data.Prepare(index, {2}, 1000.0, inf, inf, rf);
    CHECK(info.present == 2 && info.classes[0] == 0 && info.classes[1] == 1 && (long)info.counts[1] == ones);
    CHECK(info.ignored_by_class > 0 && info.ignored_by_size == 0);
    CHECK(data.ResidentBytes() == before + 4u * 2u * (uint64_t)((H * W + 1023) / 1024));

    NetPimpl::TrainingNet t;
    t.Initialize();
    t.SetNetWidth(0.25, 4);
    t.SetClassCount(3);
    t.SetLearningRate(0.05);
    std::vector<anh_crop_spec> crops(4);
    std::vector<anh_crop_draw> draws(4);
    for (int i = 0; i < 4; ++i) {
        crops[i] = anh_crop_spec{};
        crops[i].image = index; crops[i].brightness_change = 1.0; crops[i].flip_left_right = i & 1;
        draws[i] = anh_crop_draw{(uint32_t)i, 1000003ull * (uint64_t)(i + 1), 17u * (uint32_t)i, 0xFFFFFFFFu - (uint32_t)i};
    }
    t.StartTrainingOnPickedCrops(data, crops, draws, dim, 0.5, 0.5);
    const double loss = anh_trainer_get_last_loss(t.handle());
    CHECK(std::isfinite(loss) && loss > 0 && anh_trainer_get_step_count(t.handle()) == 1);
    bool threw = false;
    try { t.StartTrainingOnPickedCrops(data, crops, {}, dim, 0.5, 0.5); } catch (const std::exception&) { threw = true; }   // one draw per crop
    CHECK(threw);
    std::printf("one step on 4 picked crops: loss %.6f\n", loss);
    std::printf("dataset prepare shim ok\n");
    return 0;
}
