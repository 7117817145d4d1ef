// eval_shim.cpp — the evaluation surface of include/NetPimpl.h: NetPimpl::Evaluation's figures on a given matrix, and (with a GPU)
// TrainingNet::Evaluate against RuntimeNet::Evaluate of a snapshot.  Without a GPU the calls must fail the reference's way: an exception.
#define ANNONET_HIP_NO_DLIB
#include <cmath>
#include <cstdio>
#include <cstring>

#include "NetPimpl.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    NetPimpl::Evaluation e;
    e.classes = 3;
    e.per_image = {{2.0, 1.0, 6, 0}, {4.0, 2.0, 5, 1}};
    e.confusion = {3, 1, 0, 0, 2, 0, 0, 0, 0, /* image 1 */ 1, 0, 0, 2, 1, 0, 0, 0, 0};
    const std::vector<uint64_t> m = e.Matrix();
    CHECK(m.size() == 9 && m[0] == 4 && m[1] == 1 && m[3] == 2 && m[4] == 3 && m[8] == 0);
    CHECK(e.images() == 2 && e.Counted() == 11);
    CHECK(e.MeanLoss() == 2.0);
    CHECK(e.PixelAccuracy() == 7.0 / 11.0);
    const std::vector<double> iou = e.ClassIoU();
    CHECK(iou.size() == 3 && iou[0] == 4.0 / 7.0 && iou[1] == 3.0 / 6.0 && std::isnan(iou[2]));   // class 2 occurs on neither side
    CHECK(e.MeanIoU() == (4.0 / 7.0 + 3.0 / 6.0) / 2);

    const int dim = NetPimpl::RuntimeNet::GetRecommendedInputDimension(NetPimpl::TrainingNet::GetRequiredInputDimension());
    std::vector<NetPimpl::input_type> samples(2);
    std::vector<NetPimpl::training_label_type> labels(2);
    for (int i = 0; i < 2; ++i) {
        samples[i].set_size(dim, dim);
        labels[i].set_size(dim, dim);
        for (long r = 0; r < dim; ++r)
            for (long c = 0; c < dim; ++c) {
                samples[i](r, c) = dlib::rgb_pixel{(unsigned char)(r * 7 + c), (unsigned char)(c * 3 + i), (unsigned char)(r + c)};
                labels[i](r, c) = {(uint16_t)((r + c + i) % 5 == 0 ? 65535 : (r / 8 + c / 8) % 3), 1.f + 0.25f * (float)((r + c) % 3)};
            }
    }
    if (anh_device_count() == 0) {
        bool threw = false;
        try { NetPimpl::TrainingNet t; t.Initialize(); (void)t.Evaluate(samples, labels, ANH_FP32); }
        catch (const std::exception& ex) { threw = true; std::printf("no GPU: %s\n", ex.what()); }
        CHECK(threw);
        std::printf("eval shim ok (host logic only)\n");
        return 0;
    }
    NetPimpl::TrainingNet t;
    NetPimpl::check(anh_trainer_set_precision(t.handle(), ANH_FP32));
    t.Initialize();
    t.SetNetWidth(0.25, 4);
    t.SetClassCount(3);
    t.SetLearningRate(0.05);
    t.StartTraining(samples, labels);
    const NetPimpl::Evaluation a = t.Evaluate(samples, labels, ANH_FP32), b = t.GetRuntimeNet(ANH_FP32).Evaluate(samples, labels);
    CHECK(a.classes == 3 && a.images() == 2 && a.confusion == b.confusion);
    CHECK(std::memcmp(a.per_image.data(), b.per_image.data(), 2 * sizeof(anh_eval_image)) == 0);
    uint64_t cells = 0, unclassified = 0;
    for (uint64_t v : a.confusion) cells += v;
    for (const anh_eval_image& im : a.per_image) unclassified += im.unclassified;
    CHECK(cells + unclassified == a.Counted() && a.Counted() > 0);
    CHECK(std::isfinite(a.MeanLoss()) && a.PixelAccuracy() >= 0 && a.PixelAccuracy() <= 1);
    bool threw = false;
    try { (void)t.Evaluate(samples, labels, ANH_FP32, {1.0}); } catch (const std::exception&) { threw = true; }   // gains: one value per class
    CHECK(threw);
    std::printf("evaluated 2 windows: loss %.6f accuracy %.4f\n", a.MeanLoss(), a.PixelAccuracy());
    std::printf("eval shim ok\n");
    return 0;
}
