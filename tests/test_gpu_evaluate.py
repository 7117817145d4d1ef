"""Held-out evaluation through the net: RuntimeNet.evaluate_device / evaluate and TrainingNet.evaluate / evaluate_device.

fp32: the reference is tests/eval_ref.py on the oracle's orc_forward logits, which the fp32 inference path reproduces bit for bit, so
counts, matrices and predicted maps are exact and the loss meets the bar of tests/test_gpu_eval_logits.py (2e-5 * max(1, |want / pixels|)
on loss_sum / pixels).  19 windows of 35 x 35 are more than one forward batch (Engine::kMaxTileBatch = 16): every image still equals its
single call bit for bit.  bf16 introduces no tolerance: evaluate_device must equal the tally (eval_logits_device) on the logits
forward_device leaves for the same windows, bit for bit.  The trainer's calls equal snapshot + RuntimeNet.evaluate bit for bit and
leave a training run exactly where it was: two trainers with one seed, one of which evaluates after every step, end with identical
state files (parameters, momentum, running statistics and their update counts, recorded and pending losses, learning rate, step count)."""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import eval_ref as er
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

NETS = {"two_levels": (2, 3, 3, 0.25, 4), "one_level": (1, 3, 3, 0.25, 4)}   # the benchmark net has two levels
CASES = [(35, 35, 5), (51, 51, 5), (35, 51, 5), (35, 35, 19)]


@functools.lru_cache(maxsize=None)
def windows(h, w, n, classes=3):
    rng = np.random.default_rng(h * 1000 + w * 10 + n)
    images = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    labels = rng.integers(0, classes, (n, h, w)).astype(np.uint16)
    labels[rng.random((n, h, w)) < 0.1] = aa.LABEL_IGNORE
    weights = rng.uniform(0.5, 2.0, (n, h, w)).astype(np.float32)
    weights[rng.random((n, h, w)) < 0.1] = 0
    for a in (images, labels, weights):
        a.setflags(write=False)
    return images, labels, weights


@functools.lru_cache(maxsize=None)
def oracle_net(name):
    o = OracleNet(*NETS[name])
    p, r = random_params(o, 3)
    o.params[:], o.running[:] = p, r
    return o, p, r


@functools.lru_cache(maxsize=None)
def expected(name, h, w, n):
    images, labels, weights = windows(h, w, n)
    return er.eval_ref(oracle_net(name)[0].forward(np.array(images)), labels, weights)


@functools.lru_cache(maxsize=None)
def runtime(name, precision):
    _, p, r = oracle_net(name)
    net = aa.RuntimeNet(aa.net_config(*NETS[name], precision))
    net.set_params(p, r)
    return net


def on_device(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(np.array(a.view(np.int16) if a.dtype == np.uint16 else a)).cuda()
    torch.cuda.current_stream().synchronize()
    return t


def device_evaluate(net, images, labels, weights, **kw):
    """evaluate_device (a RuntimeNet's or a TrainingNet's) on windows torch uploads, with the predicted maps read back"""
    import torch
    n, h, w = labels.shape
    d = [on_device(images), on_device(labels), on_device(weights) if weights is not None else None]
    pred = torch.full((n, h, w), 0x1234, dtype=torch.int16, device="cuda")
    torch.cuda.current_stream().synchronize()
    r = net.evaluate_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else 0, n, h, w, d_predicted_ptr=pred.data_ptr(), prefill=0xA5, **kw)
    r.predicted = pred.cpu().numpy().view(np.uint16)
    return r


def same_bits(a, b, what=""):
    assert a.per_image.tobytes() == b.per_image.tobytes(), what
    np.testing.assert_array_equal(a.confusion, b.confusion, err_msg=what)
    np.testing.assert_array_equal(a.predicted, b.predicted, err_msg=what)


def wlabels(labels, weights):
    out = []
    for l, w in zip(labels, weights):
        a = np.zeros(l.shape, dtype=aa.netpimpl.WLABEL)
        a["label"], a["weight"] = l, w
        out.append(a)
    return out


@pytest.mark.parametrize("h,w,n", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(NETS))
def test_fp32_evaluation_equals_the_reference_on_the_oracle_logits(name, h, w, n):
    assert aa.RuntimeNet.GetRecommendedInputDimension(NETS[name][0], h) == h and aa.RuntimeNet.GetRecommendedInputDimension(NETS[name][0], w) == w
    images, labels, weights = windows(h, w, n)
    want = expected(name, h, w, n)
    net = runtime(name, aa.ANH_FP32)
    r = device_evaluate(net, images, labels, weights)
    for key in ("counted", "unclassified"):
        np.testing.assert_array_equal(r.per_image[key], want[key], err_msg=key)
    np.testing.assert_array_equal(r.confusion, want["confusion"])
    np.testing.assert_array_equal(r.predicted, want["predicted"])
    assert (r.confusion.sum(axis=(1, 2)) + r.per_image["unclassified"] == r.per_image["counted"]).all()
    pixels = h * w
    for got, ref in zip(r.per_image["loss_sum"], want["loss_sum"]):
        print(f"loss per pixel {name} {h}x{w} n={n}: got {got / pixels:.9g} want {ref / pixels:.9g}")
        assert abs(got / pixels - ref / pixels) <= 2e-5 * max(1.0, abs(ref / pixels))
    for got, ref in zip(r.per_image["weight_sum"], want["weight_sum"]):
        assert abs(got - ref) <= 1e-12 * abs(ref)
    assert abs(r.mean_loss() - er.mean_loss(want)) <= 2e-5 * max(1.0, abs(er.mean_loss(want)))
    assert r.pixel_accuracy() == er.pixel_accuracy(want)
    np.testing.assert_array_equal(r.class_iou(), er.class_iou(want))
    if n == 19:   # two forward batches: every image equals its single call, doubles included
        for i in range(n):
            single = device_evaluate(net, images[i:i + 1], labels[i:i + 1], weights[i:i + 1])
            assert single.per_image[0].tobytes() == r.per_image[i].tobytes(), i
            np.testing.assert_array_equal(single.confusion[0], r.confusion[i])
            np.testing.assert_array_equal(single.predicted[0], r.predicted[i])


@pytest.mark.parametrize("h,w,n", [(35, 51, 5), (35, 35, 19)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(NETS))
def test_bf16_evaluation_equals_the_tally_on_the_logits_forward_device_leaves(name, h, w, n):
    import torch
    images, labels, weights = windows(h, w, n)
    net = runtime(name, aa.ANH_BF16)
    r = device_evaluate(net, images, labels, weights)
    K = NETS[name][2]
    d_img, d_lab, d_w = on_device(images), on_device(labels), on_device(weights)
    logits = torch.full((n, K, h, w), float("nan"), dtype=torch.float32, device="cuda")
    pred = torch.full((n, h, w), 0x1234, dtype=torch.int16, device="cuda")
    torch.cuda.current_stream().synchronize()
    aa._lib.check(net.L.anh_runtime_forward_device(net.h, d_img.data_ptr(), n, h, w, logits.data_ptr()))
    t = aa.eval_logits_device(net, logits.data_ptr(), d_lab.data_ptr(), d_w.data_ptr(), n, K, h, w, d_predicted_ptr=pred.data_ptr(), prefill=0x11)
    t.predicted = pred.cpu().numpy().view(np.uint16)
    same_bits(r, t, "bf16")
    assert int(r.per_image["counted"].sum()) == int((labels != aa.LABEL_IGNORE).sum()) and np.isfinite(r.per_image["loss_sum"]).all()


@pytest.mark.parametrize("precision", [aa.ANH_FP32, aa.ANH_BF16], ids=["fp32", "bf16"])
def test_the_host_form_equals_the_device_form(precision):
    images, labels, weights = windows(35, 51, 5)
    net = runtime("two_levels", precision)
    dev = device_evaluate(net, images, labels, weights)
    host = net.evaluate(list(images), wlabels(labels, weights), want_predicted=True)
    same_bits(dev, host, "host form")
    gains = [0.0, 3.0, -2.0]
    same_bits(device_evaluate(net, images, labels, weights, gains=gains), net.evaluate(list(images), wlabels(labels, weights), gains=gains, want_predicted=True), "gains")
    without = net.evaluate(list(images), wlabels(labels, weights))
    assert without.predicted is None and without.per_image.tobytes() == host.per_image.tobytes()


def test_a_label_beyond_the_classes_is_invalid_through_the_net():
    images, labels, weights = windows(35, 35, 5)
    bad = np.array(labels)
    bad[3, 7, 9] = 3
    net = runtime("one_level", aa.ANH_FP32)
    with pytest.raises(aa.AnnonetHipError) as e:
        device_evaluate(net, images, bad, weights)
    assert e.value.code == 1
    np.testing.assert_array_equal(device_evaluate(net, images, labels, weights).confusion, expected("one_level", 35, 35, 5)["confusion"])
    with pytest.raises(aa.AnnonetHipError):   # 36 is no input size of a one-level net: refused as forward_device refuses it
        net.evaluate_device(1, 1, 0, 1, 36, 36)


# ---- the trainer's hook ----
D = 35


def make_trainer(precision, seed=5):
    t = aa.TrainingNet(2, 3, precision, seed=seed)
    t.Initialize()
    t.SetNetWidth(0.25, 4)
    t.SetClassCount(3)
    t.SetLearningRate(0.05)
    t.SetLearningRateShrinkFactor(0.5)
    t.SetIterationsWithoutProgressThreshold(6)
    t.SetPreviousLossValuesDumpAmount(2)
    t.SetAllBatchNormalizationRunningStatsWindowSizes(3)
    return t


def batch(seed, n=3):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, D, D, 3), dtype=np.uint8)
    lab = rng.integers(0, 3, (n, D, D)).astype(np.uint16)
    lab[rng.random((n, D, D)) < 0.1] = aa.LABEL_IGNORE
    return list(img), [aa.set_weights(l, 0.5, 0.5) for l in lab]


@pytest.mark.parametrize("precision", [aa.ANH_FP32, aa.ANH_BF16], ids=["fp32", "bf16"])
def test_trainer_evaluate_equals_snapshot_plus_runtime_evaluate(precision):
    t = make_trainer(precision)
    images, labels, weights = windows(35, 51, 5)
    samples, wl = list(images), wlabels(labels, weights)
    before = t.evaluate(samples, wl, want_predicted=True)
    same_bits(before, t.GetRuntimeNet(precision).evaluate(samples, wl, want_predicted=True), "before the first step")
    for i in range(2):
        t.StartTraining(*batch(i))
    for eval_precision in (aa.ANH_FP32, aa.ANH_BF16):          # the evaluation precision need not be the training precision
        got = t.evaluate(samples, wl, precision=eval_precision, want_predicted=True)
        same_bits(got, t.GetRuntimeNet(eval_precision).evaluate(samples, wl, want_predicted=True), f"after two steps, precision {eval_precision}")
        same_bits(got, device_evaluate(t, images, labels, weights, precision=eval_precision), "the trainer's device form")
    after = t.evaluate(samples, wl, want_predicted=True)
    assert after.per_image["loss_sum"].tobytes() != before.per_image["loss_sum"].tobytes()      # the steps changed the weights


@pytest.mark.parametrize("precision", [aa.ANH_FP32, aa.ANH_BF16], ids=["fp32", "bf16"])
def test_evaluating_leaves_the_training_run_where_it_was(precision, tmp_path):
    plain, watched = make_trainer(precision), make_trainer(precision)
    small, large = windows(35, 35, 5), windows(51, 51, 5)       # the batch's window size, and another
    losses = {"plain": [], "watched": []}
    for i in range(6):
        plain.StartTraining(*batch(i))
        watched.StartTraining(*batch(i))
        for images, labels, weights in (small, large):
            watched.evaluate(list(images), wlabels(labels, weights))
        device_evaluate(watched, *small)
        losses["plain"].append(plain.get_last_loss())
        losses["watched"].append(watched.get_last_loss())
    assert losses["plain"] == losses["watched"]
    for a, b in zip(plain.get_params() + (plain.get_momentum(),), watched.get_params() + (watched.get_momentum(),)):
        np.testing.assert_array_equal(a, b)
    assert plain.GetLearningRate() == watched.GetLearningRate() and plain.step_count() == watched.step_count() == 6
    plain.save_state(str(tmp_path / "plain.dat"))
    watched.save_state(str(tmp_path / "watched.dat"))
    assert (tmp_path / "plain.dat").read_bytes() == (tmp_path / "watched.dat").read_bytes()     # schedule history, pending losses and bn update counts included
    for i in range(6, 8):                                        # and the runs stay together afterwards
        plain.StartTraining(*batch(i))
        watched.StartTraining(*batch(i))
    np.testing.assert_array_equal(plain.get_params()[0], watched.get_params()[0])
