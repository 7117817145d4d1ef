"""Parity of the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Bars:
  * ANH_FP32 inference: logits, blended planes and label maps BIT-EXACT (every conv output is the same k-ordered
    fmaf chain as the oracle's; bn is folded on the host with the same arithmetic).
  * ANH_FP32 training: loss / gradients / updated parameters within fp32 reduction-order tolerance
    (rtol 2e-3, atol 2e-5*max|g|): batch statistics and filter gradients are sums over up to 10^6 pixels whose
    order differs between the GPU's tree reductions and the oracle's double accumulation.
  * ANH_BF16: bf16 storage + fp32 accumulate; logits within 3% of the logit range, label maps >= 97% equal and every
    mismatching pixel a near-tie (top-2 margin below the logit tolerance); gradients by relative L2 error (< 6%).
"""
import numpy as np
import pytest

import annonet_amd as aa
from conftest import free_port, random_params
from oracle.oracle import OracleNet, IGNORE

pytestmark = pytest.mark.gpu


def pair(levels, in_ch, classes, scaler, minf, precision, seed=7):
    o = OracleNet(levels, in_ch, classes, scaler, minf)
    p, r = random_params(o, seed)
    o.params[:] = p
    o.running[:] = r
    net = aa.RuntimeNet(aa.net_config(levels, in_ch, classes, scaler, minf, precision))
    net.set_params(p, r)
    return o, net


FP32_CASES = [(0, 3, 3, 0.25, 4), (1, 1, 2, 0.25, 4), (2, 3, 3, 0.25, 4), (3, 3, 4, 0.125, 4), (2, 3, 3, 1.0, 1), (2, 1, 3, 0.1, 5)]


@pytest.mark.parametrize("levels,in_ch,classes,scaler,minf", FP32_CASES)
def test_fp32_forward_is_bit_exact(levels, in_ch, classes, scaler, minf):
    o, net = pair(levels, in_ch, classes, scaler, minf, aa.ANH_FP32)
    rng = np.random.default_rng(1)
    d = o.recommended_input_dim(37 if scaler < 1 else 23)
    img = rng.integers(0, 256, (2, d, d + (1 << levels), in_ch), dtype=np.uint8)
    want = o.forward(img)
    got = net.Forward(img)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_forward_rejects_invalid_sizes_and_channels():
    _, net = pair(2, 3, 3, 0.25, 4, aa.ANH_FP32)
    with pytest.raises(aa.AnnonetHipError) as e:
        net.Forward(np.zeros((24, 24, 3), np.uint8))
    assert e.value.code == 1
    with pytest.raises(aa.AnnonetHipError):
        net.Forward(np.zeros((23, 23, 1), np.uint8))
    assert net.Forward(np.zeros((23, 23, 3), np.uint8)).shape == (3, 23, 23)  # handle still usable


def test_serialize_roundtrip_keeps_outputs():
    o, net = pair(1, 3, 3, 0.25, 4, aa.ANH_FP32)
    blob = net.Serialize()
    net2 = aa.RuntimeNet.Deserialize(blob, aa.ANH_FP32)
    img = np.random.default_rng(3).integers(0, 256, (15, 19, 3), dtype=np.uint8)
    np.testing.assert_array_equal(net.Forward(img), net2.Forward(img))
    p, r = net2.get_params()
    np.testing.assert_array_equal(p, o.params)
    np.testing.assert_array_equal(r, o.running)
    with pytest.raises(aa.AnnonetHipError) as e:
        aa.RuntimeNet.Deserialize(blob[:-4], aa.ANH_FP32)
    assert e.value.code == 4


@pytest.mark.parametrize("H,W,max_tile", [(23, 31, 1024), (21, 30, 1024), (90, 140, 64), (130, 75, 57), (5, 3, 1024)])
def test_fp32_tiled_infer_is_bit_exact(H, W, max_tile):
    o, net = pair(1, 3, 3, 0.25, 4, aa.ANH_FP32, seed=9)
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ov = o.required_input_dim()
    want_labels, want_bl = o.infer(img, max_tile=(max_tile, max_tile), overlap=ov, want_blended=True)
    tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
    got_labels, got_bl = aa.annonet_infer(net, img, tiling_parameters=tp, want_blended=True)
    np.testing.assert_array_equal(got_bl, want_bl)
    np.testing.assert_array_equal(got_labels, want_labels)
    gains = [0.0, 0.35, -0.2]
    np.testing.assert_array_equal(aa.annonet_infer(net, img, gains=gains, tiling_parameters=tp),
                                  o.infer(img, gains=gains, max_tile=(max_tile, max_tile), overlap=ov))


def test_caller_tile_list_whose_frames_reach_into_unique_rectangles_is_blended_sequentially():
    """tiling::get_tiles never lets a tile's full rectangle reach into another tile's unique rectangle (the reference asserts `out == 0.f`
    before an assignment, annonet_infer.cpp:158), and the one-launch-per-batch blend relies on it.  A caller's own tile list may break it:
    such a batch must take the per-tile launches — the reference's loop literally (assign, then the later tile's ramp added on top)."""
    import torch
    o, net = pair(1, 3, 3, 0.25, 4, aa.ANH_FP32, seed=9)
    H, W = 40, 90
    img = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    # two tiles with equal windows (one batch); the second one's frame (x = 40..59) covers x = 40..49 of the first one's unique rectangle
    tiles = [((0, 0, 49, H - 1), (0, 0, 49, H - 1)), ((40, 0, W - 1, H - 1), (60, 0, W - 1, H - 1))]
    want_labels, want_bl = o.infer(img, tiles=tiles, want_blended=True)
    assert np.abs(want_bl[:, :, 40:50] - o.infer(img, tiles=tiles[:1], want_blended=True)[1][:, :, 40:50]).max() > 0   # the case is not vacuous
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(img).to(dev)
    d_lab = torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_bl = torch.full((3, H, W), 7.0, dtype=torch.float32, device=dev)   # dirty planes: the call clears what it must
    torch.cuda.synchronize()
    aa.annonet_infer_device(net, d_img.data_ptr(), H, W, d_lab.data_ptr(), d_bl.data_ptr(), tiles=tiles)
    net.synchronize()
    np.testing.assert_array_equal(d_bl.cpu().numpy(), want_bl)
    np.testing.assert_array_equal(d_lab.cpu().numpy().view(np.uint16), want_labels)


def test_infer_detection_levels_and_nan():
    o, net = pair(1, 3, 3, 0.25, 4, aa.ANH_FP32, seed=9)
    img = np.random.default_rng(4).integers(0, 256, (31, 31, 3), dtype=np.uint8)
    for det in ([0.0, 1e9, 1e9], [0.0, 0.0, 0.0], [0.0, 0.5, 0.25], [0.1, 0.0, 2.0]):
        np.testing.assert_array_equal(aa.annonet_infer(net, img, detection_levels=det), o.infer(img, detection_levels=det))
    # blobs that span many 32x32 flood tiles of the device-side filter (large flat regions, ragged image size)
    base = np.random.default_rng(5).integers(0, 256, (6, 7, 3))
    big = np.kron(base, np.ones((27, 25, 1))).astype(np.uint8)[:150, :170]
    labels0 = o.infer(big)
    assert max(np.bincount(labels0.ravel())) > 4000          # there are blobs larger than a few tiles
    for det in ([0.0, 0.05, 0.02], [0.02, 0.3, 0.0], [0.0, 1e9, 0.01]):
        np.testing.assert_array_equal(aa.annonet_infer(net, big, detection_levels=det), o.infer(big, detection_levels=det))
    # all-NaN logits keep the start label 65535 (annonet_infer.cpp:172-183)
    p, r = net.get_params()
    head = aa.net_layers(net.cfg)[-1]
    p[head.b_off:head.b_off + 3] = np.nan
    net.set_params(p, r)
    assert (aa.annonet_infer(net, img) == 65535).all()


def make_batch(rng, n, d, in_ch, classes):
    img = rng.integers(0, 256, (n, d, d, in_ch), dtype=np.uint8)
    lab = rng.integers(0, classes, (n, d, d)).astype(np.uint16)
    lab[rng.random((n, d, d)) < 0.05] = IGNORE
    wl = [aa.set_weights(lab[i], 0.5, 0.5) for i in range(n)]
    w = np.stack([x["weight"] for x in wl])
    return img, lab, w, wl


def trainer_pair(levels, in_ch, classes, scaler, minf, precision, seed=11, lr=0.05):
    o = OracleNet(levels, in_ch, classes, scaler, minf)
    p, r = random_params(o, seed)
    o.params[:] = p
    o.running[:] = r
    o.set_hyper(lr=lr, wd=0.0005, mom=0.9, bn_window=100)
    t = aa.TrainingNet(levels, in_ch, precision)
    t.SetNetWidth(scaler, minf)
    t.SetClassCount(classes)
    t.Initialize()
    t.SetLearningRate(lr)
    t.SetAllBatchNormalizationRunningStatsWindowSizes(100)
    t.set_params(p, r)
    mom = np.random.default_rng(seed).normal(0, 1e-3, o.n_params).astype(np.float32)
    o.momentum[:] = mom
    t.set_momentum(mom)
    return o, t


@pytest.mark.parametrize("levels,in_ch,classes,scaler,minf", [(0, 3, 3, 0.25, 4), (1, 1, 2, 0.25, 4), (2, 3, 3, 0.25, 4), (3, 3, 3, 0.125, 4), (2, 3, 3, 0.1, 5)])
def test_fp32_training_step_matches_oracle(levels, in_ch, classes, scaler, minf):
    o, t = trainer_pair(levels, in_ch, classes, scaler, minf, aa.ANH_FP32)
    rng = np.random.default_rng(2)
    d = o.recommended_input_dim(27)
    img, lab, w, wl = make_batch(rng, 3, d, in_ch, classes)
    want_loss = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    got_loss = t.get_last_loss()
    assert abs(got_loss - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
    g, gw = t.get_grads(), o.grads
    scale = np.abs(gw).max()
    np.testing.assert_allclose(g, gw, rtol=2e-3, atol=2e-5 * scale)
    p, r = t.get_params()
    np.testing.assert_allclose(p, o.params, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(t.get_momentum(), o.momentum, rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(r, o.running, rtol=1e-4, atol=1e-5)
    # per-layer taps: raw conv outputs of the training forward
    for li, L in enumerate(o.layers):
        want = o.layer_output(li, 0)
        got = t.layer_tensor(li, 0)
        if not L.has_bn:
            continue  # the head tap carries the bias; covered by the loss check
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-4 * np.abs(want).max())


@pytest.mark.parametrize("classes", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("precision", [aa.ANH_FP32, aa.ANH_BF16])
def test_fused_head_kernel_for_every_class_count(classes, precision):
    """Full-width nets end in a 32-channel layer, which takes the fused head kernel (1x1 head + loss + head backward in one
    pass): one exact instantiation each for 2, 3 and 4 classes, the run-time-count body for 1 class, and the unfused
    kernels beyond 4 — all against the oracle (fp32 tight; bf16 against the bf16-restating oracle)."""
    o, t = trainer_pair(1, 3, classes, 1.0, 1, precision)
    rng = np.random.default_rng(40 + classes)
    d = o.recommended_input_dim(21)
    img, lab, w, wl = make_batch(rng, 3, d, 3, classes)
    if precision == aa.ANH_BF16:
        o.set_bf16_emulation(True)
    want_loss = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    got_loss = t.get_last_loss()
    head = o.layers[-1]
    hw = slice(head.w_off, head.w_off + head.cin * head.cout)
    hb = slice(head.b_off, head.b_off + head.cout)
    g, gw = t.get_grads(), o.grads
    if precision == aa.ANH_FP32:
        assert abs(got_loss - want_loss) <= 2e-5 * max(1.0, abs(want_loss))
        np.testing.assert_allclose(g, gw, rtol=2e-3, atol=2e-5 * np.abs(gw).max())
        p, _ = t.get_params()
        np.testing.assert_allclose(p, o.params, rtol=1e-4, atol=2e-6)
    else:
        assert abs(got_loss - want_loss) <= 2e-3 * max(1.0, abs(want_loss))
        for sl in (hw, hb):   # the head's own gradients come straight out of the fused kernel
            np.testing.assert_allclose(g[sl], gw[sl], rtol=3e-2, atol=3e-3 * max(np.abs(gw[sl]).max(), 1e-12))


def test_fp32_multi_step_training_tracks_oracle():
    o, t = trainer_pair(1, 3, 3, 0.25, 4, aa.ANH_FP32, lr=0.02)
    rng = np.random.default_rng(5)
    d = o.recommended_input_dim(21)
    for step in range(4):
        img, lab, w, wl = make_batch(rng, 2, d, 3, 3)
        want = o.train_step(img, lab, w)
        t.StartTraining(list(img), wl)
        assert abs(t.get_last_loss() - want) <= 1e-3 * max(1.0, abs(want))
    p, r = t.get_params()
    np.testing.assert_allclose(p, o.params, rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(r, o.running, rtol=2e-3, atol=2e-5)
    assert t.step_count() == 4
    # the snapshot (GetRuntimeNet) runs inference with the running statistics, like the oracle in inference mode
    rt = t.GetRuntimeNet(aa.ANH_FP32)
    o2 = OracleNet(1, 3, 3, 0.25, 4)
    o2.params[:], o2.running[:] = p, r
    img = rng.integers(0, 256, (1, d, d, 3), dtype=np.uint8)
    np.testing.assert_array_equal(rt.Forward(img), o2.forward(img))


def test_training_rejects_bad_labels_and_sizes():
    o, t = trainer_pair(1, 3, 3, 0.25, 4, aa.ANH_FP32)
    img = np.zeros((1, 15, 15, 3), np.uint8)
    wl = aa.set_weights(np.full((15, 15), 7, np.uint16), 0.5, 0.5)
    with pytest.raises(aa.AnnonetHipError) as e:
        t.StartTraining(list(img), [wl])
    assert e.value.code == 1 and "label" in str(e.value)
    with pytest.raises(aa.AnnonetHipError):
        t.StartTraining([np.zeros((16, 16, 3), np.uint8)], [aa.set_weights(np.zeros((16, 16), np.uint16), 0.5, 0.5)])
    with pytest.raises(aa.AnnonetHipError):
        t.StartTraining([], [])


def test_loss_scale_uses_global_batch_and_grad_bucket_layout():
    import ctypes as C
    import torch
    o, t = trainer_pair(1, 3, 3, 0.25, 4, aa.ANH_FP32)
    rng = np.random.default_rng(6)
    d = o.recommended_input_dim(17)
    img, lab, w, _ = make_batch(rng, 2, d, 3, 3)
    want = o.train_step(img, lab, w, loss_scale_n=8, apply_update=False)
    dev = torch.device("cuda:0")
    timg, tlab, tw = (torch.from_numpy(a).to(dev) for a in (img, lab.view(np.int16), w))
    t.forward_backward_device(timg.data_ptr(), tlab.data_ptr(), tw.data_ptr(), 2, d, d, 8)
    t.synchronize()
    np.testing.assert_allclose(t.get_grads(), o.grads, rtol=2e-3, atol=2e-5 * np.abs(o.grads).max())
    ptr, n = t.grad_buffer()
    assert n == o.n_params + 1


# ------------------------------------------------------------------------------------------------------------------
# bf16 throughput mode.  Two bars: (a) against the oracle restating the bf16 storage points (weights, conv inputs,
# stored conv outputs, stored gradients rounded to bf16; fp32 accumulation) — tight; (b) against the plain fp32
# oracle — the documented precision loss of the mode.
# ------------------------------------------------------------------------------------------------------------------
BF16_CASES = [(2, 1.0, 1), (2, 0.25, 4), (1, 1.0, 1), (3, 0.5, 1), (2, 0.1, 5)]


@pytest.mark.parametrize("levels,scaler,minf", BF16_CASES)
def test_bf16_forward(levels, scaler, minf):
    o, net = pair(levels, 3, 3, scaler, minf, aa.ANH_BF16)
    rng = np.random.default_rng(1)
    d = o.recommended_input_dim(45)
    img = rng.integers(0, 256, (2, d, d + (1 << levels), 3), dtype=np.uint8)
    got = net.Forward(img)
    # (a) bf16-restating oracle: only fp32 accumulation order and rare rounding-boundary flips differ.  Nets whose layers all run on
    # the persistent MFMA kernels store post-activation tensors in inference, the others raw conv outputs: the oracle restates either
    assert net.stores_activations() or scaler != 1.0     # the full-width nets take the activation-storing form
    o.set_bf16_emulation(1 if net.stores_activations() else 2)
    emu = o.forward(img)
    span = emu.max() - emu.min()
    assert np.abs(got - emu).max() <= 4e-3 * span, (np.abs(got - emu).max(), span)
    assert np.abs(got - emu).mean() <= 2e-4 * span
    mism = got.argmax(1) != emu.argmax(1)
    srt = np.sort(emu, axis=1)
    assert (srt[:, -1] - srt[:, -2])[mism].max(initial=0) <= 8e-3 * span
    assert mism.mean() <= 2e-3
    # (b) plain fp32 oracle
    o.set_bf16_emulation(False)
    want = o.forward(img)
    tol = 0.03 * span
    assert np.abs(got - want).max() <= tol
    mism = got.argmax(1) != want.argmax(1)
    srt = np.sort(want, axis=1)
    assert mism.mean() <= 0.03 and ((srt[:, -1] - srt[:, -2])[mism] <= 2 * tol).all()  # only near-ties may flip


def test_bf16_tiled_inference_full_width_net():
    """bf16 annonet_infer() on the full-width net (32-channel last hidden layer): the 1x1 head and the blend run as ONE kernel
    (head_blend); blended planes against the bf16-restating oracle, tiles small enough to exercise ramps and ragged edges."""
    o, net = pair(2, 3, 3, 1.0, 1, aa.ANH_BF16, seed=21)
    rng = np.random.default_rng(12)
    H, W = 210, 173
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ov = o.required_input_dim()
    tp = aa.tiling.parameters(96, 128, ov, ov)
    labels, blended = aa.annonet_infer(net, img, tiling_parameters=tp, want_blended=True)
    streamed = aa.annonet_infer(net, img, tiling_parameters=tp)           # the streamed host path (no planes requested)
    np.testing.assert_array_equal(streamed, labels)
    o.set_bf16_emulation(1 if net.stores_activations() else 2)
    want_labels, want = o.infer(img, max_tile=(96, 128), overlap=ov, want_blended=True)
    span = want.max() - want.min()
    # the worst pixel is one bf16 rounding flip in the last hidden layer times a large head weight (identical with the
    # unfused head, ANH_FUSE_HEAD_BLEND=0): 4.5e-3 of the span here; the mean bar is the tight one
    assert np.abs(blended - want).max() <= 6e-3 * span, (np.abs(blended - want).max(), span)
    assert np.abs(blended - want).mean() <= 2e-4 * span
    assert (labels != want_labels).mean() <= 2e-3


@pytest.mark.parametrize("levels,scaler,minf,in_ch", [(2, 1.0, 1, 3), (1, 0.25, 4, 3), (3, 0.5, 1, 3), (2, 0.1, 5, 3), (1, 1.0, 1, 1), (3, 1.0, 1, 3)])
def test_bf16_training_step(levels, scaler, minf, in_ch):
    o, t = trainer_pair(levels, in_ch, 3, scaler, minf, aa.ANH_BF16)   # in_ch = 1: the grayscale build variant
    rng = np.random.default_rng(2)
    d = o.recommended_input_dim(35)
    img, lab, w, wl = make_batch(rng, 4, d, in_ch, 3)
    p0, r0, m0 = o.params.copy(), o.running.copy(), o.momentum.copy()
    fp32_loss = o.train_step(img, lab, w, apply_update=False)
    o.set_bf16_emulation(True)
    want_loss = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    got_loss = t.get_last_loss()
    assert abs(got_loss - want_loss) <= 2e-3 * max(1.0, abs(want_loss))
    assert abs(got_loss - fp32_loss) <= 0.03 * max(1.0, abs(fp32_loss))
    # Whole-net gradients can only be held to a loose bar in bf16: two correct implementations decorrelate at the level
    # of one bf16 ulp (summation order moves dbeta by ~0.3%, which shifts every dy and re-rolls every rounding), and that
    # compounds through each bn backward.  Kernel-exact checks with identical inputs live in test_gpu_ops.py (convolutions) and
    # test_gpu_train_ops.py: dgamma / dbeta / coef of every bn layer (exact from the table totals), dy, the head's dW / db / loss.
    g, gw = t.get_grads(), o.grads
    for li, L in enumerate(o.layers):
        nw = L.k * L.k * L.cin * L.cout
        a, b = g[L.w_off:L.w_off + nw], gw[L.w_off:L.w_off + nw]
        rel = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-20)
        cos = float(a @ b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)
        # the two bars say the same thing for equal norms (rel^2 = 2 (1 - cos): cos 0.985 <-> rel 0.173); the deepest layer of
        # the three-level net sits at rel 0.13-0.15 depending on the reduction order of the head's partial sums
        assert rel < 0.175 and cos > 0.985, (li, L.cin, L.cout, L.k, rel, cos)
        if L.has_bn:
            want = o.layer_output(li, 0)
            got = t.layer_tensor(li, 0)
            assert np.abs(got - want).max() <= 1e-2 * np.abs(want).max(), li  # forward: at most one bf16 ulp
    p, r = t.get_params()
    assert np.isfinite(p).all() and np.isfinite(r).all()
    np.testing.assert_allclose(r, o.running, rtol=2e-2, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------------
# full-size cases (BASELINE.json configs) and the RCCL plumbing
# ------------------------------------------------------------------------------------------------------------------
def test_single_227_tile_through_annonet_infer_on_the_benchmark_net():
    """BASELINE config [0] on the HIP path: ONE 227 x 227 x 3 random tile of the benchmark net (levels 2, width 1.0, K = 3) through
    annonet_infer() — tiles.size() == 1, unique == full, no blend ramps (/root/reference/annonet_infer.cpp:42-66,147).
    fp32: planes and label map bit-exact against the oracle; bf16: the near-tie bar of test_bf16_forward."""
    img = np.random.default_rng(227).integers(0, 256, (227, 227, 3), dtype=np.uint8)
    o, net = pair(2, 3, 3, 1.0, 1, aa.ANH_FP32, seed=31)
    assert o.recommended_input_dim(227) == 227 and len(aa.tiling.get_tiles(227, 227, aa.tiling.parameters(1024, 1024, 35, 35))) == 1
    want_labels, want = o.infer(img, want_blended=True)
    labels, planes = aa.annonet_infer(net, img, want_blended=True)
    np.testing.assert_array_equal(planes, want)
    np.testing.assert_array_equal(labels, want_labels)
    np.testing.assert_array_equal(planes, net.Forward(img))          # one tile: the planes ARE the net's output
    _, net16 = pair(2, 3, 3, 1.0, 1, aa.ANH_BF16, seed=31)
    labels16, planes16 = aa.annonet_infer(net16, img, want_blended=True)
    span = want.max() - want.min()
    tol = 0.03 * span
    assert np.abs(planes16 - want).max() <= tol
    mism = labels16 != want_labels
    srt = np.sort(want, axis=0)
    assert mism.mean() <= 0.03 and ((srt[-1] - srt[-2])[mism] <= 2 * tol).all()      # only near-ties may flip
    o.set_bf16_emulation(1 if net16.stores_activations() else 2)
    emu_labels, emu = o.infer(img, want_blended=True)
    assert np.abs(planes16 - emu).max() <= 6e-3 * span and np.abs(planes16 - emu).mean() <= 2e-4 * span
    assert (labels16 != emu_labels).mean() <= 2e-3


# per-layer filter-gradient bar of the full-size bf16 step against the bf16-restating oracle (rel-L2; the cosine bar is the same statement)
FULL_SIZE_BF16_REL = 0.10     # measured 0.057 (worst layer) on the round-5 build: cos > 0.995


def test_full_size_training_step_batch32_227():
    """BASELINE config [1]: batch 32 x 3 x 227 x 227, levels 2, width 1.0.  fp32 parity mode against the oracle (which needs
    ~15 s of host time for this batch), and the bf16 mode's loss against both oracles."""
    rng = np.random.default_rng(0)
    n, d = 32, 227
    img = rng.integers(0, 256, (n, d, d, 3), dtype=np.uint8)
    lab = rng.integers(0, 3, (n, d, d)).astype(np.uint16)
    lab[rng.random((n, d, d)) < 0.05] = IGNORE
    wl = [aa.set_weights(lab[i], 0.5, 0.5) for i in range(n)]
    w = np.stack([x["weight"] for x in wl])
    o, t = trainer_pair(2, 3, 3, 1.0, 1, aa.ANH_FP32, lr=0.1)
    want = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    assert abs(t.get_last_loss() - want) <= 2e-5 * max(1.0, abs(want))
    g, gw = t.get_grads(), o.grads
    np.testing.assert_allclose(g, gw, rtol=5e-3, atol=5e-5 * np.abs(gw).max())
    p, r = t.get_params()
    np.testing.assert_allclose(p, o.params, rtol=1e-4, atol=5e-6)
    np.testing.assert_allclose(r, o.running, rtol=1e-4, atol=1e-5)
    o2, t2 = trainer_pair(2, 3, 3, 1.0, 1, aa.ANH_BF16, lr=0.1)
    t2.StartTraining(list(img), wl)
    assert abs(t2.get_last_loss() - want) <= 0.02 * max(1.0, abs(want))
    g2 = t2.get_grads()
    for L in o.layers:  # at this batch size the bf16 gradients line up with fp32 far better than on toy batches
        nw = L.k * L.k * L.cin * L.cout
        a, b = g2[L.w_off:L.w_off + nw], gw[L.w_off:L.w_off + nw]
        cos = float(a @ b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)
        assert cos > 0.97, (L.cin, L.cout, cos)
    # ... and against the oracle RESTATING the bf16 storage points, at the bars of test_bf16_training_step: this is the regime bench.py
    # runs (256 persistent workgroups walking 3.5-29 items each), where a wrong halo row on every n-th tile would still pass a cosine
    # against fp32.  Loss 2e-3, every layer's filter gradient rel-L2 / cosine, every bn layer's stored forward output within one bf16 ulp.
    o2.set_bf16_emulation(True)
    want16 = o2.train_step(img, lab, w)
    assert abs(t2.get_last_loss() - want16) <= 2e-3 * max(1.0, abs(want16))
    gw16 = o2.grads
    worst = []
    for li, L in enumerate(o2.layers):
        nw = L.k * L.k * L.cin * L.cout
        a, b = g2[L.w_off:L.w_off + nw], gw16[L.w_off:L.w_off + nw]
        rel = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-20)
        cos = float(a @ b) / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30)
        worst.append((round(float(rel), 4), li))
        assert rel < FULL_SIZE_BF16_REL and cos > 1.0 - FULL_SIZE_BF16_REL ** 2 / 2, (li, L.cin, L.cout, L.k, rel, cos)
        if L.has_bn:
            want_y = o2.layer_output(li, 0)
            got_y = t2.layer_tensor(li, 0)
            assert np.abs(got_y - want_y).max() <= 1e-2 * np.abs(want_y).max(), li
    print("full-size bf16 step vs the bf16-restating oracle, per-layer filter-gradient rel-L2:", sorted(worst, reverse=True)[:4])


@pytest.mark.parametrize("H,W,scaler,min_filters", [(1500, 2100, 0.25, 4), (4096, 4096, 1.0, 1)])
def test_large_image_tiled_inference_properties(H, W, scaler, min_filters):
    """BASELINE config [2]: tiled sliding-window inference with 1024^2 tiles — a ragged multi-tile image on a narrow net, and THE
    config itself (4096 x 4096, the benchmark net: levels 2, width 1.0, K = 3) — through size-independent properties: fp32 labels
    and planes bit-exact against the oracle on windows deep inside several tiles, determinism, the device-resident entry point
    equal to the host one, a two-replica run equal except at near-ties, and label agreement bf16 vs fp32."""
    o, net = pair(2, 3, 3, scaler, min_filters, aa.ANH_FP32, seed=13)
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ov = o.required_input_dim()
    tp = aa.tiling.parameters(1024, 1024, ov, ov)
    labels, blended = aa.annonet_infer(net, img, tiling_parameters=tp, want_blended=True)
    labels2 = aa.annonet_infer(net, img, tiling_parameters=tp)            # the streamed host path (strips up, label rows down)
    np.testing.assert_array_equal(labels, labels2)                       # deterministic, and both host paths agree
    assert labels.max() < 3 and blended.shape == (3, H, W)
    tiles = aa.tiling.get_tiles(W, H, tp)
    assert len(tiles) == (6 if H == 1500 else 25)
    # a pixel deep inside a tile's unique rect sees only real image data: its logits equal a plain forward of a crop around it
    picks = [0] if H == 1500 else [0, 12, 24, 9]      # corner, centre, opposite corner and an edge tile of the 5 x 5 grid
    for ti in picks:
        (fl, ft, fr, fb), (ul, ut, ur, ub) = tiles[ti]
        # the net input window of that tile (annonet_infer.cpp:46-66); the net is translation-equivariant only for shifts that
        # are multiples of 2^levels (stride-2 grid phase), so the comparison crop is aligned to the window modulo 4
        fw, fh = fr - fl + 1, fb - ft + 1
        win_left = fl + fw // 2 - o.recommended_input_dim(fw) // 2
        win_top = ft + fh // 2 - o.recommended_input_dim(fh) // 2
        d = o.recommended_input_dim(2 * ov + 41)
        cy, cx = (ut + ub) // 2, (ul + ur) // 2
        top = win_top + ((cy - d // 2 - win_top) // 4) * 4
        left = win_left + ((cx - d // 2 - win_left) // 4) * 4
        crop = img[top:top + d, left:left + d]
        want = o.forward(crop[None])[0]
        m = ov  # margin: receptive field
        np.testing.assert_array_equal(blended[:, top + m:top + d - m, left + m:left + d - m], want[:, m:d - m, m:d - m])
        np.testing.assert_array_equal(labels[top + m:top + d - m, left + m:left + d - m], want[:, m:d - m, m:d - m].argmax(0))
    assert np.isfinite(blended).all()
    # the device-resident entry point (image, planes and label map in HBM) equals the host one
    import torch
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(img).to(dev)
    d_lab = torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_pl = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    aa.annonet_infer_device(net, d_img.data_ptr(), H, W, d_lab.data_ptr(), d_pl.data_ptr(), tiling_parameters=tp)
    net.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy().view(np.uint16), labels)
    np.testing.assert_array_equal(d_pl.cpu().numpy(), blended)
    del d_img, d_lab, d_pl
    # two replicas (device 0 twice on this box): one host label map, equal except where four tiles meet and the sum order differs
    p, r = net.get_params()
    aa.set_devices([0, 0])
    try:
        net2 = aa.RuntimeNet(aa.net_config(2, 3, 3, scaler, min_filters, aa.ANH_FP32))
        net2.set_params(p, r)
        sharded = aa.annonet_infer(net2, img, tiling_parameters=tp)
    finally:
        aa.set_devices([])
    assert (sharded != labels).mean() < 1e-4
    # bf16 mode: label agreement
    _, net16 = pair(2, 3, 3, scaler, min_filters, aa.ANH_BF16, seed=13)
    l16 = aa.annonet_infer(net16, img, tiling_parameters=tp)
    assert (l16 == labels).mean() > 0.97


def test_16384_square_image_tiled_inference_properties():
    """BASELINE config [4]'s workload on ONE GPU: a 16384 x 16384 synthetic image, the benchmark net, 1024^2 tiles with the receptive
    field as overlap (289 tiles; /root/reference/annonet_infer_main.cpp:300-303,423-427), image, class planes (3 GiB) and label map resident
    in HBM.  Size-independent properties, as the 4096^2 case: fp32 planes and labels bit-exact against the oracle's forward on windows
    deep inside five tiles (corners, centre, an edge), labels = argmax of the planes on those windows, every label a class, and the
    bf16 mode's label map >= 97 % equal to the fp32 one on the same windows."""
    import torch
    H = W = 16384
    o, net = pair(2, 3, 3, 1.0, 1, aa.ANH_FP32, seed=13)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    d_img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    ov = o.required_input_dim()
    tp = aa.tiling.parameters(1024, 1024, ov, ov)
    tiles = aa.tiling.get_tiles(W, H, tp)
    assert len(tiles) == 289
    d_lab = torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_pl = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    aa.annonet_infer_device(net, d_img.data_ptr(), H, W, d_lab.data_ptr(), d_pl.data_ptr(), tiling_parameters=tp)
    net.synchronize()
    assert int(d_lab.view(torch.int16).max()) < 3 and int(d_lab.min()) >= 0
    assert bool(torch.isfinite(d_pl[:, ::97, ::89]).all())
    windows = []
    for ti in (0, 16, 144, 272, 288, 8 * 17):      # four corners' tiles, the centre tile and a left-edge tile of the 17 x 17 grid
        (fl, ft, fr, fb), (ul, ut, ur, ub) = tiles[ti]
        fw, fh = fr - fl + 1, fb - ft + 1
        win_left = fl + fw // 2 - o.recommended_input_dim(fw) // 2
        win_top = ft + fh // 2 - o.recommended_input_dim(fh) // 2
        d = o.recommended_input_dim(2 * ov + 41)
        cy, cx = (ut + ub) // 2, (ul + ur) // 2
        top = win_top + ((cy - d // 2 - win_top) // 4) * 4      # (the net is translation-equivariant for shifts that are multiples of 2^levels)
        left = win_left + ((cx - d // 2 - win_left) // 4) * 4
        crop = d_img[top:top + d, left:left + d].cpu().numpy()
        want = o.forward(crop[None])[0]
        m = ov
        got_pl = d_pl[:, top + m:top + d - m, left + m:left + d - m].cpu().numpy()
        got_lab = d_lab[top + m:top + d - m, left + m:left + d - m].cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(got_pl, want[:, m:d - m, m:d - m])
        np.testing.assert_array_equal(got_lab, want[:, m:d - m, m:d - m].argmax(0))
        windows.append((top + m, top + d - m, left + m, left + d - m, got_lab))
    # bf16 mode on the same image: label agreement on the windows
    p, r = net.get_params()
    del d_pl
    net16 = aa.RuntimeNet(aa.net_config(2, 3, 3, 1.0, 1, aa.ANH_BF16))
    net16.set_params(p, r)
    d_pl16 = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    d_lab16 = torch.zeros((H, W), dtype=torch.int16, device=dev)
    aa.annonet_infer_device(net16, d_img.data_ptr(), H, W, d_lab16.data_ptr(), d_pl16.data_ptr(), tiling_parameters=tp)
    net16.synchronize()
    same = total = 0
    for (t0, t1, l0, l1, lab32) in windows:
        lab16 = d_lab16[t0:t1, l0:l1].cpu().numpy().view(np.uint16)
        same += int((lab16 == lab32).sum()); total += lab32.size
    assert same / total > 0.97, same / total
    # ... and on a strided sample of the whole map (every tile contributes)
    agree = float((d_lab16[::61, ::67] == d_lab[::61, ::67]).float().mean())
    assert agree > 0.97, agree
    del d_img, d_lab, d_lab16, d_pl16
    torch.cuda.empty_cache()


def test_grad_bucket_is_a_live_view_and_all_reduce_runs_on_it():
    """The gradient bucket handed to torch.distributed is the library's own HBM (zero copy), and an RCCL all-reduce on it
    (world size 1 on this box) leaves the step's result unchanged."""
    import os
    import torch
    import torch.distributed as dist
    from annonet_amd import dist as aad
    o, t = trainer_pair(1, 3, 3, 0.25, 4, aa.ANH_FP32)
    rng = np.random.default_rng(6)
    d = o.recommended_input_dim(17)
    img, lab, w, _ = make_batch(rng, 2, d, 3, 3)
    dev = torch.device("cuda:0")
    timg, tlab, tw = (torch.from_numpy(a).to(dev) for a in (img, lab.view(np.int16), w))
    bucket = aad.grad_bucket_tensor(t)
    assert bucket.numel() == o.n_params + 1 and bucket.is_cuda
    t.forward_backward_device(timg.data_ptr(), tlab.data_ptr(), tw.data_ptr(), 2, d, d, 2)
    t.synchronize()
    want = o.train_step(img, lab, w, apply_update=False)
    assert abs(float(bucket[-1].item()) - want) <= 2e-5 * max(1.0, abs(want))      # trailing slot = loss
    head = o.layers[-1]
    got_bias_grad = bucket[head.b_off:head.b_off + 3].cpu().numpy()               # bias segment is layout-independent
    np.testing.assert_allclose(got_bias_grad, o.grads[head.b_off:head.b_off + 3], rtol=2e-3, atol=1e-7)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        before = bucket.clone()
        with torch.cuda.stream(aad.handle_stream(t)):    # the collective is ordered on the trainer's own stream
            dist.all_reduce(bucket, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        assert torch.equal(before, bucket)
        t.apply_update(1.0)
        t.synchronize()
    finally:
        dist.destroy_process_group()
    o.train_step(img, lab, w)  # same step with the update applied
    p, _ = t.get_params()
    np.testing.assert_allclose(p, o.params, rtol=1e-4, atol=2e-6)


def test_early_reduce_overlaps_the_all_reduce_and_changes_nothing():
    """dist.EarlyReduce: the bucket's tail (layers >= 2, head, loss slot) is all-reduced on a side stream gated by the library's
    event while backward still runs, the first two layers' part afterwards on the trainer's stream.  Three bf16 steps at world size 1
    (RCCL) end with parameters BIT-identical to the plain schedule."""
    import os
    import torch
    import torch.distributed as dist
    from annonet_amd import dist as aad
    rng = np.random.default_rng(12)
    n, d = 4, 99
    img = rng.integers(0, 256, (n, d, d, 3), dtype=np.uint8)
    lab = rng.integers(0, 3, (n, d, d)).astype(np.uint16)
    w = np.ones((n, d, d), np.float32)
    dev = torch.device("cuda:0")
    timg, tlab, tw = (torch.from_numpy(a).to(dev) for a in (img, lab.view(np.int16), w))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        params = []
        for use_early in (True, False):
            t = aa.TrainingNet(2, 3, aa.ANH_BF16, seed=3)
            t.SetNetWidth(1.0, 1); t.SetClassCount(3); t.Initialize(); t.SetLearningRate(0.05)
            bucket = aad.grad_bucket_tensor(t)
            stream = aad.handle_stream(t)
            early = aad.EarlyReduce(t, bucket) if use_early else None
            if use_early:
                assert early.split and early.first == t.early_grads() and 0 < early.first < bucket.numel() // 4   # the early part is most of the bucket
            for _ in range(3):
                aad.data_parallel_step(t, bucket, timg.data_ptr(), tlab.data_ptr(), tw.data_ptr(), n, d, d, 1, force_collective=True, stream=stream, early=early)
            t.synchronize()
            params.append(t.get_params())
            del bucket, stream, early, t
    finally:
        dist.destroy_process_group()
    np.testing.assert_array_equal(params[0][0], params[1][0])
    np.testing.assert_array_equal(params[0][1], params[1][1])


def test_single_tile_whose_layer_planes_exceed_2_31_elements():
    """One 8195 x 8195 tile through the benchmark net: the 32-channel tensors at full resolution hold 8195^2 x 32 = 2.15e9 elements,
    past the 32-bit element offsets of the persistent conv kernels, so those layers take the one-tile-per-workgroup kernels with
    64-bit indexing (and the net the raw-output storage form).  Checked where it can be: against the bf16-restating oracle on crops
    deep inside the image — at the far corner too, where the element offsets are largest — and through finiteness / label range."""
    o, net = pair(2, 3, 3, 1.0, 1, aa.ANH_BF16, seed=17)
    side = 8195
    assert o.recommended_input_dim(side) == side and side * side * 32 >= 2 ** 31
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    labels, blended = aa.annonet_infer(net, img, want_blended=True)        # no tiling parameters: ONE tile
    assert not net.stores_activations()                                    # the persistent kernels do not cover every layer here
    assert labels.max() < 3 and np.isfinite(blended[:, ::97, ::89]).all()
    o.set_bf16_emulation(2)
    ov = o.required_input_dim()
    d = o.recommended_input_dim(2 * ov + 41)
    worst_mismatch = 0.0
    for top, left in ((4096, 4000), (side - d - 4 - (side - d - 4) % 4, side - d - 8 - (side - d - 8) % 4), (8, 7000)):
        top -= top % 4; left -= left % 4                                  # the stride-2 grid phase of the whole-image window (origin 0)
        want = o.forward(img[top:top + d, left:left + d][None])[0]
        m = ov
        got = blended[:, top + m:top + d - m, left + m:left + d - m]
        ref = want[:, m:d - m, m:d - m]
        span = want.max() - want.min()
        assert np.abs(got - ref).max() <= 6e-3 * span, (top, left, float(np.abs(got - ref).max()), float(span))
        assert np.abs(got - ref).mean() <= 3e-4 * span
        worst_mismatch = max(worst_mismatch, float((labels[top + m:top + d - m, left + m:left + d - m] != ref.argmax(0)).mean()))
    assert worst_mismatch <= 0.01


def test_non_finite_bn_sums_poison_the_table_instead_of_passing_as_numbers():
    """The bn accumulator tables hold integers (bnacc.h): a workgroup partial that is not finite, or too large for the fixed-point
    range, cannot be added — it raises the table's poison word and every fold of that table yields NaN: a diverged net shows as NaN
    parameters after the step (the loss itself clamps its probabilities and stays finite), never as finite numbers formed from a
    wrapped or truncated sum.  A stem filter blown up to 1e30 overflows the stem's sum of squares."""
    o, t = trainer_pair(2, 3, 3, 1.0, 1, aa.ANH_BF16, lr=0.05)
    p, r = t.get_params()
    L0 = o.layers[0]
    p = p.copy()
    p[L0.w_off:L0.w_off + 16] = 1e30
    t.set_params(p, r)
    rng = np.random.default_rng(3)
    d = 43
    img = rng.integers(1, 256, (2, d, d, 3), dtype=np.uint8)
    lab = rng.integers(0, 3, (2, d, d)).astype(np.uint16)
    t.StartTraining(list(img), [aa.set_weights(l, 0.5, 0.5) for l in lab])
    t.synchronize()
    after, _ = t.get_params()
    L1 = o.layers[1]
    assert np.isnan(after[L1.w_off:L1.w_off + 64]).all()      # the next layer's filters saw a NaN input through the poisoned fold
