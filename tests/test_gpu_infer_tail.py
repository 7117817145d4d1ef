"""The tail of tiled inference where the planes are NOT fresh zeros, and class counts beyond the specialised kernels.

A. annonet_infer() on DIRTY class planes.  When the tile list is the image's complete tiling, Engine::infer_device clears only the frames
   between each tile's full and unique rectangle (zero_rects, the list cached under a hash of the geometry); everything else is assigned.
   In production the planes are dirty on every image after the first (anh_infer reuses stage_blended).  Every case here starts from planes
   filled with NaN (propagates through any accumulation into an uncleared pixel) and again from planes filled with 7.0 (a finite value
   turns into a plausible wrong number), and a label map filled with 0xABAB.  fp32: planes and label maps BIT-EXACT against the oracle.
   Also: the rectangle cache across geometries on one handle and one buffer, the host form over a shrinking stage_blended, caller tile
   lists in another order than the tiler's (blend_batch gathers "in list order"), anh_argmax_device on row ranges.
B. Class counts 6 ... 64 (spec.cpp accepts 1..64): blend_batch, head_blend, the head-in-epilogue form and head_train stop at 4 classes, so
   the head runs as a plain conv with cout = K (fp32: conv_f32_mfma*, output channels padded to 32), the loss as loss_kernel<8> (K <= 8) or
   loss_kernel<64>, argmax on its scalar path above 8.  Bars: those of test_gpu_parity.py for the same comparison at 3 classes, unchanged.
"""
import functools

import numpy as np
import pytest

import annonet_amd as aa
from conftest import random_params
from oracle.oracle import OracleNet, IGNORE

pytestmark = pytest.mark.gpu

NARROW = (1, 3, 0.25, 4)     # levels, input channels, width scaler, min filters: the 8-channel net of part A
FULL = (1, 3, 1.0, 1)        # full width: 32-channel last hidden layer
LABEL_FILL = 0xABAB
FILLS = [float("nan"), 7.0]
FILL_IDS = ["nan", "seven"]


def pair(levels, in_ch, classes, scaler, minf, precision, seed=7):
    o = OracleNet(levels, in_ch, classes, scaler, minf)
    p, r = random_params(o, seed)
    o.params[:] = p
    o.running[:] = r
    net = aa.RuntimeNet(aa.net_config(levels, in_ch, classes, scaler, minf, precision))
    net.set_params(p, r)
    return o, net


@functools.lru_cache(maxsize=None)
def oracle_net(classes, shape=NARROW, seed=9):
    levels, in_ch, scaler, minf = shape
    o = OracleNet(levels, in_ch, classes, scaler, minf)
    o.params[:], o.running[:] = random_params(o, seed)
    return o


def runtime_net(classes, shape=NARROW, seed=9, precision=aa.ANH_FP32):
    levels, in_ch, scaler, minf = shape
    o = oracle_net(classes, shape, seed)
    net = aa.RuntimeNet(aa.net_config(levels, in_ch, classes, scaler, minf, precision))
    net.set_params(o.params.copy(), o.running.copy())
    return net


@functools.lru_cache(maxsize=None)
def image(H, W):
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def class_gains(K):
    return np.linspace(-0.2, 0.2, K)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def expected(classes, H, W, max_tile, overlap=None, with_gains=False, order=None, shape=NARROW):
    """(labels, planes) of the oracle, computed once per case and shared read-only.  order = None: the oracle's own tiler;
    otherwise a tuple of tile indices into the tiler's list (a caller's list)."""
    o = oracle_net(classes, shape)
    ov = o.required_input_dim() if overlap is None else overlap
    gains = class_gains(classes) if with_gains else None
    if order is None:
        return frozen(*o.infer(image(H, W), gains=gains, max_tile=(max_tile, max_tile), overlap=ov, want_blended=True))
    tiles = tiler_list(H, W, max_tile, ov)
    return frozen(*o.infer(image(H, W), gains=gains, tiles=[tiles[i] for i in order], want_blended=True))


def tiler_list(H, W, max_tile, ov):
    return aa.tiling.get_tiles(W, H, aa.tiling.parameters(max_tile, max_tile, ov, ov))


class DevicePlanes:
    """One flat fp32 buffer in HBM for the class planes, filled ONCE; every call lays its [K, H, W] planes over its start, so a second
    call finds the previous image's planes (of another geometry) where it writes.  The label map is filled with 0xABAB per call."""

    def __init__(self, floats, fill):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.buf = torch.full((floats,), fill, dtype=torch.float32, device=self.dev)

    def infer(self, net, img, gains=None, tiling_parameters=None, tiles=None):
        torch = self.torch
        H, W = img.shape[:2]
        K = net.cfg.classes
        assert K * H * W <= self.buf.numel()
        d_img = torch.from_numpy(np.ascontiguousarray(img)).to(self.dev)
        d_lab = torch.full((H, W), LABEL_FILL - 65536, dtype=torch.int16, device=self.dev)
        torch.cuda.synchronize()
        aa.annonet_infer_device(net, d_img.data_ptr(), H, W, d_lab.data_ptr(), self.buf.data_ptr(), gains=gains, tiling_parameters=tiling_parameters, tiles=tiles)
        net.synchronize()
        return d_lab.cpu().numpy().view(np.uint16), self.buf[:K * H * W].cpu().numpy().reshape(K, H, W)


def check(got, want):
    np.testing.assert_array_equal(got[1], want[1])      # planes (NaN == NaN here, but the oracle's planes are finite)
    np.testing.assert_array_equal(got[0], want[0])      # label map
    assert np.isfinite(want[1]).all()


# ------------------------------------------------------------------------------------------------------------------
# A. dirty planes
# ------------------------------------------------------------------------------------------------------------------
#   H    W  max tile  tiles  classes
TILINGS = [(40, 150, 64, 3, 3),        # 1 x 3: one axis fits a tile — no frames above or below
           (150, 40, 64, 3, 3),        # 3 x 1: the other axis
           (130, 75, 57, 6, 3)]        # 3 x 2, ragged sides
for _K in (1, 2, 4, 5, 9):             # <= 4 classes: the batched blend; >= 5: one blend launch per tile
    TILINGS.append((90, 140, 64, 6, _K))      # 2 x 3: corners where four tiles meet
    TILINGS.append((170, 190, 48, 30, _K))    # 5 x 6: more equal windows than one batch holds (16) — two batches of 15, frames across their boundary


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("H,W,max_tile,n_tiles,classes", TILINGS)
def test_frame_clear_on_dirty_planes(H, W, max_tile, n_tiles, classes, fill):
    o = oracle_net(classes)
    ov = o.required_input_dim()
    assert ov == 15 and len(tiler_list(H, W, max_tile, ov)) == n_tiles
    net = runtime_net(classes)
    tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
    for with_gains in (False, True):
        planes = DevicePlanes(classes * H * W, fill)
        got = planes.infer(net, image(H, W), gains=class_gains(classes) if with_gains else None, tiling_parameters=tp)
        check(got, expected(classes, H, W, max_tile, with_gains=with_gains))


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
def test_frame_rectangle_cache_across_geometries_on_one_handle_and_one_buffer(fill):
    """The frame list is cached under a hash of (H, W, count, rectangles).  One handle, one plane buffer that is never refilled: each
    call finds the previous image's planes.  Step 3 returns to a geometry seen before, step 4 keeps H, W and the tile count and moves
    the rectangles (a key without them would reuse step 3's frames)."""
    o = oracle_net(3)
    ov = o.required_input_dim()
    wide = 22      # a larger overlap: 90 x 140 / 64 is still 2 x 3 tiles, every rectangle elsewhere
    std, other = tiler_list(90, 140, 64, ov), tiler_list(90, 140, 64, wide)
    assert len(std) == 6 and len(other) == 6 and other != std
    assert tiler_list(90, 140, 60, ov) == std          # (max_tile = 60 is NOT another tiling)
    assert [u for _, u in other] != [u for _, u in std] and [f for f, _ in other] != [f for f, _ in std]
    net = runtime_net(3)
    planes = DevicePlanes(3 * 90 * 140, fill)
    for with_gains in (False, True):       # the sequence twice on the same handle and buffer
        for H, W, max_tile, overlap in [(90, 140, 64, ov), (130, 75, 57, ov), (90, 140, 64, ov), (90, 140, 64, wide), (40, 150, 64, ov)]:
            got = planes.infer(net, image(H, W), gains=class_gains(3) if with_gains else None, tiling_parameters=aa.tiling.parameters(max_tile, max_tile, overlap, overlap))
            check(got, expected(3, H, W, max_tile, overlap=overlap, with_gains=with_gains))


def test_host_form_blends_each_image_over_the_previous_images_planes():
    """anh_infer keeps stage_blended between calls (reserve only grows it): from large to small it is never reallocated, so every
    image after the first is blended over the planes of the one before."""
    o = oracle_net(3)
    ov = o.required_input_dim()
    net = runtime_net(3)
    for H, W, max_tile, det in [(170, 190, 48, None), (90, 140, 64, None), (40, 150, 64, None), (90, 140, 64, [0.0, 0.5, 0.25])]:
        tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
        got = aa.annonet_infer(net, image(H, W), detection_levels=det, tiling_parameters=tp, want_blended=True)
        want = expected(3, H, W, max_tile) if det is None else o.infer(image(H, W), detection_levels=det, max_tile=(max_tile, max_tile), overlap=ov, want_blended=True)
        check(got, want)
        if det is not None:
            assert (want[0] != expected(3, H, W, max_tile)[0]).any()      # the filter relabels something: the case is not vacuous


def caller_order(kind, n):
    if kind == "tiler":
        return tuple(range(n))
    if kind == "reversed":
        return tuple(range(n))[::-1]
    if kind == "shuffled":
        return tuple(int(i) for i in np.random.default_rng(3).permutation(n))
    return tuple(i for i in range(n) if i != 2)       # "without_2"


@pytest.mark.parametrize("fill", FILLS, ids=FILL_IDS)
@pytest.mark.parametrize("kind", ["tiler", "reversed", "shuffled", "without_2"])
@pytest.mark.parametrize("H,W,max_tile", [(90, 140, 64), (170, 190, 48)])
def test_caller_tile_lists_with_tiling_parameters_on_dirty_planes(H, W, max_tile, kind, fill):
    """tiles= AND tiling_parameters=: the tiler's own list is recognised as the complete tiling (frame clear), every other list takes
    the full clear and is blended in ITS order — the float sums where tiles overlap depend on that order."""
    o = oracle_net(3)
    ov = o.required_input_dim()
    tiles = tiler_list(H, W, max_tile, ov)
    order = caller_order(kind, len(tiles))
    std = expected(3, H, W, max_tile)
    want = expected(3, H, W, max_tile, order=order)
    # non-vacuity, on the oracle's output alone
    if kind == "tiler":
        np.testing.assert_array_equal(want[1], std[1])
    elif kind in ("reversed", "shuffled"):
        assert sorted(order) == list(range(len(tiles))) and order != tuple(range(len(tiles)))
        assert (want[1] != std[1]).sum() > 1000 and np.abs(want[1] - std[1]).max() < 1e-5      # another order of the same sums
    else:
        ul, ut, ur, ub = tiles[2][1]
        assert (want[1][:, ut:ub + 1, ul:ur + 1] == 0).all() and (want[0][ut:ub + 1, ul:ur + 1] == 0).all()
        assert (std[1][:, ut:ub + 1, ul:ur + 1] != 0).all()
    net = runtime_net(3)
    tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
    for with_gains in (False, True):
        planes = DevicePlanes(3 * H * W, fill)
        got = planes.infer(net, image(H, W), gains=class_gains(3) if with_gains else None, tiling_parameters=tp, tiles=[tiles[i] for i in order])
        check(got, expected(3, H, W, max_tile, with_gains=with_gains, order=order))


def test_bf16_frame_clear_equals_full_clear_on_dirty_planes():
    """The full-width bf16 net (head-in-epilogue conv + blend_batch): the complete tiling through tiling_parameters= (frame clear) and
    the same list through tiles= alone (full clear) run the same blends and differ only in the clear."""
    H, W, max_tile = 90, 140, 64
    o = oracle_net(3, FULL, seed=21)
    net = runtime_net(3, FULL, seed=21, precision=aa.ANH_BF16)
    ov = o.required_input_dim()
    tiles = tiler_list(H, W, max_tile, ov)
    assert len(tiles) == 6
    tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
    framed = DevicePlanes(3 * H * W, float("nan")).infer(net, image(H, W), tiling_parameters=tp)
    full = DevicePlanes(3 * H * W, float("nan")).infer(net, image(H, W), tiles=tiles)
    assert np.isfinite(framed[1]).all() and np.isfinite(full[1]).all()
    np.testing.assert_array_equal(framed[1], full[1])
    np.testing.assert_array_equal(framed[0], full[0])
    o.set_bf16_emulation(1 if net.stores_activations() else 2)
    try:
        want_labels, want = o.infer(image(H, W), max_tile=(max_tile, max_tile), overlap=ov, want_blended=True)
    finally:
        o.set_bf16_emulation(False)
    span = want.max() - want.min()
    worst = (float(np.abs(framed[1] - want).max() / span), float(np.abs(framed[1] - want).mean() / span), float((framed[0] != want_labels).mean()))
    print("bf16 tiled planes vs the bf16-restating oracle (max / span, mean / span, label mismatches):", worst)
    assert worst[0] <= 6e-3
    assert worst[1] <= 2e-4
    assert worst[2] <= 2e-3


def find_label_reference(planes, gains):
    """find_label (annonet_infer.cpp:170-185) in numpy: start label 65535, start best -inf, value = float32(float64(v) + gain),
    strict '>' (a NaN never wins), lowest index wins a tie."""
    label = np.full(planes.shape[1:], 65535, np.uint16)
    best = np.full(planes.shape[1:], -np.inf, np.float32)
    for c in range(planes.shape[0]):
        value = (planes[c].astype(np.float64) + (0.0 if gains is None else float(gains[c]))).astype(np.float32)
        wins = value > best
        label[wins] = c
        best[wins] = value[wins]
    return label


@pytest.mark.parametrize("K", [1, 3, 8, 9, 33])
def test_argmax_device_row_ranges(K):
    """anh_argmax_device on rows [row0, row1) of [K, 37, 53] planes: the width is odd, so row0 * W is no multiple of 4 and the
    four-pixel path (K <= 8) starts unaligned and ends in its scalar remainder; K > 8 takes the scalar path.  Rows outside the range
    keep the fill."""
    import torch
    H, W = 37, 53
    rng = np.random.default_rng(100 + K)
    planes = rng.normal(0, 1, (K, H, W)).astype(np.float32)
    flat = planes.reshape(K, -1)
    px = rng.permutation(H * W)
    ties = []
    if K > 1:
        for p in px[:120]:                                  # exact ties at the top: the lowest index must win
            a, b = (int(c) for c in rng.choice(K, 2, replace=False))
            flat[a, p] = flat[b, p] = 6.0 + (p % 3)
            ties.append((p, min(a, b)))
    flat[:, px[120:150]] = np.nan                           # every class NaN: no class wins, the label stays 65535
    for p in px[150:220]:
        flat[rng.integers(0, K), p] = np.nan                # one class NaN
    lowest = K - 1
    flat[lowest, px[220:300]] = -np.inf                     # one class at -inf (K = 1: -inf > -inf is false, 65535 again)
    gains = class_gains(K)
    want = {False: find_label_reference(planes, None), True: find_label_reference(planes, gains)}
    # non-vacuity, on the reference alone
    assert (want[False] == 65535).sum() >= 30
    if K <= 9:
        assert set(range(K)) <= set(np.unique(want[False]).tolist())
    else:
        assert (want[False] == 32).any() and (want[True] == 32).any()
    assert all(want[False].reshape(-1)[p] == c for p, c in ties)      # the winner of those pixels is the lower of two equal values
    assert (want[True] != want[False]).any() or K == 1
    net = aa.RuntimeNet(aa.net_config(1, 3, K, 0.25, 4, aa.ANH_FP32))
    dev = torch.device("cuda", 0)
    d_planes = torch.from_numpy(planes).to(dev)
    assert (5 * W) % 4 == 1 and (3 * W) % 4 == 3
    for row0, row1 in [(0, 37), (5, 6), (3, 30), (36, 37)]:
        for with_gains in (False, True):
            d_lab = torch.full((H, W), LABEL_FILL - 65536, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            aa.argmax_device(net, d_planes.data_ptr(), H, W, row0, row1, d_lab.data_ptr(), gains=gains if with_gains else None)
            net.synchronize()
            got = d_lab.cpu().numpy().view(np.uint16)
            exp = np.full((H, W), LABEL_FILL, np.uint16)
            exp[row0:row1] = want[with_gains][row0:row1]
            np.testing.assert_array_equal(got, exp, err_msg=str((K, row0, row1, with_gains)))


# ------------------------------------------------------------------------------------------------------------------
# B. class counts 6 ... 64
# ------------------------------------------------------------------------------------------------------------------
MANY = [6, 8, 9, 33, 64]
SHAPE_IDS = ["narrow", "full"]


@pytest.mark.parametrize("shape", [NARROW, FULL], ids=SHAPE_IDS)
@pytest.mark.parametrize("K", MANY)
def test_fp32_forward_is_bit_exact_for_many_classes(K, shape):
    levels, in_ch, scaler, minf = shape
    o, net = pair(levels, in_ch, K, scaler, minf, aa.ANH_FP32)
    rng = np.random.default_rng(1)
    d = o.recommended_input_dim(37 if scaler < 1 else 23)
    img = rng.integers(0, 256, (2, d, d + (1 << levels), in_ch), dtype=np.uint8)
    want = o.forward(img)
    got = net.Forward(img)
    assert got.shape == want.shape == (2, K, d, d + (1 << levels))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape", [NARROW, FULL], ids=SHAPE_IDS)
@pytest.mark.parametrize("K", MANY)
def test_fp32_tiled_infer_is_bit_exact_for_many_classes(K, shape):
    H, W, max_tile = 90, 140, 64
    o = oracle_net(K, shape)
    net = runtime_net(K, shape)
    ov = o.required_input_dim()
    assert len(tiler_list(H, W, max_tile, ov)) == 6
    tp = aa.tiling.parameters(max_tile, max_tile, ov, ov)
    got = aa.annonet_infer(net, image(H, W), gains=class_gains(K), tiling_parameters=tp, want_blended=True)
    want = expected(K, H, W, max_tile, with_gains=True, shape=shape)
    check(got, want)
    assert len(np.unique(want[0])) > min(K, 8) // 2      # the label map is not one class


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


@pytest.mark.parametrize("shape", [NARROW, FULL], ids=SHAPE_IDS)
@pytest.mark.parametrize("K", MANY)
def test_fp32_training_step_matches_oracle_for_many_classes(K, shape):
    """The bars of test_fp32_training_step_matches_oracle; only the class count differs: the 1x1 head as a plain conv with cout = K,
    its backward-data reducing over K channels two per instruction (odd K, K > 32), loss_kernel<8> / <64>, K + 1 finalize workgroups."""
    levels, in_ch, scaler, minf = shape
    o, t = trainer_pair(levels, in_ch, K, scaler, minf, aa.ANH_FP32)
    rng = np.random.default_rng(40 + K)
    d = o.recommended_input_dim(21)
    img, lab, w, wl = make_batch(rng, 3, d, in_ch, K)
    assert set(range(K)) <= set(np.unique(lab).tolist()) and (lab == IGNORE).any()
    want_loss = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    got_loss = t.get_last_loss()
    assert abs(got_loss - want_loss) <= 2e-5 * max(1.0, abs(want_loss)), (got_loss, want_loss)
    g, gw = t.get_grads(), o.grads
    np.testing.assert_allclose(g, gw, rtol=2e-3, atol=2e-5 * np.abs(gw).max())
    p, _ = t.get_params()
    np.testing.assert_allclose(p, o.params, rtol=1e-4, atol=2e-6)


@pytest.mark.parametrize("K", [6, 9])
def test_bf16_forward_for_many_classes(K):
    """bars (a) of test_bf16_forward: the full-width net against the oracle restating the bf16 storage points"""
    levels, in_ch, scaler, minf = FULL
    o, net = pair(levels, in_ch, K, scaler, minf, aa.ANH_BF16)
    rng = np.random.default_rng(1)
    d = o.recommended_input_dim(45)
    img = rng.integers(0, 256, (2, d, d + (1 << levels), in_ch), dtype=np.uint8)
    got = net.Forward(img)
    o.set_bf16_emulation(1 if net.stores_activations() else 2)
    emu = o.forward(img)
    span = emu.max() - emu.min()
    mism = got.argmax(1) != emu.argmax(1)
    srt = np.sort(emu, axis=1)
    worst = (float(np.abs(got - emu).max() / span), float(np.abs(got - emu).mean() / span), float((srt[:, -1] - srt[:, -2])[mism].max(initial=0) / span), float(mism.mean()))
    print("bf16 forward, K = %d, vs the bf16-restating oracle (max / span, mean / span, widest flipped margin / span, label mismatches):" % K, worst)
    assert worst[0] <= 4e-3
    assert worst[1] <= 2e-4
    assert worst[2] <= 8e-3
    assert worst[3] <= 2e-3


@pytest.mark.parametrize("K", [6, 9])
def test_bf16_training_step_for_many_classes(K):
    """the bf16 bars of test_fused_head_kernel_for_every_class_count, beyond the fused head's four classes"""
    levels, in_ch, scaler, minf = FULL
    o, t = trainer_pair(levels, in_ch, K, scaler, minf, aa.ANH_BF16)
    rng = np.random.default_rng(40 + K)
    d = o.recommended_input_dim(21)
    img, lab, w, wl = make_batch(rng, 3, d, in_ch, K)
    o.set_bf16_emulation(True)
    want_loss = o.train_step(img, lab, w)
    t.StartTraining(list(img), wl)
    got_loss = t.get_last_loss()
    head = o.layers[-1]
    assert head.cout == K
    g, gw = t.get_grads(), o.grads
    loss_err = abs(got_loss - want_loss) / max(1.0, abs(want_loss))
    print("bf16 training step, K = %d: loss error %.3g" % (K, loss_err))
    assert loss_err <= 2e-3
    for name, sl in (("dW", slice(head.w_off, head.w_off + head.cin * head.cout)), ("db", slice(head.b_off, head.b_off + head.cout))):
        atol = 3e-3 * max(np.abs(gw[sl]).max(), 1e-12)
        excess = float((np.abs(g[sl] - gw[sl]) / (atol + 3e-2 * np.abs(gw[sl]))).max())
        print("bf16 training step, K = %d: head %s, largest |diff| / (atol + rtol |want|) = %.3g" % (K, name, excess))
        np.testing.assert_allclose(g[sl], gw[sl], rtol=3e-2, atol=atol)
