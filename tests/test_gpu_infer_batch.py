"""Batched inference over equal-sized images (anh_infer_batch and its mirrors): several images go through the net as the samples of
one forward, and the labels of single-tile images come straight from the batch's logits (anh_labels_from_logits_device).  A batch
member is the same arithmetic as the single-image call, so every comparison here is equality: fp32 against the oracle image by image,
bf16 against annonet_infer() of the image alone."""
import os
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
OV = 35            # TrainingNet::GetRequiredInputDimension() of a 2-level net
SMALL = (45, 61)   # one tile (window 47 x 63)
LARGE = (90, 140)  # 2 x 3 tiles of at most 64 x 64: frames, and batches that span image boundaries
ANH_ERR_OOM = 2


def tp(shape):
    return aa.tiling.parameters(64, 64, 10, 10) if shape == LARGE else None


def oracle_tiling(shape):
    return dict(max_tile=(64, 64), overlap=10) if shape == LARGE else dict(max_tile=(1024, 1024), overlap=OV)


def images_of(shape, n, seed=0):
    return np.random.default_rng(seed + 1000 * shape[0] + n).integers(0, 256, (n,) + shape + (3,), dtype=np.uint8)


def gains_of(k):
    return [0.0, 0.1, -0.05, 0.2, 0.0, 0.05][:k]


_NETS = {}


def narrow(k):
    """the narrow (8-channel) fp32 net with k classes, its oracle and its parameters"""
    if k not in _NETS:
        o = OracleNet(2, 3, k, 0.25, 8)
        p, r = random_params(o, 30 + k)
        o.params[:], o.running[:] = p, r
        net = aa.RuntimeNet(aa.net_config(2, 3, k, 0.25, 8, aa.ANH_FP32))
        net.set_params(p, r)
        _NETS[k] = (o, net, (p, r))
    return _NETS[k]


def full_bf16(k):
    key = ("bf16", k)
    if key not in _NETS:
        o = OracleNet(2, 3, k, 1.0, 1)
        p, r = random_params(o, 60 + k)
        net = aa.RuntimeNet(aa.net_config(2, 3, k, 1.0, 1, aa.ANH_BF16))
        net.set_params(p, r)
        _NETS[key] = (net, (p, r))
    return _NETS[key]


_WANT = {}


def oracle_results(k, shape, n, gains=None, detection_levels=None):
    """the oracle's (labels, planes) of every image of images_of(shape, n), computed once per case"""
    key = (k, shape, n, None if gains is None else tuple(gains), None if detection_levels is None else tuple(detection_levels))
    if key not in _WANT:
        o = narrow(k)[0]
        _WANT[key] = [o.infer(img, gains=gains, detection_levels=detection_levels, want_blended=True, **oracle_tiling(shape)) for img in images_of(shape, n)]
    return _WANT[key]


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
def find_label(logits, gains):
    """find_label (annonet_infer.cpp:170-185) on [K,H,W]: value = float(double(v) + gain), strict '>' from -inf, start label 65535"""
    best = np.full(logits.shape[1:], -np.inf, np.float32)
    label = np.full(logits.shape[1:], 65535, np.uint16)
    for c in range(logits.shape[0]):
        value = (logits[c].astype(np.float64) + (gains[c] if gains is not None else 0.0)).astype(np.float32)
        with np.errstate(invalid="ignore"):
            wins = value > best
        label[wins] = c
        best[wins] = value[wins]
    return label


# (window h, w), (image h, w): the window is centred on the image as tile_window() centres it
GEOMETRIES = [((47, 63), (45, 61)), ((47, 63), (47, 63)), ((67, 67), (64, 64)), ((67, 67), (65, 66))]


@pytest.mark.parametrize("k", [2, 3, 8, 9, 33])
@pytest.mark.parametrize("count", [1, 3, 16])
def test_labels_from_logits_kernel_equals_numpy(count, k):
    import torch
    net = narrow(3)[1]
    rng = np.random.default_rng(count * 100 + k)
    for (wh, ww), (H, W) in GEOMETRIES:
        top, left = H // 2 - wh // 2, W // 2 - ww // 2
        logits = rng.standard_normal((count, k, wh, ww)).astype(np.float32)
        ys, xs = rng.integers(0, wh, 60), rng.integers(0, ww, 60)
        for i in range(0, 20):      # exact ties between two classes at the top: the lowest index wins
            a, b = rng.choice(k, 2, replace=False)
            logits[i % count, [a, b], ys[i], xs[i]] = 9.0
        for i in range(20, 30):     # every class NaN: no class wins
            logits[i % count, :, ys[i], xs[i]] = np.nan
        for i in range(30, 40):     # one class NaN: it never wins
            logits[i % count, rng.integers(0, k), ys[i], xs[i]] = np.nan
        for i in range(40, 50):     # a class at -inf; and every class at -inf (nothing exceeds the start value)
            logits[i % count, rng.integers(0, k), ys[i], xs[i]] = -np.inf
        for i in range(50, 60):
            logits[i % count, :, ys[i], xs[i]] = -np.inf
        d_logits = torch.from_numpy(logits).cuda()
        inside = logits[:, :, -top:-top + H, -left:-left + W]
        for gains in (None, list(rng.uniform(-0.5, 0.5, k))):
            d_labels = torch.full((count * H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
            aa.labels_from_logits_device(net, d_logits.data_ptr(), count, k, wh, ww, top, left, H, W, d_labels.data_ptr(), gains=gains)
            net.synchronize()
            got = d_labels.cpu().numpy().view(np.uint16).reshape(count, H, W)
            want = np.stack([find_label(inside[s], gains) for s in range(count)])
            np.testing.assert_array_equal(got, want)
            assert (want == 65535).any()


def test_labels_from_logits_refuses_a_window_that_does_not_cover_the_image():
    import torch
    net = narrow(3)[1]
    d_logits = torch.zeros((1, 3, 47, 63), device="cuda")
    d_labels = torch.zeros((45 * 61,), dtype=torch.int16, device="cuda")
    for top, left, H, W in ((1, -1, 45, 61), (-1, -1, 47, 61), (-1, -3, 45, 61)):
        with pytest.raises(aa.AnnonetHipError, match="does not cover the image"):
            aa.labels_from_logits_device(net, d_logits.data_ptr(), 1, 3, 47, 63, top, left, H, W, d_labels.data_ptr())


# ---- 2. fp32 against the oracle ---------------------------------------------------------------------------------------------------
def check_against_oracle(k, shape, n, gains=None):
    net = narrow(k)[1]
    imgs = images_of(shape, n)
    want = oracle_results(k, shape, n, gains)
    labels = aa.annonet_infer_batch(net, imgs, gains=gains, tiling_parameters=tp(shape))
    with_planes, planes = aa.annonet_infer_batch(net, imgs, gains=gains, tiling_parameters=tp(shape), want_blended=True)
    for i in range(n):
        np.testing.assert_array_equal(labels[i], want[i][0])
        np.testing.assert_array_equal(with_planes[i], want[i][0])
        assert planes[i].tobytes() == want[i][1].tobytes()


@pytest.mark.parametrize("n", [1, 2, 5, 17])
@pytest.mark.parametrize("k", [3, 5])
def test_single_tile_images_equal_the_oracle(k, n):
    check_against_oracle(k, SMALL, n)


@pytest.mark.parametrize("k", [3, 5])
def test_tiled_images_equal_the_oracle(k):
    check_against_oracle(k, LARGE, 3)


@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 2), (SMALL, 5), (SMALL, 17), (LARGE, 3)])
@pytest.mark.parametrize("k", [3, 5])
def test_gains_equal_the_oracle(k, shape, n):
    check_against_oracle(k, shape, n, gains=gains_of(k))


@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 17), (LARGE, 3)])
@pytest.mark.parametrize("k", [3, 5])
def test_device_form_on_dirty_buffers(k, shape, n):
    import torch
    net = narrow(k)[1]
    H, W = shape
    imgs = images_of(shape, n)
    gains = gains_of(k)
    want = oracle_results(k, shape, n, gains)
    stream = torch.cuda.ExternalStream(net.stream_ptr())
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(imgs).cuda()
        d_labels = torch.full((n * H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_only = torch.full((n * H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_planes = torch.full((n, k, H, W), float("nan"), dtype=torch.float32, device="cuda")
        aa.annonet_infer_batch_device(net, d_img.data_ptr(), n, H, W, d_labels.data_ptr(), d_planes.data_ptr(), gains=gains, tiling_parameters=tp(shape))
        aa.annonet_infer_batch_device(net, d_img.data_ptr(), n, H, W, d_only.data_ptr(), gains=gains, tiling_parameters=tp(shape))
        stream.synchronize()
    got, only, planes = d_labels.cpu().numpy().view(np.uint16).reshape(n, H, W), d_only.cpu().numpy().view(np.uint16).reshape(n, H, W), d_planes.cpu().numpy()
    for i in range(n):
        np.testing.assert_array_equal(got[i], want[i][0])
        np.testing.assert_array_equal(only[i], want[i][0])
        assert planes[i].tobytes() == want[i][1].tobytes()


@pytest.mark.parametrize("shape,n", [(SMALL, 5), (LARGE, 3)])
def test_detection_levels_equal_annonet_infer_per_image(shape, n):
    o, net, _ = narrow(3)
    imgs = images_of(shape, n)
    det = [0.0, 1.0, 1.0]
    got = aa.annonet_infer_batch(net, imgs, detection_levels=det, tiling_parameters=tp(shape))
    plain = aa.annonet_infer_batch(net, imgs, tiling_parameters=tp(shape))
    changed = False
    for i in range(n):
        np.testing.assert_array_equal(got[i], aa.annonet_infer(net, imgs[i], detection_levels=det, tiling_parameters=tp(shape)))
        changed = changed or (got[i] != plain[i]).any()
    assert changed      # the filter changes something at these levels


def test_fast_path_and_planes_path_give_the_same_labels():
    for net in (narrow(3)[1], full_bf16(3)[0]):
        imgs = images_of(SMALL, 7, seed=3)
        direct = aa.annonet_infer_batch(net, imgs)
        through_planes, _ = aa.annonet_infer_batch(net, imgs, want_blended=True)
        mixed, planes = aa.annonet_infer_batch(net, imgs, want_blended=[False, True] + [False] * 5)
        assert planes[0] is None and planes[1] is not None
        for i in range(7):
            np.testing.assert_array_equal(direct[i], through_planes[i])
            np.testing.assert_array_equal(direct[i], mixed[i])


def launch_order(net, imgs, **kw):
    net.profile_enable(True)
    try:
        aa.annonet_infer_batch(net, imgs, **kw)
        return net.profile_launch_order()
    finally:
        net.profile_enable(False)


def test_the_launches_of_a_batch():
    """what the feature is for: 17 single-tile frames are two forwards and two label launches; three 6-tile images are two forwards of nine"""
    for net in (narrow(3)[1], full_bf16(3)[0]):
        order = launch_order(net, images_of(SMALL, 17))
        assert sum(":fwd_L0_" in name for name in order) == 2
        assert order.count("labels_from_logits") == 2
        assert not any(name in ("blend_accumulate", "head_blend_fused", "argmax_gain") for name in order)
        order = launch_order(net, images_of(SMALL, 17), want_blended=True)      # through the planes: blends, then ONE label launch for all 17 maps
        assert sum(":fwd_L0_" in name for name in order) == 2
        assert order.count("blend_accumulate") == 2 and order.count("labels_from_logits") == 1 and order[-1] == "labels_from_logits"
        order = launch_order(net, images_of(LARGE, 3), tiling_parameters=tp(LARGE))   # 18 equal windows: 9 + 9, the first batch ends inside image 1
        assert sum(":fwd_L0_" in name for name in order) == 2
        assert order.count("blend_accumulate") == 2 and order.count("labels_from_logits") == 1


# ---- 3. bf16: a batch member is the image alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 6])      # 3: head in the conv epilogue, blend_batch, labels from logits; 6: the generic head, per-tile blends
@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 2), (SMALL, 5), (SMALL, 17), (LARGE, 3)])
def test_bf16_batch_members_equal_the_image_alone(k, shape, n):
    net = full_bf16(k)[0]
    imgs = images_of(shape, n)
    alone = [aa.annonet_infer(net, img, tiling_parameters=tp(shape), want_blended=True) for img in imgs]
    labels = aa.annonet_infer_batch(net, imgs, tiling_parameters=tp(shape))
    with_planes, planes = aa.annonet_infer_batch(net, imgs, tiling_parameters=tp(shape), want_blended=True)
    for i in range(n):
        np.testing.assert_array_equal(labels[i], alone[i][0])
        np.testing.assert_array_equal(with_planes[i], alone[i][0])
        assert planes[i].tobytes() == alone[i][1].tobytes()
    if n >= 3:      # the same images in a batch of another size and at other positions
        order = [2, 0, 1][:n] + list(range(3, min(n, 4)))
        again, again_planes = aa.annonet_infer_batch(net, imgs[order], tiling_parameters=tp(shape), want_blended=True)
        for at, i in enumerate(order):
            np.testing.assert_array_equal(again[at], alone[i][0])
            assert again_planes[at].tobytes() == alone[i][1].tobytes()
        for at, i in enumerate(order):
            np.testing.assert_array_equal(aa.annonet_infer_batch(net, imgs[order], tiling_parameters=tp(shape))[at], alone[i][0])


# ---- 4. two replicas rehearsed on one GPU -------------------------------------------------------------------------------------------
# (a single tiled image on two replicas is served by anh_infer's sharded path, which has its own tests and its known near-ties where
# tiles of two replicas meet: the bit-for-bit case with fewer images than replicas is the single-tile one)
@pytest.mark.parametrize("shape,counts", [(SMALL, (5, 1)), (LARGE, (5,))])
def test_two_replicas(shape, counts):
    _, one, (p, r) = narrow(3)
    aa.set_devices([0, 0])
    try:
        net = aa.RuntimeNet(aa.net_config(2, 3, 3, 0.25, 8, aa.ANH_FP32))
    finally:
        aa.set_devices([])
    assert net.L.anh_handle_replicas(net.h, 0) == 2
    net.set_params(p, r)
    for n in counts:
        imgs = images_of(shape, n)
        want, want_planes = aa.annonet_infer_batch(one, imgs, gains=gains_of(3), tiling_parameters=tp(shape), want_blended=True)
        got, planes = aa.annonet_infer_batch(net, imgs, gains=gains_of(3), tiling_parameters=tp(shape), want_blended=True)
        only = aa.annonet_infer_batch(net, imgs, gains=gains_of(3), tiling_parameters=tp(shape))
        for i in range(n):
            np.testing.assert_array_equal(only[i], want[i])
            np.testing.assert_array_equal(got[i], want[i])
            assert planes[i].tobytes() == want_planes[i].tobytes()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_that_cannot_fit_is_ANH_ERR_OOM_and_the_handle_infers_on():
    import torch
    # 64 classes on one input channel: the planes of an image are 256 times its own bytes, so a batch whose planes exceed the whole device
    # memory by a quarter is still only ~0.5 % of it as images.  The arrays handed over really hold n images: the call is refused while
    # its buffers are reserved, and if it ever were not, its kernels would stay inside them.
    K, H, W = 64, 200, 200                                  # four tiles of at most 128: the labels need the images' planes
    o = OracleNet(2, 1, K, 0.25, 8)
    p, r = random_params(o, 77)
    o.params[:], o.running[:] = p, r
    net = aa.RuntimeNet(aa.net_config(2, 1, K, 0.25, 8, aa.ANH_FP32))
    net.set_params(p, r)
    total = torch.cuda.mem_get_info()[1]
    n = int(1.25 * total / (K * 4 * H * W)) + 1
    assert n * K * 4 * H * W > total and n * H * W * 3 < 0.02 * total
    d_images = torch.zeros((n, H, W, 1), dtype=torch.uint8, device="cuda")
    d_labels = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
    with pytest.raises(aa.AnnonetHipError) as err:
        aa.annonet_infer_batch_device(net, d_images.data_ptr(), n, H, W, d_labels.data_ptr(), tiling_parameters=aa.tiling.parameters(128, 128, 10, 10))
    assert err.value.code == ANH_ERR_OOM and "memory" in str(err.value).lower()
    del d_images, d_labels
    imgs = np.random.default_rng(9).integers(0, 256, (3, H, W, 1), dtype=np.uint8)      # the same handle infers a batch that fits
    got = aa.annonet_infer_batch(net, imgs, tiling_parameters=aa.tiling.parameters(128, 128, 10, 10))
    for i in range(3):
        np.testing.assert_array_equal(got[i], o.infer(imgs[i], max_tile=(128, 128), overlap=10))


def test_bad_arguments_are_errors():
    net = narrow(3)[1]
    with pytest.raises(aa.AnnonetHipError, match="at least one image"):
        aa.annonet_infer_batch(net, [])
    with pytest.raises(aa.AnnonetHipError, match="one size"):
        aa.annonet_infer_batch(net, [np.zeros((45, 61, 3), np.uint8), np.zeros((45, 60, 3), np.uint8)])
    with pytest.raises(aa.AnnonetHipError, match="channel count"):
        aa.annonet_infer_batch(net, [np.zeros((45, 61), np.uint8)])


# ---- 6. the C++ drop-in header --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n,tile", [(SMALL, 5, 1024), (LARGE, 3, 64)])
def test_cpp_header_annonet_infer_batch(tmp_path, shape, n, tile):
    net = narrow(3)[1]
    exe = str(tmp_path / "infer_batch_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "infer_batch_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    imgs = images_of(shape, n)
    H, W = shape
    (tmp_path / "net.bin").write_bytes(net.Serialize())
    (tmp_path / "images.raw").write_bytes(imgs.tobytes())
    r = subprocess.run([exe, str(tmp_path / "net.bin"), str(tmp_path / "images.raw"), str(n), str(H), str(W), str(tile), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want, want_planes = aa.annonet_infer_batch(net, imgs, tiling_parameters=aa.tiling.parameters(tile, tile, 10, 10), want_blended=True)
    assert r.stdout.split() == [str(n), str(H), str(W), "3"]
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.labels.raw").read_bytes(), np.uint16).reshape(n, H, W), np.stack(want))
    assert (tmp_path / "out.planes.raw").read_bytes() == want_planes[-1].tobytes()


# ---- 7. the inference program ---------------------------------------------------------------------------------------------------------
def test_infer_program_image_batch(tmp_path):
    _, net, _ = narrow(3)
    d = tmp_path / "frames"
    d.mkdir()
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", 1.0, net.Serialize()))
    rng = np.random.default_rng(11)
    # five frames of 60 x 80 and two of 50 x 50, interleaved by name: groups of 2, 1, 2, 1, 1 at --image-batch 4
    names = [("f1.png", (60, 80)), ("f2.png", (60, 80)), ("f3.png", (50, 50)), ("f4.png", (60, 80)), ("f5.png", (60, 80)), ("f6.png", (50, 50)), ("f7.png", (60, 80))]
    for name, (h, w) in names:
        pu.write_png(d / name, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), filter_type=1)
        gt = np.zeros((h, w), np.uint16)
        for _ in range(6):
            y, x = rng.integers(0, h), rng.integers(0, w)
            gt[y:y + rng.integers(5, 30), x:x + rng.integers(5, 30)] = rng.integers(0, 3)
        gt[rng.random((h, w)) < 0.3] = 65535
        pu.write_png(str(d / name) + "_mask.png", pu.labels_to_rgba(gt))

    def run(batch):
        r = subprocess.run([TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "--precision", "fp32", "--full-image-reader-thread-count", "1", "--image-batch", str(batch)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "All 7 images processed" in r.stdout and "All result images written!" in r.stdout
        pngs = {}
        for name, _ in names:
            pngs[name] = open(str(d / name) + "_result.png", "rb").read()
            os.remove(str(d / name) + "_result.png")
        lines = r.stdout.splitlines()
        return pngs, lines[lines.index("Confusion matrix per pixel:"):]
    one_by_one, matrices = run(1)
    batched, batched_matrices = run(4)
    assert batched == one_by_one
    assert batched_matrices == matrices
    assert len(matrices) > 8 and any(ch.isdigit() and ch != "0" for line in matrices for ch in line)
