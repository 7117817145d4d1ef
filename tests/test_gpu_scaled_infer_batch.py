"""Batched downscaled inference (anh_infer_scaled_batch and its mirrors): n images of one original size are shrunk by one launch, go
through the net as the samples of annonet_infer_batch()'s forwards and their label maps are blown up by one launch.  Everything is
integer-valued and a batch member is the arithmetic of the single-image call, so every comparison is equality: the two batched resizes
against their numpy restatements image by image, fp32 end to end against the oracle (shrink -> annonet_infer -> nearest neighbour, as
tests/test_gpu_scaled_infer.py::oracle_scaled states it), bf16 against annonet_infer_scaled() of the image alone."""
import os
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
import resize_util as ru
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
OV = 35              # TrainingNet::GetRequiredInputDimension() of a 2-level net
SMALL = (90, 122)    # at factor 2: 45 x 61, one tile
LARGE = (180, 280)   # at factor 2: 90 x 140, 2 x 3 tiles of at most 64 x 64
ANH_ERR_OOM = 2


def tp(shape):
    return aa.tiling.parameters(64, 64, 10, 10) if shape == LARGE else None


def oracle_tiling(shape):
    return dict(max_tile=(64, 64), overlap=10) if shape == LARGE else dict(max_tile=(1024, 1024), overlap=OV)


def images_of(shape, n, seed=0):
    return np.random.default_rng(seed + 1000 * shape[0] + n).integers(0, 256, (n,) + shape + (3,), dtype=np.uint8)


GAINS = [0.0, 0.1, -0.05]
_NETS = {}


def narrow():
    """the narrow (8-channel) fp32 net with 3 classes of the batch tests, its oracle and its parameters"""
    if "fp32" not in _NETS:
        o = OracleNet(2, 3, 3, 0.25, 8)
        p, r = random_params(o, 33)
        o.params[:], o.running[:] = p, r
        net = aa.RuntimeNet(aa.net_config(2, 3, 3, 0.25, 8, aa.ANH_FP32))
        net.set_params(p, r)
        _NETS["fp32"] = (o, net, (p, r))
    return _NETS["fp32"]


def full_bf16():
    if "bf16" not in _NETS:
        o = OracleNet(2, 3, 3, 1.0, 1)
        p, r = random_params(o, 63)
        net = aa.RuntimeNet(aa.net_config(2, 3, 3, 1.0, 1, aa.ANH_BF16))
        net.set_params(p, r)
        _NETS["bf16"] = net
    return _NETS["bf16"]


_WANT = {}


def oracle_results(shape, n, factor, gains=None):
    """per image of images_of(shape, n): (original-size map, map at the net's resolution, planes at the net's resolution), as the
    reference's program computes them; computed once per case and left unchanged"""
    key = (shape, n, factor, None if gains is None else tuple(gains))
    if key not in _WANT:
        o = narrow()[0]
        out = []
        for img in images_of(shape, n):
            scaled, planes = o.infer(ru.shrink(img, factor), gains=gains, want_blended=True, **oracle_tiling(shape))
            out.append((pu.resize_nearest(scaled, shape[1], shape[0]), scaled, planes))
        _WANT[key] = out
    return _WANT[key]


# ---- 1. the two kernels against numpy -----------------------------------------------------------------------------------------------
# (source height, width), (destination height, width).  The per-image strides are off the store boundaries: (97, 131) -> (49, 66) is
# 9702 bytes at 3 channels (2 mod 4) and its blown-up map has 12707 labels (odd: with 8 images or more the maps start at every one of
# the 8 `back` values); (1, 57) -> (1, 29) has strides of 29 and 87 bytes (every `head` value within four images).
def half(shape):
    return (ru.scaled_size(shape[0], 0.5), ru.scaled_size(shape[1], 0.5))


KERNEL_CASES = [((97, 131), half((97, 131))), ((1, 57), half((1, 57))), ((61, 1), half((61, 1))),
                ((3, 90), (ru.scaled_size(3, 1 / 2.9), ru.scaled_size(90, 1 / 2.9))),      # a single output row
                ((40, 30), (80, 60))]                                                      # enlarges the image
assert KERNEL_CASES[0][1] == (49, 66) and KERNEL_CASES[1][1] == (1, 29) and KERNEL_CASES[3][1][0] == 1


def check_image_batch(count, channels, src, dst):
    rng = np.random.default_rng(count * 7 + channels + src[0] * 31 + src[1])
    imgs = rng.integers(0, 256, (count,) + src + (channels,), dtype=np.uint8)      # the images of a batch all differ
    want = np.stack([ru.bilinear_to(img, dst[0], dst[1]) for img in imgs])
    for garbage in (0xAB, 0x00):   # a destination element the kernel leaves out keeps one of the two fills
        got = aa.resize_image_batch(imgs, dst[0], dst[1], prefill=garbage)
        assert got.shape == (count,) + dst + (channels,)
        np.testing.assert_array_equal(got, want)
    if channels == 1:
        np.testing.assert_array_equal(aa.resize_image_batch(imgs[..., 0], dst[0], dst[1], prefill=0x5C), want[..., 0])
    if count == 1:
        np.testing.assert_array_equal(aa.resize_image(imgs[0], dst[0], dst[1], prefill=0xAB), got[0])


def check_labels_batch(count, src, dst):
    rng = np.random.default_rng(count * 5 + src[0] * 3 + src[1])
    maps = rng.integers(0, 7, (count,) + src).astype(np.uint16)
    maps[rng.random(maps.shape) < 0.2] = 65535
    want = np.stack([pu.resize_nearest(m, dst[1], dst[0]) for m in maps])
    assert (want == 65535).any()
    for garbage in (0xAB, 0x00):
        got = aa.resize_labels_batch(maps, dst[1], dst[0], prefill=garbage)
        assert got.shape == (count,) + dst
        np.testing.assert_array_equal(got, want)
    if count == 1:
        np.testing.assert_array_equal(aa.resize_labels(maps[0], dst[1], dst[0], prefill=0xAB), got[0])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("count", [1, 3, 16])
@pytest.mark.parametrize("src,dst", KERNEL_CASES)
def test_resize_image_batch_kernel_equals_numpy(src, dst, count, channels):
    check_image_batch(count, channels, src, dst)


@pytest.mark.parametrize("count", [1, 3, 16])
@pytest.mark.parametrize("src,dst", KERNEL_CASES)
def test_resize_labels_batch_kernel_equals_numpy(src, dst, count):
    # the direction inference uses: maps at the net's resolution (dst) blown up to the original size (src); and the reverse
    check_labels_batch(count, dst, src)
    check_labels_batch(count, src, dst)


@pytest.mark.parametrize("channels", [1, 3])
def test_resize_image_batch_more_than_one_chunk_per_row(channels):
    check_image_batch(2, channels, (40, 2300), (20, 1150))      # 1150 columns: 290 units of 4 pixels, two chunks of 256
    check_image_batch(2, channels, (20, 1150), (40, 2300))


def test_resize_labels_batch_more_than_one_chunk_per_row():
    check_labels_batch(2, (20, 1150), (40, 2300))               # 2300 columns: two chunks of 2048
    check_labels_batch(2, (40, 2300), (20, 1150))


@pytest.mark.parametrize("channels", [1, 3])
def test_resize_image_batch_grid_stride_second_round(channels):
    check_image_batch(17, channels, (130, 95), (260, 190))      # 17 * 260 = 4420 items on a grid of 4096 workgroups


def test_resize_labels_batch_grid_stride_second_round():
    check_labels_batch(17, (130, 95), (260, 190))               # (the shape of the image case: 17 * 9 bands)
    # 4100 maps of one band and one chunk each: 4100 items on a grid of 4096 workgroups.  All maps share their source positions, which
    # the numpy restatement gives once, on a map of indices.
    rng = np.random.default_rng(41)
    maps = rng.integers(0, 7, (4100, 2, 3)).astype(np.uint16)
    maps[rng.random(maps.shape) < 0.2] = 65535
    index = pu.resize_nearest(np.arange(6, dtype=np.uint16).reshape(2, 3), 5, 3)
    want = maps.reshape(4100, 6)[:, index.reshape(-1)].reshape(4100, 3, 5)
    np.testing.assert_array_equal(want[7], pu.resize_nearest(maps[7], 5, 3))
    for garbage in (0xAB, 0x00):
        np.testing.assert_array_equal(aa.resize_labels_batch(maps, 5, 3, prefill=garbage), want)


# ---- 2. fp32 end to end against the oracle --------------------------------------------------------------------------------------------
def check_against_oracle(shape, n, factor, gains=None):
    net = narrow()[1]
    imgs = images_of(shape, n)
    want = oracle_results(shape, n, factor, gains)
    labels = aa.annonet_infer_scaled_batch(net, imgs, factor, gains=gains, tiling_parameters=tp(shape))      # labels only: the direct path where every image is one tile
    full, scaled, planes = aa.annonet_infer_scaled_batch(net, imgs, factor, gains=gains, tiling_parameters=tp(shape), want_scaled=True, want_blended=True)
    only_scaled, scaled_direct = aa.annonet_infer_scaled_batch(net, imgs, factor, gains=gains, tiling_parameters=tp(shape), want_scaled=True)
    assert len(labels) == len(full) == len(scaled) == len(planes) == n
    for i in range(n):
        assert labels[i].shape == shape and scaled[i].shape == aa.scaled_dims(shape[0], shape[1], factor)
        np.testing.assert_array_equal(scaled[i], want[i][1])
        np.testing.assert_array_equal(scaled_direct[i], want[i][1])
        np.testing.assert_array_equal(labels[i], want[i][0])
        np.testing.assert_array_equal(full[i], want[i][0])
        np.testing.assert_array_equal(only_scaled[i], want[i][0])
        assert planes[i].tobytes() == want[i][2].tobytes()


@pytest.mark.parametrize("gains", [None, GAINS])
@pytest.mark.parametrize("n", [1, 2, 5, 17])
def test_single_tile_images_equal_the_oracle(n, gains):
    check_against_oracle(SMALL, n, 2.0, gains)


@pytest.mark.parametrize("gains", [None, GAINS])
def test_tiled_images_equal_the_oracle(gains):
    check_against_oracle(LARGE, 3, 2.0, gains)


@pytest.mark.parametrize("shape,n,factor", [(SMALL, 3, 1.5), (LARGE, 2, 3.7)])
def test_other_factors_equal_the_oracle(shape, n, factor):
    check_against_oracle(shape, n, factor, GAINS)


def test_optional_outputs_per_image():
    net = narrow()[1]
    imgs = images_of(SMALL, 5)
    want = oracle_results(SMALL, 5, 2.0)
    got, scaled, planes = aa.annonet_infer_scaled_batch(net, imgs, 2.0, want_scaled=[False, True, False, False, True], want_blended=[False, False, True, False, False])
    assert [s is None for s in scaled] == [True, False, True, True, False] and [p is None for p in planes] == [True, True, False, True, True]
    for i in range(5):
        np.testing.assert_array_equal(got[i], want[i][0])
    np.testing.assert_array_equal(scaled[1], want[1][1])
    np.testing.assert_array_equal(scaled[4], want[4][1])
    assert planes[2].tobytes() == want[2][2].tobytes()


# ---- 3. the device form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 17), (LARGE, 3)])
def test_device_form_on_dirty_buffers(shape, n):
    import torch
    net = narrow()[1]
    H, W = shape
    sh, sw = aa.scaled_dims(H, W, 2.0)
    imgs = images_of(shape, n)
    want = oracle_results(shape, n, 2.0, GAINS)
    stream = torch.cuda.ExternalStream(net.stream_ptr())
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(imgs).cuda()
        dirty = lambda count: torch.full((count * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_labels, d_only, d_with_scaled = dirty(n * H * W), dirty(n * H * W), dirty(n * H * W)
        d_scaled, d_scaled_only = dirty(n * sh * sw), dirty(n * sh * sw)
        d_planes = torch.full((n, 3, sh, sw), float("nan"), dtype=torch.float32, device="cuda")
        aa.annonet_infer_scaled_batch_device(net, d_img.data_ptr(), n, H, W, 2.0, d_labels.data_ptr(), d_scaled.data_ptr(), d_planes.data_ptr(), gains=GAINS, tiling_parameters=tp(shape))
        aa.annonet_infer_scaled_batch_device(net, d_img.data_ptr(), n, H, W, 2.0, d_only.data_ptr(), gains=GAINS, tiling_parameters=tp(shape))
        aa.annonet_infer_scaled_batch_device(net, d_img.data_ptr(), n, H, W, 2.0, d_with_scaled.data_ptr(), d_scaled_only.data_ptr(), gains=GAINS, tiling_parameters=tp(shape))
        stream.synchronize()
    maps = lambda t, h, w: t.cpu().numpy().view(np.uint16).reshape(n, h, w)
    planes = d_planes.cpu().numpy()
    for i in range(n):
        for t in (d_labels, d_only, d_with_scaled):
            np.testing.assert_array_equal(maps(t, H, W)[i], want[i][0])
        for t in (d_scaled, d_scaled_only):
            np.testing.assert_array_equal(maps(t, sh, sw)[i], want[i][1])
        assert planes[i].tobytes() == want[i][2].tobytes()


# ---- 4. detection levels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [(SMALL, 5), (LARGE, 3)])
def test_detection_levels_equal_annonet_infer_scaled_per_image(shape, n):
    net = narrow()[1]
    imgs = images_of(shape, n)
    det = [0.0, 1.0, 1.0]
    got, scaled = aa.annonet_infer_scaled_batch(net, imgs, 2.0, detection_levels=det, tiling_parameters=tp(shape), want_scaled=True)
    plain = oracle_results(shape, n, 2.0)
    changed = False
    for i in range(n):
        alone, alone_scaled = aa.annonet_infer_scaled(net, imgs[i], 2.0, detection_levels=det, tiling_parameters=tp(shape), want_scaled=True)
        np.testing.assert_array_equal(got[i], alone)
        np.testing.assert_array_equal(scaled[i], alone_scaled)
        changed = changed or (alone != plain[i][0]).any()
    assert changed      # the filter changes something at these levels


# ---- 5. factor 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [((45, 61), 5), ((90, 140), 3)])
def test_factor_one_is_annonet_infer_batch(shape, n):
    net = narrow()[1]
    tiling = aa.tiling.parameters(64, 64, 10, 10) if shape == (90, 140) else None
    imgs = images_of(shape, n)
    want, want_planes = aa.annonet_infer_batch(net, imgs, gains=GAINS, tiling_parameters=tiling, want_blended=True)
    got, scaled, planes = aa.annonet_infer_scaled_batch(net, imgs, 1.0, gains=GAINS, tiling_parameters=tiling, want_scaled=True, want_blended=True)
    only = aa.annonet_infer_scaled_batch(net, imgs, 1.0, gains=GAINS, tiling_parameters=tiling)
    for i in range(n):
        np.testing.assert_array_equal(got[i], want[i])
        np.testing.assert_array_equal(scaled[i], got[i])
        np.testing.assert_array_equal(only[i], want[i])
        assert planes[i].tobytes() == want_planes[i].tobytes()


def test_factor_one_device_form():
    import torch
    net = narrow()[1]
    n, (H, W) = 5, (45, 61)
    imgs = images_of((H, W), n)
    want = aa.annonet_infer_batch(net, imgs)
    stream = torch.cuda.ExternalStream(net.stream_ptr())
    with torch.cuda.stream(stream):
        d_img = torch.from_numpy(imgs).cuda()
        d_labels = torch.full((n * H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        d_scaled = torch.full((n * H * W * 2,), 0xAB, dtype=torch.uint8, device="cuda")
        aa.annonet_infer_scaled_batch_device(net, d_img.data_ptr(), n, H, W, 1.0, d_labels.data_ptr(), d_scaled.data_ptr())
        stream.synchronize()
    np.testing.assert_array_equal(d_labels.cpu().numpy().view(np.uint16).reshape(n, H, W), np.stack(want))
    np.testing.assert_array_equal(d_scaled.cpu().numpy().view(np.uint16).reshape(n, H, W), np.stack(want))


# ---- 6. bf16: a batch member is the image alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 5), (SMALL, 17), (LARGE, 3)])
def test_bf16_batch_members_equal_the_image_alone(shape, n):
    net = full_bf16()
    imgs = images_of(shape, n)
    alone = [aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp(shape), want_scaled=True, want_blended=True) for img in imgs]
    labels = aa.annonet_infer_scaled_batch(net, imgs, 2.0, tiling_parameters=tp(shape))
    full, scaled, planes = aa.annonet_infer_scaled_batch(net, imgs, 2.0, tiling_parameters=tp(shape), want_scaled=True, want_blended=True)
    for i in range(n):
        np.testing.assert_array_equal(labels[i], alone[i][0])
        np.testing.assert_array_equal(full[i], alone[i][0])
        np.testing.assert_array_equal(scaled[i], alone[i][1])
        assert planes[i].tobytes() == alone[i][2].tobytes()
    if n >= 3:      # the same images in a batch of another size and at other positions
        order = [2, 0, 1] + list(range(3, min(n, 4)))
        again, again_scaled, again_planes = aa.annonet_infer_scaled_batch(net, imgs[order], 2.0, tiling_parameters=tp(shape), want_scaled=True, want_blended=True)
        direct = aa.annonet_infer_scaled_batch(net, imgs[order], 2.0, tiling_parameters=tp(shape))
        for at, i in enumerate(order):
            np.testing.assert_array_equal(again[at], alone[i][0])
            np.testing.assert_array_equal(again_scaled[at], alone[i][1])
            assert again_planes[at].tobytes() == alone[i][2].tobytes()
            np.testing.assert_array_equal(direct[at], alone[i][0])


# ---- 7. the launches of a batch ---------------------------------------------------------------------------------------------------------
def launches(net, fn):
    """profiler entries of the launches fn() enqueues: name -> (launches, bytes)"""
    net.profile_enable(True)
    try:
        net.profile_reset()
        fn()
        return {e["name"]: (e["launches"], e["bytes"]) for e in net.profile()}
    finally:
        net.profile_enable(False)


def test_the_launches_of_a_batch():
    """what the feature is for: 17 single-tile frames are ONE shrink, two forwards and ONE blow-up; the per-image loop is 17 of each.  The
    two resizes are entered with the bytes of all their images."""
    per_image = {"resize_image_bilinear": (90 * 122 + 45 * 61) * 3, "resize_labels_nearest": (90 * 122 + 45 * 61) * 2}
    for net in (narrow()[1], full_bf16()):
        imgs = images_of(SMALL, 17)
        batch = launches(net, lambda: aa.annonet_infer_scaled_batch(net, imgs, 2.0))
        loop = launches(net, lambda: [aa.annonet_infer_scaled(net, img, 2.0) for img in imgs])
        for name, nbytes in per_image.items():
            assert batch[name] == (1, 17 * nbytes)
            assert loop[name] == (17, 17 * nbytes)
        assert sum(count for name, (count, _) in batch.items() if ":fwd_L0_" in name) == 2
        assert sum(count for name, (count, _) in loop.items() if ":fwd_L0_" in name) == 17


# ---- 8. two replicas rehearsed on one GPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,counts", [(SMALL, (5, 1)), (LARGE, (5,))])
def test_two_replicas(shape, counts):
    _, one, (p, r) = narrow()
    aa.set_devices([0, 0])
    try:
        net = aa.RuntimeNet(aa.net_config(2, 3, 3, 0.25, 8, aa.ANH_FP32))
    finally:
        aa.set_devices([])
    assert net.L.anh_handle_replicas(net.h, 0) == 2
    net.set_params(p, r)
    for n in counts:
        imgs = images_of(shape, n)
        want, want_scaled, want_planes = aa.annonet_infer_scaled_batch(one, imgs, 2.0, gains=GAINS, tiling_parameters=tp(shape), want_scaled=True, want_blended=True)
        got, scaled, planes = aa.annonet_infer_scaled_batch(net, imgs, 2.0, gains=GAINS, tiling_parameters=tp(shape), want_scaled=True, want_blended=True)
        only = aa.annonet_infer_scaled_batch(net, imgs, 2.0, gains=GAINS, tiling_parameters=tp(shape))
        for i in range(n):
            np.testing.assert_array_equal(only[i], want[i])
            np.testing.assert_array_equal(got[i], want[i])
            np.testing.assert_array_equal(scaled[i], want_scaled[i])
            assert planes[i].tobytes() == want_planes[i].tobytes()


# ---- 9. errors --------------------------------------------------------------------------------------------------------------------------
def test_a_batch_that_cannot_fit_is_ANH_ERR_OOM_and_the_handle_infers_on():
    import torch
    # 64 classes on one input channel, as the batch's own test of this: the planes of n images exceed the whole device memory by a quarter.
    # At factor 2 the planes of an image are 64 * 4 * sh * sw bytes and the image and map handed over 3 * H * W: 3 H W / (64 * 4 sh sw) * 1.25
    # stays below 5 % where H W / (sh sw) < 3.41, which an even height cannot give (it is 4).  5 rows become 3 (2.5 rounds up): 3.33.
    # The arrays handed over really hold n images: the call is refused while its buffers are reserved, and if it ever were not, its
    # kernels would stay inside them.
    K, H, W = 64, 5, 600
    sh, sw = aa.scaled_dims(H, W, 2.0)
    assert (sh, sw) == (3, 300)
    tiling = aa.tiling.parameters(128, 128, 10, 10)                 # three tiles: the labels need the images' planes
    assert len(aa.tiling.get_tiles(sw, sh, tiling)) >= 2
    o = OracleNet(2, 1, K, 0.25, 8)
    p, r = random_params(o, 77)
    o.params[:], o.running[:] = p, r
    net = aa.RuntimeNet(aa.net_config(2, 1, K, 0.25, 8, aa.ANH_FP32))
    net.set_params(p, r)
    total = torch.cuda.mem_get_info()[1]
    n = int(1.25 * total / (K * 4 * sh * sw)) + 1
    assert n * K * 4 * sh * sw > 1.25 * total and n * H * W * (1 + 2) < 0.05 * total
    d_images = torch.zeros((n, H, W, 1), dtype=torch.uint8, device="cuda")
    d_labels = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
    with pytest.raises(aa.AnnonetHipError) as err:
        aa.annonet_infer_scaled_batch_device(net, d_images.data_ptr(), n, H, W, 2.0, d_labels.data_ptr(), tiling_parameters=tiling)
    assert err.value.code == ANH_ERR_OOM and "memory" in str(err.value).lower()
    del d_images, d_labels
    imgs = np.random.default_rng(9).integers(0, 256, (3, H, W, 1), dtype=np.uint8)      # the same handle infers a batch that fits
    got, scaled = aa.annonet_infer_scaled_batch(net, imgs, 2.0, tiling_parameters=tiling, want_scaled=True)
    for i in range(3):
        want_scaled = o.infer(ru.shrink(imgs[i], 2.0), max_tile=(128, 128), overlap=10)
        np.testing.assert_array_equal(scaled[i], want_scaled)
        np.testing.assert_array_equal(got[i], pu.resize_nearest(want_scaled, W, H))


def test_bad_arguments_are_errors():
    net = narrow()[1]
    with pytest.raises(aa.AnnonetHipError, match="at least one image"):
        aa.annonet_infer_scaled_batch(net, [], 2.0)
    with pytest.raises(aa.AnnonetHipError, match="one size"):
        aa.annonet_infer_scaled_batch(net, [np.zeros((90, 122, 3), np.uint8), np.zeros((90, 120, 3), np.uint8)], 2.0)
    with pytest.raises(aa.AnnonetHipError, match="channel count"):
        aa.annonet_infer_scaled_batch(net, [np.zeros((90, 122), np.uint8)], 2.0)
    with pytest.raises(aa.AnnonetHipError, match="too small for this downscaling factor"):
        aa.annonet_infer_scaled_batch(net, images_of(SMALL, 2), 400.0)
    want = oracle_results(SMALL, 2, 2.0)
    got = aa.annonet_infer_scaled_batch(net, images_of(SMALL, 2), 2.0)      # the handle is still usable
    for i in range(2):
        np.testing.assert_array_equal(got[i], want[i][0])


# ---- 10. the C++ drop-in header -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n,tile", [(SMALL, 5, 1024), (LARGE, 3, 64)])
def test_cpp_header_annonet_infer_scaled_batch(tmp_path, shape, n, tile):
    net = narrow()[1]
    exe = str(tmp_path / "scaled_infer_batch_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scaled_infer_batch_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    imgs = images_of(shape, n)
    H, W = shape
    sh, sw = aa.scaled_dims(H, W, 2.0)
    (tmp_path / "net.bin").write_bytes(net.Serialize())
    (tmp_path / "images.raw").write_bytes(imgs.tobytes())
    r = subprocess.run([exe, str(tmp_path / "net.bin"), str(tmp_path / "images.raw"), str(n), str(H), str(W), "2", str(tile), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want, want_scaled, want_planes = aa.annonet_infer_scaled_batch(net, imgs, 2.0, tiling_parameters=aa.tiling.parameters(tile, tile, 10, 10), want_scaled=True, want_blended=True)
    assert r.stdout.split() == [str(n), str(H), str(W), str(n), str(sh), str(sw), "3"]
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.labels.raw").read_bytes(), np.uint16).reshape(n, H, W), np.stack(want))
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.scaled.raw").read_bytes(), np.uint16).reshape(n, sh, sw), np.stack(want_scaled))
    assert (tmp_path / "out.planes.raw").read_bytes() == want_planes[-1].tobytes()


# ---- 11. the inference program ---------------------------------------------------------------------------------------------------------
def test_infer_program_image_batch_with_a_downscaled_net(tmp_path):
    _, net, _ = narrow()
    d = tmp_path / "frames"
    d.mkdir()
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", 2.0, net.Serialize()))
    rng = np.random.default_rng(11)
    # five frames of 120 x 161 and two of 100 x 100, interleaved by name: groups of 2, 1, 2, 1, 1 at --image-batch 4
    names = [("f1.png", (120, 161)), ("f2.png", (120, 161)), ("f3.png", (100, 100)), ("f4.png", (120, 161)), ("f5.png", (120, 161)), ("f6.png", (100, 100)), ("f7.png", (120, 161))]
    for name, (h, w) in names:
        pu.write_png(d / name, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), filter_type=1)
        gt = np.zeros((h, w), np.uint16)      # at the ORIGINAL size: the program resizes it to the net's resolution
        for _ in range(6):
            y, x = rng.integers(0, h), rng.integers(0, w)
            gt[y:y + rng.integers(10, 60), x:x + rng.integers(10, 60)] = rng.integers(0, 3)
        gt[rng.random((h, w)) < 0.3] = 65535
        pu.write_png(str(d / name) + "_mask.png", pu.labels_to_rgba(gt))

    def run(batch):
        r = subprocess.run([TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "--precision", "fp32", "--full-image-reader-thread-count", "1", "--image-batch", str(batch)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "downscaling factor = 2" in r.stdout
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
