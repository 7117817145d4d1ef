"""How the host-buffer inference calls are composed, at the level of launches (profile_launch_order): a scaled call is a shrink, the
launches of the unscaled call on the shrunk image and a blow-up; a regions call is the launches of annonet_infer() and then the region
table; factor 1.0 is the unscaled call.  What the calls compute is held bit for bit elsewhere (test_gpu_scaled_infer*.py,
test_gpu_infer_batch.py, test_gpu_infer_regions.py); this file only pins which launches a call is made of, so that the one body under
the five entry points (api.cpp: run_share) cannot drift from what each of them launched when it had a body of its own.

The launch order is that of the most recent pass, and a pass begins where the forward begins (Engine::infer_device and
infer_batch_device clear it): the shrink in front of the forward is therefore not part of the order.  It is pinned through the profiler's
entries instead, which count every launch since profile_reset()."""
import numpy as np
import pytest

import annonet_amd as aa
import resize_util as ru
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

SMALL = (90, 122)    # at factor 2: 45 x 61, one tile
LARGE = (180, 280)   # at factor 2: 90 x 140, 2 x 3 tiles of at most 64 x 64
_NETS = {}


def tp(shape):
    return aa.tiling.parameters(64, 64, 10, 10) if shape == LARGE else None


def images_of(shape, n):
    return np.random.default_rng(1000 * shape[0] + n).integers(0, 256, (n,) + shape + (3,), dtype=np.uint8)


def net_of(kind):
    """"fp32": the narrow (8-channel) fp32 net of the batch tests; "bf16": the full-width bf16 net; 3 classes each"""
    if kind not in _NETS:
        scaler, minf, precision, seed = (0.25, 8, aa.ANH_FP32, 33) if kind == "fp32" else (1.0, 1, aa.ANH_BF16, 63)
        net = aa.RuntimeNet(aa.net_config(2, 3, 3, scaler, minf, precision))
        net.set_params(*random_params(OracleNet(2, 3, 3, scaler, minf), seed))
        _NETS[kind] = net
    return _NETS[kind]


def launched(net, fn):
    """(launch order of the last pass fn() ran, {profiler entry: launches since fn() began})"""
    net.profile_enable(True)
    try:
        net.profile_reset()
        fn()
        return net.profile_launch_order(), {e["name"]: e["launches"] for e in net.profile()}
    finally:
        net.profile_enable(False)


KINDS = ["fp32", "bf16"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_a_scaled_call_is_shrink_then_the_unscaled_call_then_blow_up(kind, shape):
    net = net_of(kind)
    img = images_of(shape, 1)[0]
    inner, _ = launched(net, lambda: aa.annonet_infer(net, ru.shrink(img, 2.0), tiling_parameters=tp(shape), want_blended=True))
    order, count = launched(net, lambda: aa.annonet_infer_scaled(net, img, 2.0, tiling_parameters=tp(shape), want_blended=True))
    assert inner and inner[-1] == "argmax_gain"
    assert order == inner + ["resize_labels_nearest"]
    assert count["resize_image_bilinear"] == 1 and count["resize_labels_nearest"] == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,n", [(SMALL, 1), (SMALL, 5), (LARGE, 1)])
def test_a_scaled_batch_is_shrink_then_the_unscaled_batch_then_blow_up(kind, shape, n):
    net = net_of(kind)
    imgs = images_of(shape, n)
    shrunk = [ru.shrink(img, 2.0) for img in imgs]
    for kw in ({}, {"want_blended": True}):
        inner, _ = launched(net, lambda: aa.annonet_infer_batch(net, shrunk, tiling_parameters=tp(shape), **kw))
        order, count = launched(net, lambda: aa.annonet_infer_scaled_batch(net, imgs, 2.0, tiling_parameters=tp(shape), **kw))
        assert inner and not any(name == "argmax_gain" for name in inner)     # a batch of one is still the batch form
        assert order == inner + ["resize_labels_nearest"]
        assert count["resize_image_bilinear"] == 1 and count["resize_labels_nearest"] == 1      # ONE launch each for all n images


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_a_regions_call_begins_with_the_launches_of_annonet_infer(kind, shape):
    net = net_of(kind)
    img = ru.shrink(images_of(shape, 1)[0], 2.0)
    inner, _ = launched(net, lambda: aa.annonet_infer(net, img, tiling_parameters=tp(shape), want_blended=True))
    order, _ = launched(net, lambda: aa.annonet_infer_regions(net, img, tiling_parameters=tp(shape)))
    assert inner and order[:len(inner)] == inner
    assert order[len(inner):] == ["label_blobs", "blob_regions"]


@pytest.mark.parametrize("kind", KINDS)
def test_factor_one_is_the_unscaled_call(kind):
    net = net_of(kind)
    imgs = [ru.shrink(img, 2.0) for img in images_of(LARGE, 3)]
    t = tp(LARGE)
    want, _ = launched(net, lambda: aa.annonet_infer(net, imgs[0], tiling_parameters=t, want_blended=True))
    got, count = launched(net, lambda: aa.annonet_infer_scaled(net, imgs[0], 1.0, tiling_parameters=t, want_scaled=True, want_blended=True))
    assert want and got == want and "resize_image_bilinear" not in count and "resize_labels_nearest" not in count
    for kw in ({}, {"want_blended": True}):
        want, _ = launched(net, lambda: aa.annonet_infer_batch(net, imgs, tiling_parameters=t, **kw))
        got, count = launched(net, lambda: aa.annonet_infer_scaled_batch(net, imgs, 1.0, tiling_parameters=t, want_scaled=True, **kw))
        assert want and got == want and "resize_image_bilinear" not in count and "resize_labels_nearest" not in count
