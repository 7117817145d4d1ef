"""bf16 inference in its activation-storing form, layer by layer: after a pass every bn layer's output still sits in the engine
(RuntimeNet.layer_tensor), so each layer is held to a float64 statement of that ONE layer applied to the input the GPU itself stored
(tests/infer_layer_ref.py: the operand roundings read from the kernels, bars derived from the arithmetic and proved on the CPU by
tests/test_infer_layer_bars.py).  Inputs are identical on both sides: every element gets the bar of one bf16 rounding, nothing compounds.

Every net is full width (scaler 1.0, min filters 1) with random parameters and running statistics; every case asserts the form it was
written for (stores_activations(), the tail's launch names).  Planes are the smallest that are ragged against the 8x32 (stride 1) and
4x32 (down / up) tiles in both directions, hold several tiles, and are exactly one tile high somewhere.
"""
import numpy as np
import pytest

import annonet_amd as aa
import infer_layer_ref as ref
from conftest import random_params
from test_infer_layer_bars import Shape

pytestmark = pytest.mark.gpu


def make_net(levels, in_ch, classes, seed):
    shape = Shape(levels, in_ch, classes)
    params, running = random_params(shape, seed)
    net = aa.RuntimeNet(aa.net_config(levels, in_ch, classes, 1.0, 1, aa.ANH_BF16))
    net.set_params(params, running)
    return shape.layers, params, running, net


def images(n, h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def stored_tensors(net, layers, missing=()):
    """the stored tensor of every bn layer; the layers in `missing` must NOT be available"""
    out = []
    for li in range(len(layers) - 1):
        if li in missing:
            with pytest.raises(aa.AnnonetHipError, match="tensor not available"):
                net.layer_tensor(li)
            out.append(None)
        else:
            out.append(net.layer_tensor(li))
    return out


def nhwc(planes):
    return np.ascontiguousarray(np.moveaxis(np.asarray(planes), -3, -1))


# ------------------------------------------------------------------------------------------------------------------
# RuntimeNet.Forward, two samples: every hidden layer and the generic head on the stored activation
# ------------------------------------------------------------------------------------------------------------------
#                  levels  in channels  K   h   w
FORWARD_CASES = [(0, 3, 3, 19, 45),
                 (1, 1, 2, 21, 77),       # grayscale stem
                 (2, 3, 3, 35, 71),       # the level-2 plane is 8 x 17
                 (3, 3, 4, 39, 79),       # 256 channels: four channel groups
                 (2, 3, 6, 35, 71)]       # many classes
MANY_TILES = (2, 3, 3, 227, 227)          # 464 stride-1 tiles on 256 workgroups: the persistent loop runs more than once


@pytest.mark.parametrize("levels,in_ch,classes,h,w", FORWARD_CASES + [MANY_TILES])
def test_forward_every_layer_on_its_stored_input(levels, in_ch, classes, h, w):
    layers, params, running, net = make_net(levels, in_ch, classes, seed=31 + levels)
    img = images(2, h, w, in_ch, seed=h * 1000 + w)
    net.profile_enable(True)
    logits = net.Forward(img)
    assert net.stores_activations()
    order = net.profile_launch_order()
    assert len(order) == len(layers) and all(name.startswith("conv_mfma_bf16:") for name in order[:-1]) and "_head_" in order[-1], order
    tensors = stored_tensors(net, layers)
    if (levels, h, w) == (2, 35, 71):
        assert tensors[4].shape == (2, 8, 17, 128)
    if levels == 3:
        assert tensors[6].shape[3] == 256
    x = ref.stem_input(img, [(0, 0, 0), (1, 0, 0)], h, w)
    report = ref.check_layers(layers, params, running, x, tensors, logits=nhwc(logits), name=f"Forward levels {levels} K {classes} {h}x{w}:")
    assert len(report) == len(layers)


# ------------------------------------------------------------------------------------------------------------------
# the three tails, through annonet_infer on a one-tile image (unique == full: the planes are the logits)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,classes,h,w,form", [(2, 3, 35, 71, "head in the epilogue"), (0, 3, 19, 45, "fused head + blend"), (2, 6, 35, 71, "generic head")])
def test_tails_of_tiled_inference(levels, classes, h, w, form):
    layers, params, running, net = make_net(levels, 3, classes, seed=41 + classes)
    img = images(1, h, w, 3, seed=77 + levels)
    net.profile_enable(True)
    _, planes = aa.annonet_infer(net, img[0], want_blended=True)
    assert net.stores_activations()
    order = net.profile_launch_order()
    convs = [name for name in order if name.startswith("conv_")]
    last_hidden = layers[-1].in_a
    x = ref.stem_input(img, [(0, 0, 0)], h, w)
    got = nhwc(planes[None])
    name = f"annonet_infer levels {levels} K {classes} ({form}):"
    if form == "head in the epilogue":
        assert len(convs) == len(layers) - 1 and not any("_head_" in c for c in convs) and "head_blend_fused" not in order and "blend_accumulate" in order, order
        tensors = stored_tensors(net, layers, missing=(last_hidden,))
        report = ref.check_layers(layers, params, running, x, tensors, epilogue_logits=got, name=name)
        assert len(report) == len(layers) - 1 and f"{len(layers) - 1} head in epilogue" in report
    elif form == "fused head + blend":
        assert order.count("head_blend_fused") == 1 and len(convs) == len(layers) - 1 and "blend_accumulate" not in order, order
        report = ref.check_layers(layers, params, running, x, stored_tensors(net, layers), logits=got, name=name)
        assert len(report) == len(layers)
    else:
        assert len(convs) == len(layers) and "_head_" in convs[-1] and "blend_accumulate" in order and "head_blend_fused" not in order, order
        report = ref.check_layers(layers, params, running, x, stored_tensors(net, layers), logits=got, name=name)
        assert len(report) == len(layers)


# ------------------------------------------------------------------------------------------------------------------
# tile batches (img_win) and image batches (img_idx)
# ------------------------------------------------------------------------------------------------------------------
def recommended_input_dim(levels, n):
    q = 1 << levels
    return q * max(1, -(-(n - (q - 1)) // q)) + q - 1


def tile_window(full, levels):
    """hostlogic.cpp tile_window: (left, top, height, width) of the net input of a tile with this full rectangle"""
    left, top, right, bottom = full
    fw, fh = right - left + 1, bottom - top + 1
    w, h = recommended_input_dim(levels, fw), recommended_input_dim(levels, fh)
    return left + fw // 2 - w // 2, top + fh // 2 - h // 2, h, w


@pytest.mark.parametrize("count", [5, 16])
def test_tile_batch_every_sample_reads_its_own_clamped_window(count):
    import torch
    levels, classes, H, W = 2, 3, 30, 40
    layers, params, running, net = make_net(levels, 3, classes, seed=51)
    img = images(1, H, W, 3, seed=52)
    corners = [(0, 0), (12, 0), (0, 10), (12, 10), (6, 5)] if count == 5 else [(left, top) for top in (0, 3, 7, 10) for left in (0, 4, 8, 12)]
    tiles = [((left, top, left + 27, top + 19),) * 2 for left, top in corners]        # 28 x 20 inside the image; the net input is 31 x 23
    windows = [tile_window(full, levels) for full, _ in tiles]
    assert len(tiles) == count and all(wd[2:] == (23, 31) for wd in windows)
    assert min(wd[0] for wd in windows) < 0 and min(wd[1] for wd in windows) < 0                      # the windows leave the image on all four sides
    assert max(wd[0] + 31 for wd in windows) > W and max(wd[1] + 23 for wd in windows) > H
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(img[0]).to(dev)
    d_lab = torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_planes = torch.zeros((classes, H, W), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    aa.annonet_infer_device(net, d_img.data_ptr(), H, W, d_lab.data_ptr(), d_planes.data_ptr(), tiles=tiles)
    net.synchronize()
    assert net.stores_activations()
    last_hidden = layers[-1].in_a
    tensors = stored_tensors(net, layers, missing=(last_hidden,))       # K = 3: the head rides in the last hidden layer's epilogue
    assert tensors[0].shape == (count, 23, 31, 32)                      # ONE batch
    x = ref.stem_input(img, [(0, left, top) for left, top, _, _ in windows], 23, 31)
    report = ref.check_layers(layers, params, running, x, tensors, name=f"tile batch of {count}:")
    assert len(report) == len(layers) - 2


def test_image_batch_sample_i_is_image_i():
    levels, classes, h, w, n = 2, 3, 35, 71, 5
    layers, params, running, net = make_net(levels, 3, classes, seed=61)
    img = images(n, h, w, 3, seed=62)
    _, planes = aa.annonet_infer_batch(net, img, want_blended=True)
    assert net.stores_activations()
    last_hidden = layers[-1].in_a
    tensors = stored_tensors(net, layers, missing=(last_hidden,))
    assert tensors[0].shape == (n, h, w, 32)                            # the five images ran as ONE batch
    x = ref.stem_input(img, [(i, 0, 0) for i in range(n)], h, w)
    report = ref.check_layers(layers, params, running, x, tensors, epilogue_logits=nhwc(np.stack(planes)), name="image batch of 5:")
    assert len(report) == len(layers) - 1


# ------------------------------------------------------------------------------------------------------------------
# the accessor itself
# ------------------------------------------------------------------------------------------------------------------
def test_layer_tensor_serves_only_what_the_last_pass_stored():
    layers, params, running, net = make_net(2, 3, 3, seed=71)
    n_layers = len(layers)
    for li in range(n_layers):                                           # before any pass
        with pytest.raises(aa.AnnonetHipError, match="tensor not available"):
            net.layer_tensor(li)
    img = images(1, 35, 71, 3, seed=72)
    net.Forward(img)
    assert net.stores_activations()
    last_hidden = layers[-1].in_a
    assert net.layer_tensor(last_hidden).shape == (1, 35, 71, 32)
    with pytest.raises(aa.AnnonetHipError, match="tensor not available"):
        net.layer_tensor(n_layers - 1)                                   # the head layer
    for li in (-1, n_layers):
        with pytest.raises(aa.AnnonetHipError, match="out of range"):
            net.layer_tensor(li)
    before = net.layer_tensor(0)
    aa.annonet_infer(net, img[0], want_blended=True)                     # the head now rides in the last hidden layer's epilogue:
    with pytest.raises(aa.AnnonetHipError, match="tensor not available"):
        net.layer_tensor(last_hidden)                                    # ... what Forward left there is stale, and is not served
    np.testing.assert_array_equal(net.layer_tensor(0), before)
    net.Forward(img)                                                     # the handle is as usable as before
    assert net.layer_tensor(last_hidden).shape == (1, 35, 71, 32)
