"""The per-layer bars of tests/infer_layer_ref.py, proved without a GPU: an emulated kernel passes every one of them, and each of a list
of subtle kernel mistakes fails one.

The emulation is what the activation-storing kernels do, in torch / numpy float32 on the same operands: an fp32 conv of the bf16 operands,
the bn constants folded in fp32 as Engine::fold_running_stats folds them, one fp32 multiply-add, relu, round to nearest even to bf16.  The
net is the levels-1 full-width net (stem 5x5, 3x3 s2 to 64 channels, 3x3 s1, transposed 3x3 s2, 3x3 s1 with skip, head) on two 21 x 45
images: every plane is ragged against the 8x32 and 4x32 tiles, and every layer has more than 10^4 positive outputs, so the rounding
statistics are asserted on every layer.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import annonet_amd as aa
import infer_layer_ref as ref
from conftest import random_params
from train_ops_ref import bf16_round

F32, F64 = np.float32, np.float64
H, W = 21, 45


class Shape:
    """layer list and blob sizes of a net configuration (what conftest.random_params reads)"""

    def __init__(self, levels, in_ch, classes):
        cfg = aa.net_config(levels, in_ch, classes, 1.0, 1, aa.ANH_BF16)
        self.layers = aa.net_layers(cfg)
        self.n_params = aa.lib().anh_net_param_count(C.byref(cfg))
        self.n_running = aa.lib().anh_net_running_count(C.byref(cfg))


@functools.lru_cache(maxsize=None)
def case():
    shape = Shape(1, 3, 3)
    params, running = random_params(shape, 5)
    images = np.random.default_rng(11).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    for a in (params, running, images):
        a.setflags(write=False)
    return shape.layers, params, running, images


def truncate_bf16(a):
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def conv_f32(L, x_nhwc, w):
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=F32)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w, dtype=F32))
    y = F.conv2d(x, wt, stride=L.stride, padding=L.pad) if L.type == 0 else F.conv_transpose2d(x, wt, stride=L.stride, padding=L.pad)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def fold_f32(L, params, running):
    """Engine::fold_running_stats: invstd = 1 / sqrt(var + eps), scale = gamma * invstd, shift = fmaf(-mean, scale, beta), all fp32"""
    g, b = params[L.g_off:L.g_off + L.cout], params[L.beta_off:L.beta_off + L.cout]
    rm, rv = running[L.rs_off:L.rs_off + L.cout], running[L.rs_off + L.cout:L.rs_off + 2 * L.cout]
    scale = g * (F32(1) / np.sqrt(rv + F32(ref.BN_EPS)))
    return scale, (b.astype(F64) - rm.astype(F64) * scale.astype(F64)).astype(F32)


def stem_samples(mut):
    """(image, left, top) of the two samples: whole images, or 21 x 45 windows that leave the image on every side"""
    if mut in ("window", "late_clamp", "sample0_window"):
        return [(0, -2, -1), (1, 3, 2)]
    return [(0, 0, 0), (1, 0, 0)]


def emulate(mut=None):
    """-> (x of the stem as the reference states it, stored tensors, logits); `mut` names one mistake of the emulated kernels"""
    layers, params, running, images = case()
    samples = stem_samples(mut)
    x_true = ref.stem_input(images, samples, H, W)
    if mut == "sample0_window":                   # sample 1 reads sample 0's window (of its own image)
        x_stem = ref.stem_input(images, [samples[0], (1,) + samples[0][1:]], H, W)
    elif mut == "late_clamp":                     # the window is clamped one pixel late: row / column 1 (H - 2) stands where the edge should
        inner = images[:, 1:-1, 1:-1]
        x_stem = ref.stem_input(inner, [(i, left - 1, top - 1) for i, left, top in samples], H, W)
    else:
        x_stem = x_true
    tensors = []
    for li, L in enumerate(layers[:-1]):
        if L.in_a < 0:
            x = x_stem.astype(F32)
        elif L.in_b < 0:
            x = tensors[L.in_a]
        elif mut == "skip_not_rounded":           # the fp32 sum goes to the conv as it is
            x = tensors[L.in_a] + tensors[L.in_b]
        else:
            x = bf16_round(tensors[L.in_a] + tensors[L.in_b])
        acc = conv_f32(L, x, ref.filters(L, params))
        scale, shift = fold_f32(L, params, running)
        if mut == "affine_xor1" and ref.kind(L) == "con3x3s1":
            scale, shift = scale[np.arange(L.cout) ^ 1], shift[np.arange(L.cout) ^ 1]
        if mut == "affine_plus32" and L.cout == 64:
            scale, shift = np.roll(scale, -32), np.roll(shift, -32)
        v = (acc.astype(F64) * scale.astype(F64) + shift.astype(F64)).astype(F32)      # one fp32 multiply-add
        if mut != "no_relu":
            v = np.maximum(v, F32(0))
        out = truncate_bf16(v) if mut == "truncate" else bf16_round(v)
        if mut == "tile_column" and ref.kind(L) == "con3x3s1":     # the last valid column of the second 32-wide tile, from its neighbour
            out = out.copy()
            out[:, :, out.shape[2] - 1] = out[:, :, out.shape[2] - 2]
        tensors.append(out)
    head = layers[-1]
    w, bias = ref.head_weights(head, params)
    logits = tensors[head.in_a] @ w.T.astype(F32) + bias.astype(F32)
    return x_true, tensors, logits


def run_checks(mut=None, epilogue=False):
    layers, params, running, _ = case()
    x, tensors, logits = emulate(mut)
    if epilogue:     # the last hidden layer is not stored; the logits come out of its epilogue
        tensors = [None if li == layers[-1].in_a else t for li, t in enumerate(tensors)]
        return ref.check_layers(layers, params, running, x, tensors, epilogue_logits=logits, name=str(mut))
    return ref.check_layers(layers, params, running, x, tensors, logits=logits, name=str(mut))


def test_net_has_one_layer_of_each_kind():
    layers = case()[0]
    assert [ref.kind(L) for L in layers] == ["stem", "con3x3s2", "con3x3s1", "cont3x3s2", "con3x3s1", "head"]
    assert [L.cout for L in layers] == [32, 64, 64, 32, 32, 3] and layers[4].in_b == 0


@pytest.mark.parametrize("form", [None, "window"])
def test_emulated_kernels_pass_every_bar(form):
    report = run_checks(form)
    assert len(report) == 6 and max(report.values()) < 1.0, report
    report = run_checks(form, epilogue=True)
    assert len(report) == 5 and "5 head in epilogue" in report and max(report.values()) < 1.0, report


def test_rounding_statistics_ran_on_every_layer():
    layers, params, running, _ = case()
    x, tensors, _ = emulate()
    for li, L in enumerate(layers[:-1]):
        xin = x if L.in_a < 0 else tensors[L.in_a] if L.in_b < 0 else ref.skip_sum(tensors[L.in_a], tensors[L.in_b])
        worst, mean_e, mean_abs, count = ref.check_hidden(f"layer {li}", tensors[li], ref.hidden(L, params, running, xin))
        assert count >= ref.MIN_STAT and abs(mean_e) < 0.01 and 0.24 < mean_abs < 0.26, (li, worst, mean_e, mean_abs, count)
        # the statistic on its own: truncation sits half an ulp low, far beyond the 0.02 the bar allows
        pos = tensors[li] > 0
        e = (truncate_bf16(np.nextafter(tensors[li][pos], F32(0))).astype(F64) - tensors[li][pos]) / ref.bf16_ulp(tensors[li][pos].astype(F64))
        assert e.mean() < -0.9          # (a stored bf16 value, truncated from just below itself, is one whole ulp low)


MUTATIONS = ["truncate", "no_relu", "affine_xor1", "affine_plus32", "tile_column", "skip_not_rounded", "sample0_window", "late_clamp"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_mistake_fails_a_bar(mut):
    with pytest.raises(AssertionError) as e:
        run_checks(mut)
    assert "worst error / bound" in str(e.value) and "layer" in str(e.value)
    print(e.value)


@pytest.mark.parametrize("mut", ["no_relu", "affine_xor1", "sample_swap"])
def test_mistakes_under_the_head_in_the_epilogue_fail_its_bar(mut):
    """The last hidden layer's activation is not stored there, so its mistakes must show in the logits.  (That bar allows every channel
    half an ulp at once: it cannot see a rounding mode, which the stored layers' own bars hold.)"""
    layers, params, running, _ = case()
    x, good, _ = emulate()
    head = layers[-1]
    L = layers[head.in_a]
    acc = conv_f32(L, bf16_round(good[L.in_a] + good[L.in_b]), ref.filters(L, params))
    scale, shift = fold_f32(L, params, running)
    if mut == "affine_xor1":
        scale, shift = scale[np.arange(L.cout) ^ 1], shift[np.arange(L.cout) ^ 1]
    v = (acc.astype(F64) * scale.astype(F64) + shift.astype(F64)).astype(F32)
    act = bf16_round(v if mut == "no_relu" else np.maximum(v, F32(0)))
    w, bias = ref.head_weights(head, params)
    logits = act @ w.T.astype(F32) + bias.astype(F32)
    if mut == "sample_swap":
        logits = logits[::-1]
    stored = [None if li == head.in_a else t for li, t in enumerate(good)]
    with pytest.raises(AssertionError) as e:
        ref.check_layers(layers, params, running, x, stored, epilogue_logits=logits, name=mut)
    assert "head in the epilogue" in str(e.value) and "worst error / bound" in str(e.value)
