"""The bf16 training convolutions, one kernel at a time, held to the float64 statement of tests/train_conv_ref.py: forward with the three
prologues, backward-data plain and into a tensor that holds a gradient already, the filter gradient with the three prologues, the stem's
filter gradient with dy given and with dy formed in the kernel.  tests/test_train_conv_bars.py proves on the CPU that an fp32 emulation
passes these bars and which kernel mistakes break them.

Every case asserts its bars, that the output is finite, and its KERNEL FORM.  EXPECT is written from mfma_conv_supported, stem_mfma_ok,
stem_wgrad_mfma_ok and mfma_wgrad_supported (kernels_mfma.hip), per (layer, op) = (forward, backward-data, filter gradient):
  * a 3x3 layer whose channel counts are in {32, 64, 128, 256} runs all three on the matrix cores (backward-data of a stride-2 con layer is
    the transposed gather, which needs an odd input side: every plane here has one);
  * 8 -> 16 and 40 -> 24 (c_red % 32 != 0) and the 1x1 heads (k != 3, fp32 logits under a bias) run the generic kernels;
  * the stem's matrix-core kernels read the u8 image (SRC_IMAGE).  anh_op_conv_forward and anh_op_conv_backward_filter stage a float tensor
    (SRC_RAW), so through them the 5x5 layer is a generic conv — EXPECT says so — and the stem kernels themselves are reached through the
    entry points that take the image: op_conv_forward_stats_table(image=...) (it refuses to run anything but the MFMA kernel) and
    op_conv_backward_filter_bn.  Its backward-data does not exist in the net and is generic.
A mismatch with this table is a finding about kernel selection, not a reason to edit the table.
Backward-data into an existing gradient (ConvArgs::out_accumulate) is the skip gradient's form: it runs where the net uses it, on the layers
whose backward-data is expected on the matrix cores.
"""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import train_conv_ref as ref
from train_ops_ref import bf16_round

pytestmark = pytest.mark.gpu

BF = aa.ANH_BF16
F32, F64 = np.float32, np.float64
SHAPES = ref.SHAPES
M, G = True, False
#                              forward  backward-data  filter gradient
EXPECT = {
    (0, 5, 1, 2, 3, 32):       (G, G, G),     # through the float-tensor entry points; the image entry points: see above
    (0, 3, 1, 1, 32, 32):      (M, M, M),
    (0, 3, 1, 1, 64, 64):      (M, M, M),
    (0, 3, 1, 1, 128, 128):    (M, M, M),
    (0, 3, 2, 0, 32, 64):      (M, M, M),
    (0, 3, 2, 0, 64, 128):     (M, M, M),
    (1, 3, 2, 0, 128, 64):     (M, M, M),
    (1, 3, 2, 0, 64, 32):      (M, M, M),
    (0, 3, 1, 1, 256, 256):    (M, M, M),
    (0, 3, 2, 0, 128, 256):    (M, M, M),
    (1, 3, 2, 0, 256, 128):    (M, M, M),
    (0, 1, 1, 0, 32, 3):       (G, G, G),
    (0, 3, 1, 1, 8, 16):       (G, G, G),
    (0, 3, 1, 1, 40, 24):      (G, G, G),
    (0, 1, 1, 0, 32, 5):       (G, G, G),
    (0, 1, 1, 0, 32, 9):       (G, G, G),
    (0, 1, 1, 0, 32, 33):      (G, G, G),
    (0, 1, 1, 0, 32, 64):      (G, G, G),
    (0, 1, 1, 0, 8, 9):        (G, G, G),
}
ACCUMULATING = [s for s in SHAPES if EXPECT[s[0]][1]]


def tag_of(what, desc, n, h, w):
    return "%s %s n%d %dx%d" % (what, desc, n, h, w)


def form(flag):
    return "matrix cores" if flag else "generic"


def assert_form(tag, got, want):
    assert got == want, f"{tag}: ran on the {form(got)} kernel, expected the {form(want)} one"


@pytest.mark.parametrize("prologue", [0, 1, 2])
@pytest.mark.parametrize("desc,n,h,w", SHAPES)
def test_forward(desc, n, h, w, prologue):
    tag = tag_of("forward p%d" % prologue, desc, n, h, w)
    xa, kw, filters, rng = ref.make_inputs(desc, n, h, w, 1, prologue)
    bias = rng.uniform(-0.1, 0.1, desc[5]).astype(F32) if desc[1] == 1 else None
    got, mfma = aa.op_conv_forward(BF, desc, xa, filters=filters, bias=bias, **kw)
    r = ref.forward(desc, ref.staged(xa, **kw), filters, bias)
    out = ref.check_stored(tag, got, r, stored_bf16=bias is None)
    ref.report(tag + " [" + form(mfma) + "]", *out)
    assert_form(tag, mfma, EXPECT[desc][0])


@pytest.mark.parametrize("desc,n,h,w", [SHAPES[0], ((0, 5, 1, 2, 3, 32), 3, 21, 43), ((0, 5, 1, 2, 1, 32), 2, 19, 37)])
def test_stem_forward_on_the_image(desc, n, h, w):
    """the stem's own kernel (stem_mfma_kernel), which reads the u8 image: the entry point launches the MFMA kernel or fails"""
    tag = tag_of("stem forward on the image", desc, n, h, w)
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (n, h, w, desc[4]), dtype=np.uint8)
    lim = np.sqrt(6.0 / (25 * (desc[4] + 32)))
    filters = rng.uniform(-lim, lim, 25 * desc[4] * 32).astype(F32)
    got = aa.op_conv_forward_stats_table(BF, desc, image=img, filters=filters, tables=False)["y"]
    out = ref.check_stored(tag, got, ref.forward(desc, img.astype(F64) / 256.0, filters))
    ref.report(tag + " [matrix cores]", *out)


def backward_inputs(desc, n, h, w):
    _, _, filters, rng = ref.make_inputs(desc, n, h, w, 2, 0)
    return filters, ref.make_dy(desc, n, h, w, rng), rng


@pytest.mark.parametrize("desc,n,h,w", SHAPES)
def test_backward_data(desc, n, h, w):
    tag = tag_of("backward-data", desc, n, h, w)
    filters, dy, _ = backward_inputs(desc, n, h, w)
    got, mfma = aa.op_conv_backward_data(BF, desc, dy, filters, (h, w))
    out = ref.check_stored(tag, got, ref.backward_data(desc, dy, filters, (h, w)))
    ref.report(tag + " [" + form(mfma) + "]", *out)
    assert_form(tag, mfma, EXPECT[desc][1])


@pytest.mark.parametrize("desc,n,h,w", ACCUMULATING)
def test_backward_data_into_a_gradient(desc, n, h, w):
    """dx_init: bf16(old + q) bit for bit, q = what the same call stores without the old tensor, itself held to the element bar"""
    tag = tag_of("backward-data into a gradient", desc, n, h, w)
    filters, dy, rng = backward_inputs(desc, n, h, w)
    cin = desc[4]
    old, y_prev = (bf16_round(rng.normal(0, 1, (n, h, w, cin)).astype(F32)) for _ in range(2))
    scale, shift = rng.uniform(0.5, 1.5, cin).astype(F32), rng.uniform(-0.3, 0.3, cin).astype(F32)
    mean, invstd = rng.uniform(-0.2, 0.2, cin).astype(F32), rng.uniform(0.7, 1.4, cin).astype(F32)
    q, _, _ = aa.op_conv_backward_data_bn(BF, desc, dy, filters, (h, w), y_prev, scale, shift, mean, invstd)
    got, _, _ = aa.op_conv_backward_data_bn(BF, desc, dy, filters, (h, w), y_prev, scale, shift, mean, invstd, dx_init=old)
    plain, mfma = aa.op_conv_backward_data(BF, desc, dy, filters, (h, w))
    out = ref.check_stored(tag + ", q", q, ref.backward_data(desc, dy, filters, (h, w)))
    assert np.isfinite(got).all(), tag
    ref.check_accumulated(tag, got, old, q)
    assert np.array_equal(q, plain), tag + ": the reduction in the epilogue changed the stored gradient"
    ref.report(tag + " [" + form(mfma) + "], q", *out)
    assert_form(tag, mfma, True)


def check_filter_gradient(tag, desc, x, dy, got, mfma, want_mfma, allowance=None):
    r = ref.filter_grad(desc, x, dy, allowance)
    worst, ratio = ref.check_filter_grad(tag, desc, got, r, ref.seq_filter_grad(desc, x, dy))
    ref.report(tag + " [" + form(mfma) + "]", worst, rms_ratio=ratio)
    assert_form(tag, mfma, want_mfma)


@pytest.mark.parametrize("prologue", [0, 1, 2])
@pytest.mark.parametrize("desc,n,h,w", SHAPES)
def test_filter_gradient(desc, n, h, w, prologue):
    tag = tag_of("filter gradient p%d" % prologue, desc, n, h, w)
    xa, kw, _, rng = ref.make_inputs(desc, n, h, w, 3, prologue)
    dy = ref.make_dy(desc, n, h, w, rng, 1e-3)
    got, mfma = aa.op_conv_backward_filter(BF, desc, xa, dy=dy, **kw)
    check_filter_gradient(tag, desc, ref.staged(xa, **kw), dy, got, mfma, EXPECT[desc][2])


@functools.lru_cache(maxsize=None)
def stem_inputs(n, h, w, cin=3):
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (n, h, w, cin), dtype=np.uint8)
    da = bf16_round(rng.normal(0, 1, (n, h, w, 32)).astype(F32))
    y = bf16_round(rng.normal(0, 1, (n, h, w, 32)).astype(F32))
    scale, shift = rng.uniform(0.5, 1.5, 32).astype(F32), rng.uniform(-0.3, 0.3, 32).astype(F32)
    mean, invstd = rng.uniform(-0.2, 0.2, 32).astype(F32), rng.uniform(0.7, 1.4, 32).astype(F32)
    coef = np.concatenate([rng.uniform(0.5, 1.5, 32), rng.uniform(-0.01, 0.01, 32), rng.uniform(-0.01, 0.01, 32)]).astype(F32)
    for a in (img, da, y, scale, shift, mean, invstd, coef):
        a.setflags(write=False)
    return img, da, y, scale, shift, mean, invstd, coef


@pytest.mark.parametrize("n,h,w,cin", [(3, 21, 43, 3), (2, 19, 23, 3), (2, 19, 37, 1)])
def test_stem_filter_gradient_with_dy_formed_in_the_kernel(n, h, w, cin):
    """wgrad_stem_mfma_kernel<CIN, true> on the u8 image: dy = bf16(k0 * (dz - k1 - xhat * k2)) while staging"""
    desc = (0, 5, 1, 2, cin, 32)
    tag = tag_of("stem filter gradient, dy in the kernel", desc, n, h, w)
    img, da, y, scale, shift, mean, invstd, coef = stem_inputs(n, h, w, cin)
    got, in_kernel = aa.op_conv_backward_filter_bn(BF, desc, img, da, y, scale, shift, mean, invstd, coef)
    x = img.astype(F64) / 256.0
    dyq, flip = ref.stem_dy(da, y, mean, invstd, scale, shift, coef)
    check_filter_gradient(tag, desc, x, dyq, got, in_kernel, True, ref.tap_sums(desc, np.abs(x), flip))
