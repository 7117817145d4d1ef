"""The evaluation tally on constructed logits (anh_eval_logits_device) against tests/eval_ref.py.

Counts, counted, unclassified, the matrices and the predicted map are exact.  loss_sum / pixels lies within 2e-5 * max(1, |want / pixels|)
of the float64 reference on the same logits — the bar tests/test_gpu_train_ops.py::test_loss holds loss_kernel to, whose arithmetic the
term follows; the logits and weights are drawn as they are there.  weight_sum lies within 1e-12 relative of the float64 sum of the fp32
weights (the kernel adds exact doubles: at most 33 x 258 roundings of 1.1e-16 each).

Shapes: K 1..64 on both sides of the 4-wide path's limit of 8; maps from one pixel to 33 x 258 = 8514 pixels, which is three of the
tally's 4096-pixel workgroups; every map starts one element into its buffer, so label and predicted maps are 2-byte aligned, the
8-byte boundary falls inside the span and the plane loads are dword-aligned only.  Content: exact ties (the first class wins), all-NaN
and all -inf pixels under real labels, ignore labels, a wholly ignored image, zero weights.  Outputs are prefilled with garbage, and
the scratch is dirtied by a call on other data between two runs that must agree bit for bit."""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import eval_ref as er

pytestmark = pytest.mark.gpu

CLASSES = [1, 3, 5, 8, 9, 64]
SHAPES = [(1, 1), (1, 7), (3, 5), (37, 41), (33, 258)]
INVALID = 1


@functools.lru_cache(maxsize=None)
def case(K, shape, n):
    H, W = shape
    P = H * W
    rng = np.random.default_rng(K * 1000 + P * 7 + n)
    z = rng.uniform(-30, 30, (n, P, K)).astype(np.float32)
    z[rng.random((n, P)) < 0.5] *= 0.1                              # half the pixels undecided, as test_loss draws them
    z = np.ascontiguousarray(z.transpose(0, 2, 1))                  # [n, K, P]
    y = rng.integers(0, K, (n, P)).astype(np.uint16)
    y[rng.random((n, P)) < 0.05] = er.IGNORE
    w = rng.uniform(0.5, 2.0, (n, P)).astype(np.float32)
    w[rng.random((n, P)) < 0.1] = 0
    p = np.arange(P)
    tie, nan, ninf, tie_high = p % 11 == 3, p % 13 == 5, p % 13 == 6, p % 17 == 9
    z[:, :, tie] = 1.25                                             # every class equal: class 0
    if K > 2:
        z[:, 1:, tie_high] = 7.5                                    # classes 1.. equal above class 0: class 1
        z[:, 0, tie_high] = -2.0
    z[:, :, nan] = np.nan
    z[:, :, ninf] = -np.inf
    special = tie | nan | ninf | tie_high
    y[:, special] = (p[special] % K).astype(np.uint16)              # real labels under all of them
    if n > 1:
        y[1] = er.IGNORE                                            # a wholly ignored image
    z, y, w = z.reshape(n, K, H, W), y.reshape(n, H, W), w.reshape(n, H, W)
    for a in (z, y, w):
        a.setflags(write=False)
    return z, y, w


@functools.lru_cache(maxsize=None)
def expected(K, shape, n):
    return er.eval_ref(*case(K, shape, n))


def resident(a, offset=1, fill=0x5A):
    """`a` in HBM, `offset` elements into a buffer filled with garbage: (keep-alive, device pointer)"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    flat = flat.view(np.int16) if flat.dtype == np.uint16 else flat
    buf = torch.from_numpy(np.full((flat.size + offset + 8) * flat.itemsize, fill, np.uint8).view(flat.dtype)).cuda()
    buf[offset:offset + flat.size].copy_(torch.from_numpy(np.array(flat)))
    torch.cuda.current_stream().synchronize()        # torch's stream; the tally runs on the handle's
    return buf, buf.data_ptr() + offset * flat.itemsize


def run(net, z, y, w, gains=None, want_predicted=True, offset=1, prefill=0xA5):
    n, K, H, W = z.shape
    keep = [resident(z, offset), resident(y, offset), resident(w, offset) if w is not None else (None, 0)]
    pred = resident(np.full((n, H, W), 0x1234, np.uint16), offset) if want_predicted else (None, 0)
    r = aa.eval_logits_device(net, keep[0][1], keep[1][1], keep[2][1], n, K, H, W, gains=gains, d_predicted_ptr=pred[1], prefill=prefill)
    if want_predicted:
        r.predicted = pred[0][offset:offset + n * H * W].cpu().numpy().view(np.uint16).reshape(n, H, W)
        assert (pred[0][:offset].cpu().numpy().view(np.uint16) == 0x5A5A).all() and (pred[0][offset + n * H * W:].cpu().numpy().view(np.uint16) == 0x5A5A).all()
    return r


def assert_matches(r, want, pixels, what=""):
    for key in ("counted", "unclassified"):
        np.testing.assert_array_equal(r.per_image[key], want[key], err_msg=f"{key} {what}")
    np.testing.assert_array_equal(r.confusion, want["confusion"], err_msg=f"confusion {what}")
    if r.predicted is not None:
        np.testing.assert_array_equal(r.predicted, want["predicted"], err_msg=f"predicted {what}")
    assert (r.confusion.sum(axis=(1, 2)) + r.per_image["unclassified"] == r.per_image["counted"]).all(), what
    assert np.isfinite(r.per_image["loss_sum"]).all(), what
    for got, ref in zip(r.per_image["loss_sum"], want["loss_sum"]):
        print(f"loss per pixel {what}: got {got / pixels:.9g} want {ref / pixels:.9g}")
        assert abs(got / pixels - ref / pixels) <= 2e-5 * max(1.0, abs(ref / pixels)), what
    for got, ref in zip(r.per_image["weight_sum"], want["weight_sum"]):
        assert abs(got - ref) <= 1e-12 * abs(ref), what


def assert_same_bits(a, b, what=""):
    assert a.per_image.tobytes() == b.per_image.tobytes(), what
    np.testing.assert_array_equal(a.confusion, b.confusion, err_msg=what)
    if a.predicted is not None and b.predicted is not None:
        np.testing.assert_array_equal(a.predicted, b.predicted, err_msg=what)


@pytest.fixture(scope="module")
def net():
    return aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("K", CLASSES)
def test_tally_equals_the_reference(net, K, shape, n):
    z, y, w = case(K, shape, n)
    want = expected(K, shape, n)
    r = run(net, z, y, w)
    assert_matches(r, want, shape[0] * shape[1], f"K={K} {shape} n={n}")
    if n == 3:
        assert r.per_image[1].tobytes() == bytes(32) and not r.confusion[1].any()       # the wholly ignored image
        for i in range(n):   # every image alone, its maps lying elsewhere (another offset): the same bits, doubles included
            single = run(net, z[i:i + 1], y[i:i + 1], w[i:i + 1], offset=2, prefill=0x3C)
            assert single.per_image[0].tobytes() == r.per_image[i].tobytes(), i
            np.testing.assert_array_equal(single.confusion[0], r.confusion[i])
            np.testing.assert_array_equal(single.predicted[0], r.predicted[i])


@pytest.mark.parametrize("K,shape", [(3, (33, 258)), (9, (37, 41)), (64, (33, 258))])
def test_two_runs_over_dirtied_scratch_agree(net, K, shape):
    z, y, w = case(K, shape, 3)
    first = run(net, z, y, w)
    other = case(5, (37, 41), 3)
    run(net, *other, prefill=0xFF)                                   # other sums and counts go through the handle's scratch
    assert_same_bits(first, run(net, z, y, w, prefill=0x00), "second run")


@pytest.mark.parametrize("K,shape", [(3, (37, 41)), (8, (33, 258)), (9, (33, 258))])
def test_null_weights_are_ones_and_gains_move_only_the_prediction(net, K, shape):
    z, y, w = case(K, shape, 3)
    ones = np.ones_like(w)
    a, b = run(net, z, y, None), run(net, z, y, ones)
    assert_same_bits(a, b, "null weights")
    assert_matches(a, er.eval_ref(z, y, None), shape[0] * shape[1], "null weights")
    gains = np.zeros(K)
    gains[K - 1] = 100.0                                             # the last class wins wherever a class can win
    plain, gained = run(net, z, y, w), run(net, z, y, w, gains=gains)
    want = er.eval_ref(z, y, w, gains)
    assert_matches(gained, want, shape[0] * shape[1], "gains")
    voting = gained.predicted != er.IGNORE
    assert (gained.predicted[voting] == K - 1).all() and (plain.predicted != gained.predicted).any()
    assert plain.per_image["loss_sum"].tobytes() == gained.per_image["loss_sum"].tobytes()      # the loss has no gains
    no_map = run(net, z, y, w, want_predicted=False)                  # the predicted map is optional
    assert_same_bits(plain, no_map, "without a predicted map")


def test_a_label_beyond_the_classes_is_invalid_and_the_handle_works_afterwards(net):
    K, shape = 5, (37, 41)
    z, y, w = case(K, shape, 1)
    bad = np.array(y)
    bad[0, 20, 20] = K                                               # neither a class nor "ignore"
    with pytest.raises(aa.AnnonetHipError) as e:
        run(net, z, bad, w)
    assert e.value.code == INVALID and "class count" in str(e.value)
    assert_matches(run(net, z, y, w), expected(K, shape, 1), shape[0] * shape[1], "after the error")


def test_argument_checks(net):
    z, y, w = case(3, (3, 5), 1)
    d_z, d_y = resident(z), resident(y)
    out, conf = np.zeros(1, aa.EVAL_DTYPE), np.zeros((1, 3, 3), np.uint64)
    ptr = lambda a: a.ctypes.data
    L = net.L
    assert L.anh_eval_logits_device(net.h, d_z[1], d_y[1], None, 0, 3, 3, 5, None, ptr(out), ptr(conf), None) == INVALID      # n = 0
    assert L.anh_eval_logits_device(net.h, d_z[1], d_y[1], None, 1, 65, 3, 5, None, ptr(out), ptr(conf), None) == INVALID     # K beyond the net's limit
    assert L.anh_eval_logits_device(net.h, d_z[1], d_y[1], None, 1, 3, 0, 5, None, ptr(out), ptr(conf), None) == INVALID      # empty map
    assert L.anh_eval_logits_device(net.h, None, d_y[1], None, 1, 3, 3, 5, None, ptr(out), ptr(conf), None) == INVALID        # null logits
    assert L.anh_eval_logits_device(net.h, d_z[1], d_y[1], None, 1, 3, 3, 5, None, ptr(out), None, None) == 0                # the matrices are optional
    assert int(out["counted"][0]) == int(expected(3, (3, 5), 1)["counted"][0])
