"""tests/eval_ref.py against literal per-pixel loops on tiny cases: the argmax rule (first strictly largest from -inf, NaN never wins,
gains added in double and rounded to float), ignore labels, unclassified pixels, the weighted log-loss term, and the invariant
sum(confusion) + unclassified == counted."""
import math

import numpy as np
import pytest

import eval_ref as er


def loops(z, y, w, gains):
    n, K, H, W = z.shape
    loss, weight = np.zeros(n), np.zeros(n)
    counted, unclassified = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    confusion = np.zeros((n, K, K), np.uint64)
    predicted = np.zeros((n, H, W), np.uint16)
    for i in range(n):
        for r in range(H):
            for c in range(W):
                label, best = er.IGNORE, -math.inf
                for k in range(K):
                    value = float(np.float32(float(z[i, k, r, c]) + (0.0 if gains is None else float(gains[k]))))
                    if value > best:
                        label, best = k, value
                predicted[i, r, c] = label
                t = int(y[i, r, c])
                if t == er.IGNORE:
                    continue
                counted[i] += 1
                if label == er.IGNORE:
                    unclassified[i] += 1
                    continue
                confusion[i, t, label] += 1
                zs = [float(v) for v in z[i, :, r, c]]
                m = max(zs)
                p = math.exp(zs[t] - m) / sum(math.exp(v - m) for v in zs)
                loss[i] += float(w[i, r, c]) * -math.log(max(p, 1e-10))
                weight[i] += float(w[i, r, c])
    return dict(loss_sum=loss, weight_sum=weight, counted=counted, unclassified=unclassified, confusion=confusion, predicted=predicted)


def case(seed, n, K, H, W):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-8, 8, (n, K, H, W)).astype(np.float32)
    y = rng.integers(0, K, (n, H, W)).astype(np.uint16)
    y[rng.random((n, H, W)) < 0.2] = er.IGNORE
    w = rng.uniform(0.5, 2.0, (n, H, W)).astype(np.float32)
    flat = z.reshape(n, K, -1)
    if H * W >= 6:
        flat[:, :, 1] = 0.75                      # an exact tie: the first class wins
        flat[:, :, 2] = np.nan                    # no class exceeds -inf
        flat[:, :, 3] = -np.inf
        y.reshape(n, -1)[:, 1:4] = np.arange(3) % K
        if K > 2:
            flat[:, 1:, 4] = 3.5                  # a tie that does not include class 0
            flat[:, 0, 4] = -1.0
    return z, y, w


@pytest.mark.parametrize("gains", [False, True])
@pytest.mark.parametrize("n,K,H,W", [(1, 1, 1, 1), (1, 3, 2, 3), (2, 4, 3, 5), (1, 9, 1, 7)])
def test_eval_ref_equals_the_loops(n, K, H, W, gains):
    z, y, w = case(n * 100 + K, n, K, H, W)
    g = np.linspace(-20.0, 20.0, K) if gains else None
    got, want = er.eval_ref(z, y, w, g), loops(z, y, w, g)
    for key in ("counted", "unclassified", "confusion", "predicted"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    np.testing.assert_allclose(got["loss_sum"], want["loss_sum"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["weight_sum"], want["weight_sum"], rtol=1e-14, atol=0)
    assert (got["confusion"].sum(axis=(1, 2)) + got["unclassified"] == got["counted"]).all()
    assert np.isfinite(got["loss_sum"]).all()


def test_gains_move_the_prediction_and_not_the_loss():
    z, y, w = case(5, 1, 3, 3, 4)
    plain, gained = er.eval_ref(z, y, w), er.eval_ref(z, y, w, [0.0, 0.0, 100.0])
    voting = gained["predicted"] != er.IGNORE
    assert (gained["predicted"][voting] == 2).all() and (plain["predicted"] != gained["predicted"]).any()
    np.testing.assert_array_equal(plain["loss_sum"], gained["loss_sum"])


def test_null_weights_are_ones_and_an_ignored_image_is_all_zero():
    z, y, w = case(6, 2, 3, 3, 4)
    y[1] = er.IGNORE
    a, b = er.eval_ref(z, y, None), er.eval_ref(z, y, np.ones_like(w))
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["counted"][1] == 0 and a["unclassified"][1] == 0 and a["loss_sum"][1] == 0 and a["weight_sum"][1] == 0 and not a["confusion"][1].any()


def test_a_label_beyond_the_classes_is_an_error():
    z, y, w = case(7, 1, 3, 2, 3)
    y[0, 0, 0] = 3
    with pytest.raises(ValueError):
        er.eval_ref(z, y, w)


def test_the_figures_of_a_known_matrix():
    r = dict(loss_sum=np.array([2.0, 4.0]), weight_sum=np.array([1.0, 2.0]), counted=np.array([6, 4], np.uint64),
             confusion=np.array([[[3, 1], [0, 2]], [[1, 0], [2, 1]]], np.uint64))
    assert er.mean_loss(r) == 2.0
    assert er.pixel_accuracy(r) == 7 / 10
    np.testing.assert_allclose(er.class_iou(r), [4 / 7, 3 / 6])
