"""Held-out evaluation restated in float64 numpy (include/annonet_hip.h, "held-out evaluation"): per window the loss sums, the counts, the
confusion matrix and the predicted map, from fp32 logits [n,K,H,W], u16 labels [n,H,W] and fp32 weights [n,H,W].

The argmax is taken on the fp32 values as given — (float)((double)z + gain), the first strictly largest from -inf, NaN never wins — so
counts and maps are exact; the loss term w * (-log max(softmax(z)[truth], 1e-10)) is computed in float64 throughout."""
import numpy as np

IGNORE = 65535


def predicted_map(logits, gains=None):
    z = np.asarray(logits, np.float32)
    K = z.shape[1]
    g = np.zeros(K) if gains is None else np.asarray(gains, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        value = (z.astype(np.float64) + g[None, :, None, None]).astype(np.float32)
    value = np.where(np.isnan(value), -np.inf, value)          # a NaN is never "> best"
    first = value.argmax(axis=1)                               # the first of equal maxima
    return np.where(value.max(axis=1) > -np.inf, first, IGNORE).astype(np.uint16)


def eval_ref(logits, labels, weights=None, gains=None):
    """-> dict(loss_sum, weight_sum f64 [n]; counted, unclassified u64 [n]; confusion u64 [n,K,K]; predicted u16 [n,H,W]); raises
    ValueError for a label >= K that is not IGNORE"""
    z = np.asarray(logits, np.float32)
    y = np.asarray(labels, np.uint16)
    n, K, H, W = z.shape
    w = np.ones((n, H, W), np.float32) if weights is None else np.asarray(weights, np.float32)
    if ((y != IGNORE) & (y >= K)).any():
        raise ValueError("a label value exceeds the class count")
    predicted = predicted_map(z, gains)
    out = dict(loss_sum=np.zeros(n), weight_sum=np.zeros(n), counted=np.zeros(n, np.uint64), unclassified=np.zeros(n, np.uint64),
               confusion=np.zeros((n, K, K), np.uint64), predicted=predicted)
    for i in range(n):
        labelled = y[i] != IGNORE
        voting = labelled & (predicted[i] != IGNORE)
        out["counted"][i] = labelled.sum()
        out["unclassified"][i] = (labelled & ~voting).sum()
        t, p = y[i][voting].astype(np.int64), predicted[i][voting].astype(np.int64)
        np.add.at(out["confusion"][i], (t, p), 1)
        zi = z[i][:, voting].astype(np.float64)                # [K, pixels]
        if zi.shape[1]:
            e = np.exp(zi - zi.max(axis=0))
            prob = e[t, np.arange(t.size)] / e.sum(axis=0)
            wi = w[i][voting].astype(np.float64)
            out["loss_sum"][i] = (wi * -np.log(np.maximum(prob, 1e-10))).sum()
            out["weight_sum"][i] = wi.sum()
    return out


def mean_loss(r):
    return r["loss_sum"].sum() / r["weight_sum"].sum()


def pixel_accuracy(r):
    return float(np.trace(r["confusion"].sum(axis=0))) / float(r["counted"].sum())


def class_iou(r):
    m = r["confusion"].sum(axis=0).astype(np.float64)
    hits = np.diag(m)
    union = m.sum(axis=1) + m.sum(axis=0) - hits
    return np.where(union > 0, hits / np.where(union > 0, union, 1.0), np.nan)
