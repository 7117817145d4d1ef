"""float64 statement of ONE layer of bf16 inference in its activation-storing form, applied to the input the kernel itself read, and the
per-element bars that follow from the arithmetic (tests/test_infer_layer_bars.py proves them on the CPU, tests/test_gpu_infer_layers.py
holds the kernels to them).

A reference restates the points where the kernels round an OPERAND to bf16, and nothing else (read from kernels_mfma.hip, head_blend_kernel
and conv_generic_kernel):
  * stem input: u8 / 256 through the clamp-to-edge window (exact in bf16); outside the window the conv pads with zeros;
  * one producer: the stored bf16 tensor, read as it is (SRC_RAW);
  * skip: the sum of the two stored bf16 tensors, rounded to bf16 again (SRC_SUM2, add_bf16x8);
  * filters: bf16(w) — the MFMA operand, and the fp32 compute copy that the head kernels multiply by (sgd_kernel);
  * bias, gamma, beta, running statistics: fp32, never rounded to bf16.
The folded bn constants and every sum are float64 here.  The kernel's fp32 arithmetic (the fold on the host, the accumulation, the
epilogue's multiply-add) is covered by E below, its one rounding of the result to bf16 by half a bf16 ulp.

Bars, with n = k*k*cin, s = gamma / sqrt(running_var + 1e-4), t = beta - running_mean * s, z = s * conv(x, wq) + t, ref = max(z, 0),
A = |s| * conv(|x|, |wq|) + |t| and E = (n + 4) * 2^-23 * A  (n fp32 additions under any faithful rounding; scale, shift and the
multiply-add of the epilogue):
  hidden layer      |got - ref| <= 2^-8 * max(|ref|, |got|) + E, and got == 0 exactly wherever z < -E
  head, stored act  |logit - (sum act*wq + bias)| <= (cin + 2) * 2^-23 * (sum |act*wq| + |bias|)
  head in epilogue  the activation is never stored: reference sum ref_c*wq_c + bias from the last hidden layer's input; the stored-head bar
                    on magnitudes (|ref_c| + b_c), plus sum |wq_c| * b_c, where b_c = 2^-8 * (|ref_c| + E_c) + E_c bounds the activation
                    (|v - z| <= E_c before the rounding, relu does not increase a difference, half an ulp of |v| <= |ref_c| + E_c)
  unbiased rounding over the elements with ref > 0, when there are at least 10^4: e = (got - ref) / ulp_bf16(ref) has |mean e| <= 0.02 and
                    mean |e| <= 0.27 (round to nearest: 0 +- 0.003 and 0.25; truncation: -0.5)
Nothing here calls the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

from train_ops_ref import bf16_from_f64, bf16_round, bf16_ulp

F32, F64 = np.float32, np.float64
BN_EPS = 1e-4
U23 = 2.0 ** -23
HALF_ULP = 2.0 ** -8
MIN_STAT = 10 ** 4
MEAN_E, MEAN_ABS_E = 0.02, 0.27


def kind(L):
    if not L.has_bn:
        return "head"
    if L.in_a < 0:
        return "stem"
    if L.type == 1:
        return "cont3x3s2"
    return "con3x3s2" if L.stride == 2 else "con3x3s1"


def filters(L, params):
    """bf16(w) as float64, in torch's layout: con [co][ci][kh][kw], cont [ci][co][kh][kw] (the canonical blob's)"""
    nw = L.k * L.k * L.cin * L.cout
    w = bf16_round(np.asarray(params[L.w_off:L.w_off + nw], F32)).astype(F64)
    return w.reshape((L.cout, L.cin, L.k, L.k) if L.type == 0 else (L.cin, L.cout, L.k, L.k))


def folded(L, params, running):
    g = np.asarray(params[L.g_off:L.g_off + L.cout], F64)
    b = np.asarray(params[L.beta_off:L.beta_off + L.cout], F64)
    rm = np.asarray(running[L.rs_off:L.rs_off + L.cout], F64)
    rv = np.asarray(running[L.rs_off + L.cout:L.rs_off + 2 * L.cout], F64)
    s = g / np.sqrt(rv + BN_EPS)
    return s, b - rm * s


def conv(L, x_nhwc, w):
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=F64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w, dtype=F64))
    y = F.conv2d(x, wt, stride=L.stride, padding=L.pad) if L.type == 0 else F.conv_transpose2d(x, wt, stride=L.stride, padding=L.pad)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def stem_input(images, samples, h, w):
    """x [n][h][w][c]: sample i = the h x w window of images[samples[i][0]] whose corner is (left, top) = samples[i][1:], clamped to the edge"""
    out = []
    for index, left, top in samples:
        img = np.asarray(images[index])
        img = img[:, :, None] if img.ndim == 2 else img
        ys = np.clip(top + np.arange(h), 0, img.shape[0] - 1)
        xs = np.clip(left + np.arange(w), 0, img.shape[1] - 1)
        out.append(img[ys][:, xs].astype(F64) / 256.0)
    return np.stack(out)


def skip_sum(a, b):
    return bf16_from_f64(np.asarray(a, F64) + np.asarray(b, F64))


def hidden(L, params, running, x):
    """the layer on its input x [n][h][w][cin] (float64): z, ref, A and E, all [n][h'][w'][cout]"""
    w = filters(L, params)
    s, t = folded(L, params, running)
    z = s * conv(L, x, w) + t
    A = np.abs(s) * conv(L, np.abs(x), np.abs(w)) + np.abs(t)
    n = L.k * L.k * L.cin
    return dict(z=z, ref=np.maximum(z, 0.0), A=A, E=(n + 4) * U23 * A, n=n)


def check_hidden(tag, got, h):
    """every bar of a hidden layer on its stored output `got`; -> (worst error / bound, mean e, mean |e|, elements with ref > 0)"""
    got = np.asarray(got, F64)
    ref, E = h["ref"], h["E"]
    assert got.shape == ref.shape, f"{tag}: stored tensor {got.shape}, reference {ref.shape}"
    err = np.abs(got - ref)
    bound = HALF_ULP * np.maximum(np.abs(ref), np.abs(got)) + E
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[at])
    where = f"{tag}: worst error / bound = {worst:.4g} at {tuple(int(i) for i in at)} (got {got[at]!r}, reference {ref[at]!r})"
    assert np.isfinite(got).all(), where
    must_be_zero = h["z"] < -E
    assert (got[must_be_zero] == 0).all(), f"{int((got[must_be_zero] != 0).sum())} elements are not 0 where z < -E; {where}"
    assert worst <= 1.0, f"{int((ratio > 1).sum())} of {ratio.size} elements beyond the bound; {where}"
    pos = ref > 0
    count = int(pos.sum())
    mean_e = mean_abs = float("nan")
    if count >= MIN_STAT:
        e = (got[pos] - ref[pos]) / bf16_ulp(ref[pos])
        mean_e, mean_abs = float(e.mean()), float(np.abs(e).mean())
        assert abs(mean_e) <= MEAN_E, f"rounding is biased: mean e = {mean_e:.4f} over {count} elements; {where}"
        assert mean_abs <= MEAN_ABS_E, f"rounding is not to nearest: mean |e| = {mean_abs:.4f} over {count} elements; {where}"
    return worst, mean_e, mean_abs, count


def head_weights(L, params):
    w = filters(L, params).reshape(L.cout, L.cin)
    return w, np.asarray(params[L.b_off:L.b_off + L.cout], F64)


def head_stored(L, params, act):
    """the 1x1 head on a stored activation [n][h][w][cin]: (reference, bound) [n][h][w][K]"""
    w, bias = head_weights(L, params)
    act = np.asarray(act, F64)
    mag = np.abs(act) @ np.abs(w).T + np.abs(bias)
    return act @ w.T + bias, (L.cin + 2) * U23 * mag


def head_epilogue(L, params, h):
    """the head in the last hidden layer's epilogue, from that layer's reference h = hidden(...): (reference, bound) [n][h][w][K]"""
    w, bias = head_weights(L, params)
    b_c = HALF_ULP * (h["ref"] + h["E"]) + h["E"]
    mag = (h["ref"] + b_c) @ np.abs(w).T + np.abs(bias)
    return h["ref"] @ w.T + bias, b_c @ np.abs(w).T + (L.cin + 2) * U23 * mag


def check_head(tag, got, ref, bound):
    got = np.asarray(got, F64)
    assert got.shape == ref.shape, f"{tag}: logits {got.shape}, reference {ref.shape}"
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[at])
    where = f"{tag}: worst error / bound = {worst:.4g} at {tuple(int(i) for i in at)} (got {got[at]!r}, reference {ref[at]!r})"
    assert np.isfinite(got).all(), where
    assert worst <= 1.0, f"{int((ratio > 1).sum())} of {ratio.size} logits beyond the bound; {where}"
    return worst


def check_layers(layers, params, running, stem_x, tensors, logits=None, epilogue_logits=None, name=""):
    """Every stored layer of one pass against its own stored input.  tensors[li]: the stored tensor of bn layer li, or None where the pass
    did not store it; logits / epilogue_logits [n][h][w][K]: the head's output where it ran on the stored activation / in the last hidden
    layer's epilogue.  -> {"<li> <kind>": worst error / bound}; prints one line per layer."""
    report = {}
    head = layers[-1]
    for li, L in enumerate(layers[:-1]):
        if tensors[li] is None and not (epilogue_logits is not None and li == head.in_a):
            continue
        if L.in_a < 0:
            x = np.asarray(stem_x, F64)
        else:
            assert tensors[L.in_a] is not None and (L.in_b < 0 or tensors[L.in_b] is not None), f"layer {li}: its input was not stored"
            x = np.asarray(tensors[L.in_a], F64) if L.in_b < 0 else skip_sum(tensors[L.in_a], tensors[L.in_b])
        h = hidden(L, params, running, x)
        tag = f"{name} layer {li} ({kind(L)}, {L.cin} -> {L.cout}{', skip' if L.in_b >= 0 else ''})"
        if tensors[li] is not None:
            worst, mean_e, mean_abs, count = check_hidden(tag, tensors[li], h)
            report[f"{li} {kind(L)}"] = worst
            stats = f"mean e {mean_e:+.4f}, mean |e| {mean_abs:.4f} over" if count >= MIN_STAT else "rounding statistics not asserted:"
            print(f"{tag}: worst error / bound {worst:.3f}; {stats} {count} elements with ref > 0")
        if epilogue_logits is not None and li == head.in_a:
            tag = f"{name} layer {len(layers) - 1} (head in the epilogue of layer {li}, {head.cin} -> {head.cout})"
            worst = check_head(tag, epilogue_logits, *head_epilogue(head, params, h))
            report[f"{len(layers) - 1} head in epilogue"] = worst
            print(f"{tag}: worst error / bound {worst:.3f}")
    if logits is not None:
        tag = f"{name} layer {len(layers) - 1} (head on the stored activation, {head.cin} -> {head.cout})"
        assert tensors[head.in_a] is not None, f"{tag}: its input was not stored"
        worst = check_head(tag, logits, *head_stored(head, params, tensors[head.in_a]))
        report[f"{len(layers) - 1} head"] = worst
        print(f"{tag}: worst error / bound {worst:.3f}")
    return report
