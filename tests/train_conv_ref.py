"""float64 statement of ONE bf16 training convolution (forward, backward-data, filter gradient) on given inputs, and the bars that follow
from the arithmetic (tests/test_train_conv_bars.py proves them on the CPU, tests/test_gpu_train_conv.py and tests/helpers/run_ops_regime.py
hold the kernels to them).

A reference restates the points where the kernels round an OPERAND or a RESULT, and nothing else (read from kernels_mfma.hip: side_convert,
affine_relu_pack8, affine8, add_bf16x8, store_pixel_tiles, wgrad_stem_mfma_kernel; the generic kernels round the same values):
  * staged operand    raw (SRC_RAW): the stored bf16 tensor as it is; one producer (SRC_ACT): bf16(relu(fmaf(x, s, t))); skip (SRC_ACT2): each
                      side's relu(fmaf) in an fp32 register, one fp32 add, then bf16 — train_ops_ref.head_input(sides, bf16=True).  Padding is
                      zero AFTER the prologue (relu(shift) is not zero: NEED_MASK, P_MASK, T_MASK);
  * stem              u8 / 256, exact in bf16;
  * filters           bf16(w);  dy: the stored bf16 tensor;
  * dy formed in the stem's filter gradient (WgradArgs::dy_y): bf16(k0 * (dz - k1 - xhat * k2)), train_ops_ref.bn_bwd_apply;
  * results           forward and backward-data store bf16 (fp32 under a bias: the 1x1 head's logits), the filter gradient fp32.
Every sum is float64: forward and backward-data through torch's double conv2d / conv_transpose2d (backward-data of a con layer is the
transposed conv with the same filters, and the reverse for cont), the filter gradient as one einsum per tap,
dw[t][ci][co] = sum x(n, iy, ix, ci) * dy(n, oy, ox, co) with the gather convention of kernels.h.

Bars, with n the number of contributing (tap, channel) terms of an element, A the same sum over magnitudes and U = 2^-23 (one fp32 spacing:
every addition may be faithful rather than to nearest):
  stored bf16       |got - ref| <= 2^-8 * max(|ref|, |got|) + E,  E = (n + 2) * U * A          (stored fp32: 2^-24 in the place of 2^-8)
  rounding          over the elements with |ref| >= median |ref|, when there are at least 5000: e = (got - ref) / ulp_bf16(ref) has
                    |mean e| <= 0.02 and mean |e| <= 0.27 (to nearest: 0 and 0.25; truncation: -+0.5 and 0.5).  The selection is by magnitude
                    because training stores signed raw outputs, and near zero E is not small against an ulp.  Signed outputs also hide a
                    bias toward zero from mean e (truncation: -0.5 on the positive half, +0.5 on the negative), so mean e * sign(ref) is
                    held to the same 0.02.
  accumulated       backward-data into a tensor that holds a gradient already: bf16(old + q) bit for bit, q = what the same call stores
                    without the old tensor (q itself is held to the element bar)
  filter gradient   |got - ref| <= (P + 512) * U * A, P = batch * h_out * w_out pixels; 512 covers the partial-sum pass (at most 256
                    splits, or 512 stem workgroups).  A worst-case bar, but per element.
  ... its accuracy  rms of (got - ref) / A over a fixed subset of elements <= 2 x the same rms of seq_filter_grad: one fp32 accumulator per
                    element, terms added in (n, y, x) order — the longest chain a correct fp32 kernel could run.  The factor 2 allows the
                    matrix core's internal additions to be faithful and not to nearest.
  dy in the kernel  the two filter-gradient bars on the float64-rounded dy, plus the allowance sum |x| * ulp_bf16(dy) over the pixels whose
                    float64 dy lies within bn_bwd_apply's fp32 bound of a bf16 rounding boundary (the kernel's value may round to the other
                    side there).  The rms bar subtracts the allowance from the error first.
A check collects EVERY bar it finds broken and raises one AssertionError that names them ("broken bars: [...]"), so that a test can say which.
Nothing here calls the library.
"""
import numpy as np
import torch
import torch.nn.functional as F

from train_ops_ref import bf16_from_f64, bf16_round, bf16_ulp, bn_bwd_apply, head_input

F32, F64 = np.float32, np.float64
U23 = 2.0 ** -23
HALF_ULP = 2.0 ** -8
MIN_STAT = 5000
MEAN_E, MEAN_ABS_E = 0.02, 0.27
RMS_FACTOR = 2.0
SUBSET = 2048

#           type k  s  p  cin cout   n  h   w        tests/test_gpu_ops.py's SHAPES, the 64 -> 128 stride-2 plane grown to 10^4 outputs
SHAPES = [
    ((0, 5, 1, 2, 3, 32), 2, 19, 23),     # stem
    ((0, 3, 1, 1, 32, 32), 2, 21, 37),
    ((0, 3, 1, 1, 64, 64), 1, 18, 33),
    ((0, 3, 1, 1, 128, 128), 1, 9, 35),
    ((0, 3, 2, 0, 32, 64), 2, 23, 31),
    ((0, 3, 2, 0, 64, 128), 1, 17, 23),
    ((1, 3, 2, 0, 128, 64), 1, 7, 9),
    ((1, 3, 2, 0, 64, 32), 2, 11, 15),
    ((0, 3, 1, 1, 256, 256), 1, 9, 19),
    ((0, 3, 2, 0, 128, 256), 1, 13, 17),
    ((1, 3, 2, 0, 256, 128), 1, 5, 7),
    ((0, 1, 1, 0, 32, 3), 2, 17, 13),
    ((0, 3, 1, 1, 8, 16), 1, 12, 10),
    ((0, 3, 1, 1, 40, 24), 1, 10, 13),
    ((0, 1, 1, 0, 32, 5), 2, 17, 13),
    ((0, 1, 1, 0, 32, 9), 2, 17, 13),
    ((0, 1, 1, 0, 32, 33), 1, 11, 14),
    ((0, 1, 1, 0, 32, 64), 1, 11, 14),
    ((0, 1, 1, 0, 8, 9), 1, 12, 10),
]


def out_dim(desc, n):
    type_, k, stride, pad = desc[:4]
    return (n + 2 * pad - k) // stride + 1 if type_ == 0 else stride * (n - 1) + k - 2 * pad


def is_stem(desc):
    return desc[1] == 5


def make_inputs(desc, n, h, w, seed, prologue):
    """the inputs of tests/test_gpu_ops.py, every tensor already a bf16 value; the stem's x is an image / 256 -> (xa, kw, filters, rng)"""
    rng = np.random.default_rng(seed)
    cin, cout, k = desc[4], desc[5], desc[1]
    if is_stem(desc):
        xa = (rng.integers(0, 256, (n, h, w, cin)).astype(F32) / F32(256))
    else:
        xa = bf16_round(rng.normal(0, 1, (n, h, w, cin)).astype(F32))
    kw = {}
    if prologue >= 1:
        kw.update(sa=rng.uniform(0.5, 1.5, cin).astype(F32), ta=rng.uniform(-0.3, 0.3, cin).astype(F32))
    if prologue == 2:
        kw.update(xb=bf16_round(rng.normal(0, 1, (n, h, w, cin)).astype(F32)),
                  sb=rng.uniform(0.5, 1.5, cin).astype(F32), tb=rng.uniform(-0.3, 0.3, cin).astype(F32))
    lim = np.sqrt(6.0 / (k * k * (cin + cout)))
    filters = rng.uniform(-lim, lim, k * k * cin * cout).astype(F32)
    return xa, kw, filters, rng


def make_dy(desc, n, h, w, rng, sigma=1.0):
    return bf16_round(rng.normal(0, sigma, (n, out_dim(desc, h), out_dim(desc, w), desc[5])).astype(F32))


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def staged(xa, sa=None, ta=None, xb=None, sb=None, tb=None):
    """the operand a conv or a filter gradient stages (float64), from the stored tensors and their producers' (scale, shift)"""
    if sa is None:
        return np.asarray(xa, F64)
    sides = [(xa, sa, ta)] + ([(xb, sb, tb)] if xb is not None else [])
    return head_input(sides, bf16=True)[0]


def filters_q(desc, filters):
    """bf16(w) as float64 in torch's layout, which is the canonical blob's: con [co][ci][kh][kw], cont [ci][co][kh][kw]"""
    type_, k, _, _, cin, cout = desc
    w = bf16_round(np.asarray(filters, F32)).astype(F64)
    return w.reshape((cout, cin, k, k) if type_ == 0 else (cin, cout, k, k))


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_forward(desc, x, w):
    """the layer's forward on x [n][h][w][cin], w in torch's layout; dtype of the operands (float64 here, float32 in the emulations)"""
    type_, _, s, p = desc[:4]
    wt = torch.from_numpy(np.ascontiguousarray(w))
    return _nhwc(F.conv2d(_nchw(x), wt, stride=s, padding=p) if type_ == 0 else F.conv_transpose2d(_nchw(x), wt, stride=s, padding=p))


def conv_backward(desc, dy, w, in_hw):
    """the layer's backward-data on dy [n][ho][wo][cout]: the adjoint of conv_forward, [n][h][w][cin]"""
    type_, k, s, p = desc[:4]
    wt = torch.from_numpy(np.ascontiguousarray(w))
    if type_ == 1:
        return _nhwc(F.conv2d(_nchw(dy), wt, stride=s, padding=p))
    extra = tuple(in_hw[i] - ((dy.shape[1 + i] - 1) * s + k - 2 * p) for i in range(2))   # rows / columns the strided conv never read
    return _nhwc(F.conv_transpose2d(_nchw(dy), wt, stride=s, padding=p, output_padding=extra))


def _terms(op, desc, shape_in, c_red, *extra):
    """contributing (tap, channel) terms per output element: the op on ones, one channel, times c_red"""
    k = desc[1]
    ones = np.ones(shape_in[:3] + (1,), F64)
    return c_red * op(desc, ones, np.ones((1, 1, k, k), F64), *extra)


def forward(desc, x, filters, bias=None):
    """reference of the forward conv on the staged operand x: ref, A, n, E [n][ho][wo][cout]"""
    w = filters_q(desc, filters)
    ref, A = conv_forward(desc, x, w), conv_forward(desc, np.abs(x), np.abs(w))
    if bias is not None:
        ref, A = ref + np.asarray(bias, F64), A + np.abs(np.asarray(bias, F64))
    n = _terms(conv_forward, desc, x.shape, desc[4])
    return dict(ref=ref, A=A, n=n, E=(n + 2) * U23 * A)


def backward_data(desc, dy, filters, in_hw):
    w = filters_q(desc, filters)
    dy = np.asarray(dy, F64)
    ref, A = conv_backward(desc, dy, w, in_hw), conv_backward(desc, np.abs(dy), np.abs(w), in_hw)
    n = _terms(conv_backward, desc, dy.shape, desc[5], in_hw)
    return dict(ref=ref, A=A, n=n, E=(n + 2) * U23 * A)


# ---- the filter gradient -----------------------------------------------------------------------------------------------------------------
def tap_views(desc, x, dy):
    """per tap t = ky * k + kx the aligned pair (xs, dys) [n][hs][ws][c] with dw[t] = sum over (n, y, x) of xs (x) dys: the plane walked is the
    smaller one (dy for con, x for cont), the other is read at small * stride + tap - pad, zero outside (kernels.h)"""
    type_, k, s, p = desc[:4]
    small, big = (dy, x) if type_ == 0 else (x, dy)
    hs, ws = small.shape[1:3]
    bp = np.pad(big, ((0, 0), (p, p), (p, p), (0, 0)))
    for ky in range(k):
        for kx in range(k):
            v = bp[:, ky:ky + s * (hs - 1) + 1:s, kx:kx + s * (ws - 1) + 1:s]
            yield (v, small) if type_ == 0 else (small, v)


def to_canonical(desc, tm):
    """[t][ci][co] -> the flat canonical layout the op entry points return"""
    return np.ascontiguousarray(tm.transpose(2, 1, 0) if desc[0] == 0 else tm.transpose(1, 2, 0)).reshape(-1)


def to_tm(desc, flat):
    type_, k, _, _, cin, cout = desc
    a = np.asarray(flat)
    return a.reshape(cout, cin, k * k).transpose(2, 1, 0) if type_ == 0 else a.reshape(cin, cout, k * k).transpose(2, 0, 1)


def tap_sums(desc, x, dy):
    return np.stack([np.einsum("pi,po->io", xs.reshape(-1, xs.shape[3]), ds.reshape(-1, ds.shape[3]), optimize=True) for xs, ds in tap_views(desc, x, dy)])


def filter_grad(desc, x, dy, allowance=None):
    """reference of the filter gradient on the staged operand x and the stored dy: ref, A, bound [t][ci][co] (allowance: the same shape)"""
    x, dy = np.asarray(x, F64), np.asarray(dy, F64)
    ref, A = tap_sums(desc, x, dy), tap_sums(desc, np.abs(x), np.abs(dy))
    P = dy.shape[0] * dy.shape[1] * dy.shape[2]
    allow = np.zeros_like(A) if allowance is None else allowance
    return dict(ref=ref, A=A, P=P, allow=allow, bound=(P + 512) * U23 * A + allow)


def stem_dy(da, y, mean, invstd, scale, shift, coef):
    """dy as the stem's filter gradient forms it from (da, y) [n][h][w][c] and coef [3][c]: (bf16 of the float64 value; near * ulp, the
    magnitude by which the kernel's fp32 value may land on the other side of a rounding boundary)"""
    dy64, b = bn_bwd_apply(da, y, mean, invstd, scale, shift, np.asarray(coef, F32).reshape(3, -1))
    dyq = bf16_from_f64(dy64)
    ulp = bf16_ulp(dy64)
    near = ulp / 2 - np.abs(dy64 - dyq) <= b
    return dyq, np.where(near, ulp, 0.0)


def subset_channels(desc):
    """input channels whose every tap and output channel make the accuracy subset: the first m, at least SUBSET elements"""
    _, k, _, _, cin, cout = desc
    return min(cin, -(-SUBSET // (k * k * cout)))


def seq_filter_grad(desc, x, dy, m=None):
    """sequential fp32 emulation on the subset [t][:m][co]: one fp32 accumulator per element, terms added in (n, y, x) order.  The operands
    are bf16 values, so every product is exact in fp32 and each step rounds once."""
    m = subset_channels(desc) if m is None else m
    views = [(np.ascontiguousarray(xs[..., :m], F32).reshape(-1, m), np.ascontiguousarray(ds, F32).reshape(-1, ds.shape[3])) for xs, ds in tap_views(desc, x, dy)]
    X = np.stack([v[0] for v in views], 1)   # [P][t][m]
    D = np.stack([v[1] for v in views], 1)   # [P][t][co]
    acc = np.zeros((X.shape[1], m, D.shape[2]), F32)
    tmp = np.empty_like(acc)
    for p in range(X.shape[0]):
        np.multiply(X[p][:, :, None], D[p][:, None, :], out=tmp)
        np.add(acc, tmp, out=acc)
    return acc


def rel_rms(got, ref, A, allow=None):
    err = np.abs(np.asarray(got, F64) - ref)
    if allow is not None:
        err = np.maximum(err - allow, 0.0)
    ok = A > 0
    return float(np.sqrt(np.mean((err[ok] / A[ok]) ** 2))) if ok.any() else 0.0


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def _worst(got, ref, bound):
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return ratio, at, float(ratio[at])


def _raise(tag, broken, where):
    if broken:
        raise AssertionError(f"{tag}: broken bars: {[b[0] for b in broken]}; " + "; ".join(b[1] for b in broken) + f"; {where}")


def check_stored(tag, got, r, stored_bf16=True):
    """the element bar and the rounding statistics of a stored forward / backward-data result -> (worst error / bound, mean e, mean |e|,
    elements in the statistics: 0 where they are not claimed)"""
    got = np.asarray(got, F64)
    ref, E = r["ref"], r["E"]
    assert got.shape == ref.shape, f"{tag}: stored tensor {got.shape}, reference {ref.shape}"
    bound = (HALF_ULP if stored_bf16 else 2.0 ** -24) * np.maximum(np.abs(ref), np.abs(got)) + E
    ratio, at, worst = _worst(got, ref, bound)
    where = f"worst error / bound = {worst:.4g} at {tuple(int(i) for i in at)} (got {got[at]!r}, reference {ref[at]!r}, bound {bound[at]!r})"
    broken = []
    if not np.isfinite(got).all():
        broken.append(("finite", f"{int((~np.isfinite(got)).sum())} elements are not finite"))
    if not worst <= 1.0:
        broken.append(("element", f"{int((ratio > 1).sum())} of {ratio.size} elements beyond the bound"))
    mean_e = mean_abs = float("nan")
    count = 0
    if stored_bf16:
        big = np.abs(ref) >= np.median(np.abs(ref))
        big &= ref != 0
        if int(big.sum()) >= MIN_STAT:
            count = int(big.sum())
            e = (got[big] - ref[big]) / bf16_ulp(ref[big])
            mean_e, mean_abs = float(e.mean()), float(np.abs(e).mean())
            toward = float((e * np.sign(ref[big])).mean())      # signed outputs: a store biased toward zero (truncation) has mean e = 0
            if not (abs(mean_e) <= MEAN_E and abs(toward) <= MEAN_E):
                broken.append(("rounding bias", f"mean e = {mean_e:+.4f}, mean e * sign(ref) = {toward:+.4f} over {count} elements"))
            if not mean_abs <= MEAN_ABS_E:
                broken.append(("rounding spread", f"mean |e| = {mean_abs:.4f} over {count} elements"))
    _raise(tag, broken, where)
    return worst, mean_e, mean_abs, count


def check_accumulated(tag, got, old, q):
    """backward-data into a tensor that held `old`: bf16(old + q) bit for bit (q: the same call's stored result without it)"""
    want = bf16_round((np.asarray(old, F32).astype(F64) + np.asarray(q, F32).astype(F64)).astype(F32))   # two bf16 values: the fp32 sum is one rounding of the exact one
    got = np.asarray(got, F32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    bad &= ~((got == 0) & (want == 0))
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        _raise(tag, [("accumulate", f"{int(bad.sum())} of {bad.size} elements are not bf16(old + q)")], f"first at {at}: got {got[at]!r}, want {want[at]!r}, old {np.asarray(old)[at]!r}, q {np.asarray(q)[at]!r}")


def check_filter_grad(tag, desc, got_flat, r, seq=None):
    """the element bar on every element and, with seq = seq_filter_grad(...), the accuracy bar on the subset -> (worst error / bound, rms ratio)"""
    got = np.asarray(to_tm(desc, got_flat), F64)
    ref, A, bound = r["ref"], r["A"], r["bound"]
    assert got.shape == ref.shape, f"{tag}: gradient {got.shape}, reference {ref.shape}"
    ratio, at, worst = _worst(got, ref, bound)
    where = f"worst error / bound = {worst:.4g} at (tap, ci, co) = {tuple(int(i) for i in at)} (got {got[at]!r}, reference {ref[at]!r}, bound {bound[at]!r})"
    broken = []
    if not np.isfinite(got).all():
        broken.append(("finite", f"{int((~np.isfinite(got)).sum())} elements are not finite"))
    if not worst <= 1.0:
        broken.append(("filter element", f"{int((ratio > 1).sum())} of {ratio.size} elements beyond the bound"))
    rms_ratio = float("nan")
    if seq is not None:
        m = seq.shape[1]
        assert seq.shape[0] * m * seq.shape[2] >= min(SUBSET, ref.size), f"{tag}: the accuracy subset has only {seq.size} elements"
        sub = (slice(None), slice(0, m))
        rms_seq = rel_rms(seq, ref[sub], A[sub])
        rms_got = rel_rms(got[sub], ref[sub], A[sub], r["allow"][sub])
        rms_ratio = rms_got / rms_seq if rms_seq > 0 else (0.0 if rms_got == 0 else float("inf"))
        if not rms_ratio <= RMS_FACTOR:
            broken.append(("filter rms", f"rms of error / A = {rms_got:.3g}, {rms_ratio:.3g} x the sequential fp32 emulation's {rms_seq:.3g}"))
    _raise(tag, broken, where)
    return worst, rms_ratio


def report(tag, worst, mean_e=float("nan"), mean_abs=float("nan"), count=0, rms_ratio=float("nan")):
    """one line per case: worst error / bound, mean e, mean |e|, rms ratio"""
    stats = f"mean e {mean_e:+.4f}, mean |e| {mean_abs:.4f} over {count} elements" if count else "rounding statistics not claimed"
    rms = "" if np.isnan(rms_ratio) else f"; rms ratio {rms_ratio:.3f}"
    print(f"{tag}: worst error / bound {worst:.4f}; {stats}{rms}", flush=True)
