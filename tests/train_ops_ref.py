"""float64 numpy references of the training kernels that are not convolutions (tests/test_gpu_train_ops.py).

A reference restates a kernel's STORAGE roundings and its sign decision, and nothing else of its arithmetic:
  * bf16 (round to nearest even) where the kernel stores bf16 or passes a value through operand_round — straight from the float64
    value for results, from the fp32 register value for the head's staged operand (head_input);
  * fp32 where the kernel keeps an fp32 array (mean, invstd, scale, shift, coef, dgamma, dbeta, running statistics, sw = scale * weight);
  * the relu mask is the sign of y * scale + shift evaluated in float64 (the kernels' fmaf rounds once, so it has the sign of the exact value).
Every sum is accumulated in float64.  Nothing here calls the library.
"""
import numpy as np

LABEL_IGNORE = 65535
F32, F64 = np.float32, np.float64


def bf16_round(a):
    """float32 values rounded to bf16 (nearest even), as float32"""
    a = np.ascontiguousarray(a, dtype=F32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(a.shape)


def bf16_from_f64(a):
    """float64 values rounded ONCE to bf16's 8 significant bits (nearest even), as float64 (normal range)"""
    a = np.asarray(a, dtype=F64)
    m, e = np.frexp(a)
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


def bf16_ulp(a):
    """spacing of bf16 at |a| (float64)"""
    a = np.abs(np.asarray(a, dtype=F64))
    _, e = np.frexp(np.where(a > 0, a, 1.0))
    return np.where(a > 0, np.ldexp(1.0, e - 8), 0.0)


def store(a, bf16):
    """a float64 value as the kernel stores it: bf16, or fp32"""
    return bf16_from_f64(a) if bf16 else np.asarray(a, dtype=F64).astype(F32).astype(F64)


def ulps32(got, want):
    """|got - want| in units of fp32 spacing at the larger magnitude"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    sp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(F32)).astype(F64)
    return np.abs(got.astype(F64) - want.astype(F64)) / sp


def quantize_sums(s):
    """sums as a table can hold them exactly: multiples of 2^-60 (only values below 2^-7 ever change)"""
    s = np.asarray(s, dtype=F64)
    return np.where(np.abs(s) < 2.0 ** -7, np.rint(s * 2.0 ** 60) / 2.0 ** 60, s)


def fold(sums, pixels, gamma, beta, eps, running_mean=None, running_var=None, af=1.0, unbias=1.0):
    """bn_finalize_kernel's expression on (sum y, sum y^2) [c, 2]: float64 statistics, fp32 arrays"""
    s, q = np.asarray(sums, F64)[:, 0], np.asarray(sums, F64)[:, 1]
    m = s / F64(pixels)
    var = np.maximum(q / F64(pixels) - m * m, 0.0)
    mean = m.astype(F32)
    invstd = (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)
    scale = (np.asarray(gamma, F32).astype(F64) * invstd.astype(F64)).astype(F32)
    shift = (-mean.astype(F64) * scale.astype(F64) + np.asarray(beta, F32).astype(F64)).astype(F32)   # fmaf: one rounding of the exact value
    out = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, var=var)
    if running_mean is not None:
        out["running_mean"] = ((1.0 - af) * np.asarray(running_mean, F32).astype(F64) + af * mean.astype(F64)).astype(F32)
        out["running_var"] = ((1.0 - af) * np.asarray(running_var, F32).astype(F64) + af * unbias * var).astype(F32)
    return out


def relu_mask(y, scale, shift):
    return np.asarray(y, F64) * np.asarray(scale, F32).astype(F64) + np.asarray(shift, F32).astype(F64) > 0


def bn_bwd_sums(da, y, mean, invstd, scale, shift):
    """(sums [c, 2] = (sum dz*xhat, sum dz), their sums of magnitudes [c, 2]) over (da, y) [P, c]"""
    dz = np.where(relu_mask(y, scale, shift), np.asarray(da, F64), 0.0)
    xhat = (np.asarray(y, F64) - np.asarray(mean, F32).astype(F64)) * np.asarray(invstd, F32).astype(F64)
    t = dz * xhat
    return np.stack([t.sum(0), dz.sum(0)], 1), np.stack([np.abs(t).sum(0), np.abs(dz).sum(0)], 1)


def bn_bwd_finalize(sums, pixels, gamma, invstd):
    """bn_bwd_finalize_kernel / bnacc_finish_backward on the totals: dgamma, dbeta, coef [3, c] = [gamma*invstd | sum dz / P | sum dz*xhat / P]"""
    g, b = np.asarray(sums, F64)[:, 0], np.asarray(sums, F64)[:, 1]
    k0 = (np.asarray(gamma, F32).astype(F64) * np.asarray(invstd, F32).astype(F64)).astype(F32)
    return g.astype(F32), b.astype(F32), np.stack([k0, (b / F64(pixels)).astype(F32), (g / F64(pixels)).astype(F32)])


def bn_bwd_apply(da, y, mean, invstd, scale, shift, coef):
    """dy = k0 * (dz - k1 - xhat * k2) in float64 (NOT yet rounded to storage), and the fp32 evaluation bound of the kernels' expression:
    8 * 2^-24 * |k0| * (|dz| + |k1| + |xhat * k2|)"""
    k0, k1, k2 = (np.asarray(coef, F32)[i].astype(F64) for i in range(3))
    dz = np.where(relu_mask(y, scale, shift), np.asarray(da, F64), 0.0)
    xhat = (np.asarray(y, F64) - np.asarray(mean, F32).astype(F64)) * np.asarray(invstd, F32).astype(F64)
    dy = k0 * (dz - k1 - xhat * k2)
    return dy, 8 * 2.0 ** -24 * np.abs(k0) * (np.abs(dz) + np.abs(k1) + np.abs(xhat * k2))


def head_input(sides, bf16):
    """The head's staged operand x [P, 32]: the sum over the sides (x, scale, shift) of relu(x*scale+shift), through the roundings of the
    value the kernel passes to operand_round — each side's fmaf lands in an fp32 register (here: the float64 value rounded to fp32, which
    differs from the single rounding of the exact value about once in 2^29 elements), the skip sum is an fp32 add, then the storage type.
    Returns (x as staged, float64; relu mask of the FIRST side)."""
    total, mask0 = None, None
    for xs, sc, sh in sides:
        z = (np.asarray(xs, F64) * np.asarray(sc, F32).astype(F64) + np.asarray(sh, F32).astype(F64)).astype(F32)
        if mask0 is None:
            mask0 = z > 0
        a = np.maximum(z, F32(0))
        total = a if total is None else (total.astype(F64) + a.astype(F64)).astype(F32)
    return (bf16_round(total) if bf16 else total).astype(F64), mask0


def f32_of_fraction(fr):
    """a Fraction rounded ONCE to fp32 (nearest even)"""
    from fractions import Fraction
    c = F32(float(fr))
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        d = abs(Fraction(float(cand)) - fr)
        even = (int(np.asarray(cand).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, cand)
    return best[1]


def head_input_exact(sides, bf16):
    """head_input with every fmaf rounded once from its exact value (fractions): what the kernel's fp32 registers hold"""
    from fractions import Fraction
    xs0 = np.asarray(sides[0][0], F32)
    out = np.zeros(xs0.shape, F32)
    for p in range(xs0.shape[0]):
        for c in range(xs0.shape[1]):
            total = None
            for xs, sc, sh in sides:
                z = f32_of_fraction(Fraction(float(xs[p, c])) * Fraction(float(F32(sc[c]))) + Fraction(float(F32(sh[c]))))
                a = z if z > 0 else F32(0)
                total = a if total is None else F32(total + a)   # one fp32 add: correctly rounded either way
            out[p, c] = total
    return (bf16_round(out) if bf16 else out).astype(F64)


def softmax_loss(z, labels, weights, scale):
    """loss_multiclass_log_per_pixel_weighted on logits z [P, K] (float64): (dlogits [P, K], loss, dbias [K], error)"""
    z = np.asarray(z, F64)
    p_, k_ = z.shape
    labels = np.asarray(labels).astype(np.int64)
    valid = (labels != LABEL_IGNORE) & (labels < k_)
    error = bool(((labels != LABEL_IGNORE) & (labels >= k_)).any())
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    sw = (F32(scale) * np.asarray(weights, F32)).astype(F64)      # the kernels' fp32 product
    onehot = np.zeros_like(p)
    onehot[np.nonzero(valid)[0], labels[valid]] = 1.0
    g = np.where(valid[:, None], sw[:, None] * (p - onehot), 0.0)
    py = np.where(valid, (p * onehot).sum(1), 1.0)
    loss = float((np.where(valid, sw, 0.0) * -np.log(np.maximum(py, 1e-10))).sum())
    return g, loss, g.sum(0), error


def head_train(sides, w_tm, bias, labels, weights, scale, bf16):
    """The fused tail from its inputs: x, logits, dlogits, loss, dbias, dw [32, K], da (float64, not yet rounded to storage)."""
    w = np.asarray(w_tm, F32)
    w = (bf16_round(w) if bf16 else w).astype(F64)
    x, mask0 = head_input(sides, bf16)
    z = x @ w + np.asarray(bias, F32).astype(F64)
    g, loss, dbias, error = softmax_loss(z, labels, weights, scale)
    return dict(x=x, mask=mask0, w=w, logits=z, dlogits=g, loss=loss, dbias=dbias, dw=x.T @ g, da=g @ w.T, error=error,
                logits_mag=np.abs(x) @ np.abs(w) + np.abs(np.asarray(bias, F64)))


def head_bn_sums(da_stored, y, mask, mean, invstd):
    """The head's sums of its input layer: (sum dz*xhat, sum dz) [32, 2] over the STORED da, and the magnitude of the form the kernel
    keeps them in — invstd * (sum |dz*y| + |mean| * sum |dz|): it holds sum dz*y and sum dz and subtracts afterwards."""
    dz = np.where(mask, np.asarray(da_stored, F64), 0.0)
    y = np.asarray(y, F64)
    m, i = np.asarray(mean, F32).astype(F64), np.asarray(invstd, F32).astype(F64)
    sums = np.stack([(dz * ((y - m) * i)).sum(0), dz.sum(0)], 1)
    mag = np.stack([i * (np.abs(dz * y).sum(0) + np.abs(m) * np.abs(dz).sum(0)), np.abs(dz).sum(0)], 1)
    plain = np.abs(dz * ((y - m) * i)).sum(0)
    return sums, mag, plain
