"""float64 numpy reference of the optimiser step (sgd_kernel) and of the parameter layouts it maintains
(tests/test_update_ref.py, tests/test_gpu_update.py).

The update of one parameter, as the kernel and the oracle write it, is ONE double expression rounded ONCE to float32:

    r  = mom * m - (wd * lr) * p * mask - lr * (g * scale)        (double; mask = 1 on filter elements, 0 on bias / gamma / beta)
    v' = float32(r)
    p' = p + v'                                                    (float32 add)

There is no reduction, so the only freedom an implementation has is how it rounds the INTERMEDIATES of r: a compiler may contract
a * b - c to one fma (device code does unless it is built with -ffp-contract=off), numpy rounds every product.  Both evaluations stay within 4 * 2^-53 * S of the exact value, S = |mom m| +
|wd lr p| + |lr g scale| (one rounding in the first term, two in each of the others, one per subtraction), so they can round to
DIFFERENT float32 values only where r lies within 8 * 2^-53 * S of a float32 rounding midpoint.  tie_guard() names those elements
and the two floats either side of the midpoint; everywhere else the float32 result is unique and a test may demand equality.  With
the decimal constants 0.9, 0.05 and 0.0005 exact-arithmetic ties are common (9m/10 - g/20 is a short binary number whenever 18m - g
is divisible by 5), which is why the guard exists; with dyadic constants and confined magnitudes r itself is exact (is_exact()) and
the guard is not needed at all.

layout_maps() states the two compute layouts by reshape / transpose per layer, not by the kernel's division chain.

Nothing here computes with the library; net_shape() only asks it for the layer list of a configuration (no GPU needed).
"""
import numpy as np

from conftest import random_params

F32, F64 = np.float32, np.float64

# (levels, in_channels, classes, width_scaler, min_filters)
CASE_NETS = [
    (2, 3, 3, 0.25, 4),    # baseline net with con and cont layers
    (3, 1, 5, 0.125, 4),   # deepest net, one input channel, head above four classes
    (2, 3, 9, 0.1, 5),     # channel counts that are not multiples of anything
    (1, 3, 2, 1.0, 1),     # full width, 32-channel layers
]

# (lr, wd, mom, scale)
HYPER_DYADIC = [(3 / 64, 2.0 ** -5, 0.875, 1.0), (3 / 64, 2.0 ** -5, 0.875, 0.25), (3 / 64, 2.0 ** -5, 0.875, 4.0), (0.5, 0.25, 0.0, 1.0)]
HYPER_DECIMAL = [(0.05, 0.0005, 0.9, 1.0), (0.05, 0.3, 0.9, 1.0 / 3.0), (0.05, 0.0, 0.9, 1.0)]
# Standard deviation of the gradients drawn for each of HYPER_DECIMAL.  1e-2 is the size of a training run.  Without weight decay r has
# only two terms, and at that size (18 m - g) / 20 is an exact float32 midpoint for 4.6 % of the elements (measured with tie_guard on
# the case nets); the share falls as the two terms move apart in magnitude (1.9 % at 0.16, 0.25 % at 2.56), so the wd = 0 set draws
# gradients of size 8, where it is below 0.1 %.  The momentum term still reaches the float32 result there (0.9 * 1e-3 against ulps of 3e-8).
G_SIGMA_DECIMAL = [1e-2, 1e-2, 8.0]
DECIMAL_SEEDS = (31,)      # seeds of decimal_inputs that the GPU tests use
DYADIC_SEED = 41
GUARD_SHARE_CAP = 0.005    # |T| / n above this and the guard could hide a failure: a condition on the inputs, asserted before comparing

KINDS = ("filter", "bias", "gamma", "beta")


class NetShape:
    """layer list and blob sizes of a net configuration (what conftest.random_params reads)"""

    def __init__(self, layers, n_params, n_running):
        self.layers, self.n_params, self.n_running = layers, int(n_params), int(n_running)


def net_shape(case):
    import ctypes as C

    import annonet_amd as aa
    cfg = aa.net_config(*case, aa.ANH_FP32)
    return NetShape(aa.net_layers(cfg), aa.lib().anh_net_param_count(C.byref(cfg)), aa.lib().anh_net_running_count(C.byref(cfg)))


def segments(layers):
    """(layer index, kind, start, count) of every parameter segment, in blob order"""
    out = []
    for li, L in enumerate(layers):
        out.append((li, "filter", int(L.w_off), L.k * L.k * L.cin * L.cout))
        if L.has_bias:
            out.append((li, "bias", int(L.b_off), L.cout))
        if L.has_bn:
            out.append((li, "gamma", int(L.g_off), L.cout))
            out.append((li, "beta", int(L.beta_off), L.cout))
    return sorted(out, key=lambda s: s[2])


def param_count(layers):
    return max(start + count for _, _, start, count in segments(layers))


def filter_mask(layers):
    mask = np.zeros(param_count(layers), dtype=bool)
    for _, kind, start, count in segments(layers):
        if kind == "filter":
            mask[start:start + count] = True
    return mask


def layout_maps(layers):
    """-> (tap_major, k_major): for every canonical index of the parameter blob, its index in the tap-major and in the k-major blob.
    Canonical filters are [co][ci][t] (type 0, con) or [ci][co][t] (type 1, cont); tap-major is [t][ci][co], k-major [t][co][ci];
    bias, gamma and beta map to themselves."""
    n = param_count(layers)
    tm, km = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    for L in layers:
        kk, cin, cout, off = L.k * L.k, L.cin, L.cout, int(L.w_off)
        cnt = kk * cin * cout
        in_tm = np.arange(cnt, dtype=np.int64).reshape(kk, cin, cout)     # a [t][ci][co] array holding its own flat indices
        in_km = np.arange(cnt, dtype=np.int64).reshape(kk, cout, cin)     # likewise [t][co][ci]
        if L.type == 0:      # read both in canonical order [co][ci][t]
            tm[off:off + cnt] = off + in_tm.transpose(2, 1, 0).reshape(-1)
            km[off:off + cnt] = off + in_km.transpose(1, 2, 0).reshape(-1)
        else:                # canonical order [ci][co][t]
            tm[off:off + cnt] = off + in_tm.transpose(1, 2, 0).reshape(-1)
            km[off:off + cnt] = off + in_km.transpose(2, 1, 0).reshape(-1)
    return tm, km


def to_tap_major(canonical, tap_major):
    """a canonical blob as the gradient bucket holds it"""
    out = np.empty_like(canonical)
    out[tap_major] = canonical
    return out


def _terms(p, m, g, mask, lr, wd, mom, scale):
    p, m, g = (np.asarray(a, dtype=F32).astype(F64) for a in (p, m, g))
    a = F64(mom) * m
    b = np.where(mask, (F64(wd) * F64(lr)) * p, 0.0)
    c = F64(lr) * (g * F64(scale))
    return a, b, c


def sgd_ref(p, m, g_canonical, mask, lr, wd, mom, scale):
    """-> (v', p') as float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = _terms(p, m, g_canonical, mask, lr, wd, mom, scale)
        v = (a - b - c).astype(F32)
        return v, np.asarray(p, dtype=F32) + v


def tie_guard(p, m, g_canonical, mask, lr, wd, mom, scale):
    """-> (T, lo, hi): T marks the elements whose double result r lies within 8 * 2^-53 * (|mom m| + |wd lr p| + |lr g scale|) of the
    float32 rounding midpoint nearest to it; lo < hi (float32, one entry per element of T, in index order) bracket that midpoint."""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = _terms(p, m, g_canonical, mask, lr, wd, mom, scale)
        r = a - b - c
        near = r.astype(F32)
        # the midpoint nearest to r lies between float32(r) and its neighbour on r's side (upwards when r is a float32 itself)
        far = np.nextafter(near, np.where(near.astype(F64) > r, F32(-np.inf), F32(np.inf)).astype(F32))
        lo, hi = np.minimum(near, far), np.maximum(near, far)
        mid = 0.5 * (lo.astype(F64) + hi.astype(F64))
        tol = 8.0 * 2.0 ** -53 * (np.abs(a) + np.abs(b) + np.abs(c))
        T = np.isfinite(r) & np.isfinite(mid) & (np.abs(r - mid) <= tol)
    return T, lo[T], hi[T]


def is_exact(p, m, g_canonical, mask, lr, wd, mom, scale):
    """True where the double evaluation of r is the exact real number: recomputed in extended precision where np.longdouble has a
    64-bit significand (x86), else in rationals."""
    a, b, c = _terms(p, m, g_canonical, mask, lr, wd, mom, scale)
    r = a - b - c
    if np.finfo(np.longdouble).nmant >= 63:
        LD = np.longdouble
        pl, ml, gl = (np.asarray(x, dtype=F32).astype(LD) for x in (p, m, g_canonical))
        exact = LD(mom) * ml - np.where(mask, LD(wd) * LD(lr) * pl, LD(0)) - LD(lr) * (gl * LD(scale))
        return exact == r.astype(LD)
    from fractions import Fraction as Fr
    out = np.empty(r.shape, dtype=bool)
    for i in range(r.size):
        e = Fr(mom) * Fr(float(m[i])) - (Fr(wd) * Fr(lr) * Fr(float(p[i])) if mask[i] else 0) - Fr(lr) * Fr(float(g_canonical[i])) * Fr(scale)
        out[i] = e == Fr(float(r[i]))
    return out


# ---- the inputs of the GPU tests (here so that the CPU suite can hold them to the guard-share condition) ----
def decimal_inputs(shape, seed, g_sigma=1e-2):
    """Glorot filters, bn gamma / beta and head bias as the other tests draw them; m ~ N(0, 1e-3), g ~ N(0, g_sigma)"""
    p, running = random_params(shape, seed)
    rng = np.random.default_rng(seed + 1000)
    m = rng.normal(0, 1e-3, shape.n_params).astype(F32)
    g = rng.normal(0, g_sigma, shape.n_params).astype(F32)
    return p, running, m, g


def dyadic_inputs(shape, seed):
    """p, m, g with magnitudes uniform in [2^-12, 2^-6] and random signs: with HYPER_DYADIC every product and the three-term sum fit
    a double's 53 bits (lowest bit >= 2^-47, sum below 2^-4), so r is exact (the tests assert it with is_exact)"""
    _, running = random_params(shape, seed)
    rng = np.random.default_rng(seed + 2000)

    def draw():
        return (rng.uniform(2.0 ** -12, 2.0 ** -6, shape.n_params) * rng.choice([-1.0, 1.0], shape.n_params)).astype(F32)
    return draw(), running, draw(), draw()
