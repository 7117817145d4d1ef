"""The half of the bf16 training step the per-op tests never reached: the batch-norm accumulator tables ("table mode", bnacc.h — the
default of the step bench.py times) and the training kernels that are not convolutions, one kernel at a time on identical inputs
against the float64 references of tests/train_ops_ref.py.

  bn_fold_all / bnacc_get        tables built on the host, spread over all 16 replicas with mixed signs
  conv epilogues and prologues   statistics added into a table, producers' tables folded while staging, backward sums + finish
  bn_bwd_reduce* / finalize / bn_bwd_apply*   scalar, vector and head form; partials and table + finish; in place and out of place
  head_train_kernel + head_finalize           every class count, source kind, type and form of its bn sums
  loss_kernel<4|8|64> + loss_finalize
  the trainer's table life cycle (clear on a pass that no update followed, ticket reset)

Bars.  Exact where the arithmetic is on integers (finish from the decoded totals, ticket counts) or two forms of one kernel are compared
(bit-identity).  Derived where a rounding model exists: half a storage ulp of the float64 value plus the fp32 evaluation bound stated at
each use.  Where neither applies (softmax through expf / logf, dw, dbias) the project's existing bars for the same quantity on
identical inputs are the caps — loss 2e-5 * max(1, |loss|); head gradients rtol 2e-3, atol 2e-5 * max |g| — and the bar in force is
4 x the worst value observed on an MI355X, written as a fraction of the cap next to the observed figure (MEASURED below).
"""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import test_gpu_ops as ops
import train_ops_ref as ref
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

BF, FP = aa.ANH_BF16, aa.ANH_FP32
U24 = 2.0 ** -24
TINY = 2.0 ** -126   # below fp32's normal range (the gradient of a decided pixel) neither storage type keeps its relative precision
EPS = 1e-4

# name: (bar in force as a fraction of the cap, worst fraction observed).  Caps: see the module docstring.
MEASURED = {
    "head dlogits": (0.0337, 0.00843),
    "head loss": (0.0226, 0.00566),
    "head dbias": (0.00131, 0.000327),
    "head dw": (0.00764, 0.00191),
    "loss dlogits": (0.0246, 0.00616),
    "loss loss": (0.0261, 0.00653),
    "loss dbias": (0.00608, 0.00152),
}
_seen = {}


def measured(name, fraction):
    """one figure of a measured quantity: printed (pytest -s shows the worst per test), held to the bar in force"""
    fraction = float(fraction)
    _seen[name] = max(_seen.get(name, 0.0), fraction)
    print("measured %-14s %.3g of its cap (worst so far %.3g)" % (name, fraction, _seen[name]))
    assert fraction <= MEASURED[name][0], (name, fraction)


def half_ulp(v, bf16):
    """half a storage ulp at the float64 value v"""
    return 0.5 * ref.bf16_ulp(v) if bf16 else U24 * np.abs(v)


def rnd(a, bf16):
    return ref.bf16_round(a) if bf16 else np.asarray(a, np.float32)


def real_sums(y):
    """(sum y, sum y^2) [c, 2] of a stored tensor [P, c], as a table holds them"""
    y64 = np.asarray(y, np.float64).reshape(-1, y.shape[-1])
    return ref.quantize_sums(np.stack([y64.sum(0), (y64 * y64).sum(0)], 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# fold
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_fold(got, want, what, ulps=1.0):
    """bn_finalize_kernel's expression: the float64 statistics are the same operations in the same order (the library is built without
    contraction), so mean and var agree exactly unless a double division / square root differs in its last place: 1 fp32 ulp for the
    arrays behind them; 2^-52 of q/P + m^2 for var."""
    for n in ("mean", "invstd", "scale", "shift", "running_mean", "running_var"):
        if n in want:
            u = ref.ulps32(got[n], want[n])
            assert np.isfinite(got[n]).all() and (u <= ulps).all(), (what, n, float(u.max()))
    vmag = want["var"] + 2 * want["mean"].astype(np.float64) ** 2 + 1e-300
    assert (np.abs(got["var"] - want["var"]) <= 2.0 ** -51 * vmag).all(), (what, "var")


def fold_jobs():
    rng = np.random.default_rng(77)
    jobs = []
    for i in range(16):
        c = (8, 32, 64, 256)[i % 4] if i < 12 else (256, 8, 64, 32)[i - 12]
        pixels = int(rng.integers(1, 200000))
        mean = rng.normal(0, 2, c)
        var = rng.uniform(0.05, 4, c)
        s = np.rint(mean * pixels * 2.0 ** 20) / 2.0 ** 20
        q = np.rint((var + mean * mean) * pixels * 2.0 ** 20) / 2.0 ** 20
        j = dict(c=c, pixels=pixels, eps=EPS, gamma=rng.uniform(0.5, 1.5, c).astype(np.float32), beta=rng.uniform(-0.3, 0.3, c).astype(np.float32),
                 running_mean=rng.normal(0, 1, c).astype(np.float32), running_var=rng.uniform(0.5, 2, c).astype(np.float32),
                 af=1.0 / (1 + i), unbias=pixels / (pixels - 1.0) if pixels > 1 else 1.0)
        if i == 5:   # var at 0: sum y^2 = (sum y)^2 / P exactly (all three are powers of two times small integers), and below it in every second channel
            j["pixels"] = pixels = 4096
            s = np.round(rng.uniform(-3000, 3000, c) * 2) / 2
            q = s * s / pixels
            q[1::2] -= 2.0 ** -8 * rng.integers(1, 9, c // 2)
        if i == 9:
            j["running_mean"] = j["running_var"] = None
        j["sums"] = np.stack([s, q], 1)
        jobs.append(j)
    return jobs


def test_fold_of_sixteen_tables_in_one_launch():
    jobs = fold_jobs()
    got = aa.op_bn_fold(jobs, spread_seed=3)
    for i, (j, g) in enumerate(zip(jobs, got)):
        want = ref.fold(j["sums"], j["pixels"], j["gamma"], j["beta"], j["eps"], j["running_mean"], j["running_var"], j["af"], j["unbias"])
        assert_fold(g, want, ("job", i, j["c"]))
        assert ("running_mean" in g) == (j["running_mean"] is not None)
    assert (got[5]["var"] == 0).all() and np.allclose(got[5]["invstd"], 100.0, rtol=1e-6)
    again = aa.op_bn_fold(jobs, spread_seed=4)   # another spread of the same totals: integers, so bit-identical
    for g, h in zip(got, again):
        for n in g:
            np.testing.assert_array_equal(g[n], h[n])


@pytest.mark.parametrize("precision", [FP, BF])
@pytest.mark.parametrize("c,pixels", [(8, 1000), (24, 700), (32, 5000), (64, 1031), (256, 300)])
def test_fold_agrees_with_the_partials_form(c, pixels, precision):
    """the same tensor through the statistics kernel + finalize, and its sums through a table + fold: the same arrays to 1 ulp"""
    rng = np.random.default_rng(c + pixels)
    y = rnd(rng.normal(rng.normal(0, 1, c), rng.uniform(0.3, 2, c), (pixels, c)).astype(np.float32), precision == BF)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
    rm, rv = rng.normal(0, 1, c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32)
    kw = dict(af=0.25, unbias=pixels / (pixels - 1.0))
    part, sums = aa.op_bn_forward_stats(precision, y, gamma, beta, EPS, rm, rv, **kw)
    y64 = y.astype(np.float64)
    want = np.stack([y64.sum(0), (y64 * y64).sum(0)], 1)
    mag = np.stack([np.abs(y64).sum(0), (y64 * y64).sum(0)], 1) + 1e-12
    assert (np.abs(sums - want) <= 2e-5 * mag).all(), float((np.abs(sums - want) / mag).max())
    q = ref.quantize_sums(sums)
    tab, = aa.op_bn_fold([dict(c=c, pixels=pixels, eps=EPS, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, sums=q, **kw)])
    assert_fold(part, tab, ("partials vs table", c))
    assert_fold(tab, ref.fold(q, pixels, gamma, beta, EPS, rm, rv, **kw), ("table vs float64", c))


# ---------------------------------------------------------------------------------------------------------------------------------
# conv epilogues / prologues in table form
# ---------------------------------------------------------------------------------------------------------------------------------
STEM = ((0, 5, 1, 2, 3, 32), 2, 19, 23)


def check_forward_sums(r, cout):
    y64 = r["y"].astype(np.float64).reshape(-1, cout)
    want = np.stack([y64.sum(0), (y64 * y64).sum(0)], 1)
    mag = np.stack([np.abs(y64).sum(0), (y64 * y64).sum(0)], 1) + 1e-12
    assert (np.abs(r["sums"] - want) <= 2e-5 * mag).all(), float((np.abs(r["sums"] - want) / mag).max())
    return mag


def check_table_against_partials(tab, par, mag):
    """each workgroup's partial is one double either way; the table adds them as integers (exact, 2^-61 per add), the host adds the
    partials in double: at most one rounding of the running sum per workgroup"""
    assert np.array_equal(tab["y"], par["y"])
    bound = max(par["workgroups"], tab["workgroups"]) * 2.0 ** -52 * mag
    assert (np.abs(tab["sums"] - par["sums"]) <= bound).all(), float((np.abs(tab["sums"] - par["sums"]) / bound).max())
    assert tab["poison"] == 0 and tab["ticket"] == 0 and tab["workgroups"] >= 1   # (only the backward finish draws tickets)


@pytest.mark.parametrize("prologue", [1, 2])
@pytest.mark.parametrize("desc,n,h,w", ops.FUSED_SHAPES)
def test_conv_forward_into_a_table(desc, n, h, w, prologue):
    xa, kw, filters, _ = ops.make_inputs(desc, n, h, w, 11, prologue, True)
    a = dict(x=xa, scale=kw["sa"], shift=kw["ta"])
    b = dict(x=kw["xb"], scale=kw["sb"], shift=kw["tb"]) if prologue == 2 else None
    y_ref, _, _ = aa.op_conv_forward_stats(BF, desc, xa, filters=filters, **kw)
    tab = aa.op_conv_forward_stats_table(BF, desc, a, b, filters=filters, tables=True)
    par = aa.op_conv_forward_stats_table(BF, desc, a, b, filters=filters, tables=False)
    assert np.array_equal(tab["y"], y_ref)
    check_table_against_partials(tab, par, check_forward_sums(tab, desc[5]))


def test_stem_forward_into_a_table(shape=STEM):
    desc, n, h, w = shape
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    k = desc[1]
    lim = np.sqrt(6.0 / (k * k * (desc[4] + desc[5])))
    filters = rng.uniform(-lim, lim, k * k * desc[4] * desc[5]).astype(np.float32)
    tab = aa.op_conv_forward_stats_table(BF, desc, image=img, filters=filters, tables=True)
    par = aa.op_conv_forward_stats_table(BF, desc, image=img, filters=filters, tables=False)
    assert np.isfinite(tab["y"]).all() and np.abs(tab["y"]).max() > 0
    check_table_against_partials(tab, par, check_forward_sums(tab, desc[5]))


@pytest.mark.parametrize("prologue", [1, 2])
@pytest.mark.parametrize("desc,n,h,w", ops.FUSED_SHAPES)
def test_conv_prologue_folds_its_producers_tables(desc, n, h, w, prologue):
    xa, kw, filters, rng = ops.make_inputs(desc, n, h, w, 13, prologue, True)
    cin = desc[4]
    sides = [xa] + ([kw["xb"]] if prologue == 2 else [])
    spec, jobs = [], []
    for x in sides:
        gamma, beta = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(-0.3, 0.3, cin).astype(np.float32)
        sums = real_sums(x)
        spec.append(dict(x=x, sums=sums, gamma=gamma, beta=beta, eps=EPS))
        jobs.append(dict(c=cin, pixels=n * h * w, eps=EPS, gamma=gamma, beta=beta, sums=sums))
    folded = aa.op_bn_fold(jobs)
    tab = aa.op_conv_forward_stats_table(BF, desc, spec[0], spec[1] if prologue == 2 else None, filters=filters, tables=True)
    arrays = dict(sa=folded[0]["scale"], ta=folded[0]["shift"])
    if prologue == 2:
        arrays.update(xb=kw["xb"], sb=folded[1]["scale"], tb=folded[1]["shift"])
    y_ref, sums_ref, _ = aa.op_conv_forward_stats(BF, desc, xa, filters=filters, **arrays)
    assert np.isfinite(tab["y"]).all() and np.array_equal(tab["y"], y_ref)
    mag = check_forward_sums(tab, desc[5])
    assert (np.abs(tab["sums"] - sums_ref) <= tab["workgroups"] * 2.0 ** -52 * mag).all()
    assert tab["poison"] == 0


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("desc,n,h,w", ops.FUSED_SHAPES)
def test_conv_backward_data_with_table_sums_and_finish(desc, n, h, w, accumulate):
    rng = np.random.default_rng(5)
    cin, cout = desc[4], desc[5]
    ho, wo = aa.netpimpl._out_dim(desc, h), aa.netpimpl._out_dim(desc, w)
    k = desc[1]
    lim = np.sqrt(6.0 / (k * k * (cin + cout)))
    filters = rng.uniform(-lim, lim, k * k * cin * cout).astype(np.float32)
    dy = orc.bf16_round(rng.normal(0, 1, (n, ho, wo, cout)).astype(np.float32))
    y_prev = orc.bf16_round(rng.normal(0, 1, (n, h, w, cin)).astype(np.float32))
    init = orc.bf16_round(rng.normal(0, 1, (n, h, w, cin)).astype(np.float32)) if accumulate else None
    scale = rng.uniform(0.5, 1.5, cin).astype(np.float32); shift = rng.uniform(-0.3, 0.3, cin).astype(np.float32)
    mean = rng.uniform(-0.2, 0.2, cin).astype(np.float32); invstd = rng.uniform(0.7, 1.4, cin).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    dx_ref, _, _ = aa.op_conv_backward_data_bn(BF, desc, dy, filters, (h, w), y_prev, scale, shift, mean, invstd, dx_init=init)
    r = aa.op_conv_backward_data_bn_table(BF, desc, dy, filters, (h, w), y_prev, scale, shift, mean, invstd, gamma, dx_init=init)
    assert np.array_equal(r["dx"], dx_ref)
    # the existing bar of the partials form: fp32 mask and xhat expressions over the stored dx, 1e-4 of the sums of magnitudes
    z = y_prev.astype(np.float64) * scale + shift
    dz = np.where(z > 0, r["dx"], 0).astype(np.float64)
    xhat = ((y_prev - mean).astype(np.float32) * invstd).astype(np.float64)
    want = np.stack([(dz * xhat).reshape(-1, cin).sum(0), dz.reshape(-1, cin).sum(0)], 1)
    mag = np.stack([np.abs(dz * xhat).reshape(-1, cin).sum(0), np.abs(dz).reshape(-1, cin).sum(0)], 1) + 1e-12
    assert (np.abs(r["sums"] - want) <= 1e-4 * mag).all(), float((np.abs(r["sums"] - want) / mag).max())
    assert_finish_is_exact(r, n * h * w, gamma, invstd)


def assert_finish_is_exact(r, pixels, gamma, invstd):
    """the finish is deterministic arithmetic on the table's integers: dgamma, dbeta and coef follow EXACTLY from the decoded totals, and
    the ticket has counted every workgroup of the launch (an unfinished table leaves the NaN prefill behind)"""
    dgamma, dbeta, coef = ref.bn_bwd_finalize(r["sums"] if "sums" in r else r["bn_sums"], pixels, gamma, invstd)
    np.testing.assert_array_equal(r["dgamma"], dgamma)
    np.testing.assert_array_equal(r["dbeta"], dbeta)
    np.testing.assert_array_equal(r["coef"], coef)
    assert r["ticket"] == r["workgroups"] >= 1, (r["ticket"], r["workgroups"])


# ---------------------------------------------------------------------------------------------------------------------------------
# bn + relu backward alone
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bn_case(c, pixels, bf16):
    rng = np.random.default_rng(1000 * c + pixels)
    y = rnd(rng.normal(rng.normal(0, 1, c), rng.uniform(0.5, 1.5, c), (pixels, c)).astype(np.float32), bf16)
    da = rnd(rng.normal(0, 1, (pixels, c)).astype(np.float32), bf16)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(-0.3, 0.3, c).astype(np.float32)
    f = ref.fold(real_sums(y), pixels, gamma, beta, EPS)
    return y, da, gamma, f


def check_bn_backward(c, pixels, precision, tables_forms=(False, True)):
    bf16 = precision == BF
    y, da, gamma, f = bn_case(c, pixels, bf16)
    arrays = (f["mean"], f["invstd"], f["scale"], f["shift"])
    want_sums, mag = ref.bn_bwd_sums(da, y, *arrays)
    vector = c % 8 == 0 and 256 % (c // 8) == 0
    for tables in tables_forms:
        if tables and not vector:
            continue
        r = aa.op_bn_backward(precision, y, *arrays, da=da, gamma=gamma, tables=tables, stages=5 if tables else 7)   # the table form has no finalize kernel
        assert (np.abs(r["sums"] - want_sums) <= 1e-4 * mag + 1e-300).all(), (tables, float((np.abs(r["sums"] - want_sums) / (mag + 1e-300)).max()))
        if tables:
            assert_finish_is_exact(r, pixels, gamma, f["invstd"])
        else:   # the finalize kernel adds the partials in its own order: the totals may differ from the host's in the last place of a double
            dgamma, dbeta, coef = ref.bn_bwd_finalize(r["sums"], pixels, gamma, f["invstd"])
            for got, want in ((r["dgamma"], dgamma), (r["dbeta"], dbeta), (r["coef"], coef)):
                assert (ref.ulps32(got, want) <= 1).all()
            np.testing.assert_array_equal(r["coef"][0], coef[0])
        # dy from the coefficients the kernel read: half a storage ulp of the float64 value + the fp32 evaluation bound
        # 8 * 2^-24 * |k0| * (|dz| + |k1| + |xhat * k2|) (six roundings: y - m, * invstd, * k2, dz - k1, the difference, * k0)
        dy64, ev = ref.bn_bwd_apply(da, y, *arrays, r["coef"])
        bound = half_ulp(dy64, bf16) * 1.0001 + ev + TINY
        assert (np.abs(r["dy"] - dy64) <= bound).all(), (tables, float((np.abs(r["dy"] - dy64) / (bound + 1e-300)).max()))
        out = aa.op_bn_backward(precision, y, *arrays, da=da, tables=False, out_of_place=True, stages=4, coef_in=r["coef"])
        np.testing.assert_array_equal(out["dy"], r["dy"])   # the same coefficients, dy to its own buffer: the same bits


@pytest.mark.parametrize("precision", [FP, BF])
@pytest.mark.parametrize("pixels", [1, 255, 257, 4099])   # 4099: 17 workgroups, the replica index wraps past 16
@pytest.mark.parametrize("c", [8, 24, 32, 40, 64, 128, 256])   # 24 and 40 take the scalar kernels
def test_bn_backward(c, pixels, precision):
    check_bn_backward(c, pixels, precision)


@pytest.mark.parametrize("c,pixels", [(32, 170000), (256, 21000)])
def test_bn_backward_apply_walks_its_grid_stride_loop(c, pixels):
    """more than 2560 workgroups' worth of chunks: the apply kernels' loop runs more than once"""
    assert pixels * c // 8 > 2560 * 256
    check_bn_backward(c, pixels, BF, tables_forms=(True,))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused head
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def head_case(K, pixels, skip, bf16, sigmas=0.0, bad_label=False):
    rng = np.random.default_rng(100 * K + pixels % 97 + (7 if skip else 0) + (3 if bf16 else 0))
    sides = []
    for _ in range(2 if skip else 1):
        y = rnd(rng.normal(rng.normal(sigmas, 0.3, 32), 1.0, (pixels, 32)).astype(np.float32), bf16)
        gamma, beta = rng.uniform(0.5, 1.5, 32).astype(np.float32), rng.uniform(-0.3, 0.3, 32).astype(np.float32)
        sums = real_sums(y)
        sides.append(dict(x=y, gamma=gamma, beta=beta, sums=sums, eps=EPS))
    folded = aa.op_bn_fold([dict(c=32, pixels=pixels, eps=EPS, gamma=s["gamma"], beta=s["beta"], sums=s["sums"]) for s in sides])
    for s, f in zip(sides, folded):   # the arrays the library folds from these sums (held to float64 by the fold tests): both forms of an input say the same
        s.update(scale=f["scale"], shift=f["shift"], mean=f["mean"], invstd=f["invstd"])
    w = rng.uniform(-4, 4, (32, K)).astype(np.float32)   # logits spread over +-30
    bias = rng.uniform(-1, 1, K).astype(np.float32)
    labels = rng.integers(0, K, pixels).astype(np.uint16)
    labels[rng.random(pixels) < 0.05] = aa.LABEL_IGNORE
    if bad_label:
        labels[pixels // 2] = K
    weights = rng.uniform(0.5, 2.0, pixels).astype(np.float32)
    weights[rng.random(pixels) < 0.1] = 0
    scale = 1.0 / pixels
    want = ref.head_train([(s["x"], s["scale"], s["shift"]) for s in sides], w, bias, labels, weights, scale, bf16)
    return sides, w, bias, labels, weights, scale, want


def array_form(s):
    return dict(x=s["x"], scale=s["scale"], shift=s["shift"])


def table_form(s):
    return dict(x=s["x"], sums=s["sums"], gamma=s["gamma"], beta=s["beta"], eps=s["eps"])


def run_head(precision, case, table_inputs=False, **kw):
    sides, w, bias, labels, weights, scale, _ = case
    form = table_form if table_inputs else array_form
    return aa.op_head_train(precision, form(sides[0]), form(sides[1]) if len(sides) == 2 else None, w, bias, labels, weights, scale, **kw)


def check_head_against_float64(r, case, bf16):
    sides, w, bias, labels, weights, scale, want = case
    pixels, K = want["logits"].shape
    # logits: 8 fmaf per lane + 2 cross-lane adds + bias in fp32 on the staged operand: 16 * 2^-24 of the sum of magnitudes covers the
    # chain and, in fp32 storage, an operand whose fmaf rounded the other way (last place).  A bf16 operand that rounds the other way
    # than the reference's (its fmaf is the float64 value rounded to fp32: ~2^-29 of the elements, train_ops_ref.head_input) moves a
    # pixel by up to one bf16 ulp of the operand times |w|: at most 1e-4 of the pixels may leave the tight bound, and only that far.
    tight = 16 * U24 * want["logits_mag"]
    err = np.abs(r["logits"] - want["logits"])
    flipped = (err > tight).any(1)
    loose = tight + ref.bf16_ulp(want["x"]) @ np.abs(want["w"]) if bf16 else tight
    assert flipped.mean() <= 1e-4 and (err <= loose).all(), (int(flipped.sum()), float((err / loose).max()))
    ok = ~flipped
    gmax = np.abs(want["dlogits"]).max()
    cap = 2e-3 * np.abs(want["dlogits"]) + 2e-5 * gmax + 1e-300
    measured("head dlogits", (np.abs(r["dlogits"] - want["dlogits"])[ok] / cap[ok]).max() if ok.any() else 0.0)
    assert (np.abs(r["dlogits"] - want["dlogits"]) <= cap + 2 * (weights * np.float32(scale))[:, None] * loose.max(1, keepdims=True)).all()
    measured("head loss", abs(r["loss"] - want["loss"]) / (2e-5 * max(1.0, abs(want["loss"]))))
    measured("head dbias", (np.abs(r["dbias"] - want["dbias"]) / (2e-3 * np.abs(want["dbias"]) + 2e-5 * np.abs(want["dbias"]).max() + 1e-300)).max())
    measured("head dw", (np.abs(r["dw"] - want["dw"]) / (2e-3 * np.abs(want["dw"]) + 2e-5 * np.abs(want["dw"]).max() + 1e-300)).max())
    assert r["error_flag"] == int(want["error"])
    # da from the dlogits the kernel itself stored: K fmaf in fp32, then the storage rounding
    da64 = r["dlogits"].astype(np.float64) @ want["w"].T
    if r["da"] is not None:
        bound = half_ulp(da64, bf16) * 1.0001 + 4 * U24 * (np.abs(r["dlogits"]).astype(np.float64) @ np.abs(want["w"]).T) + TINY
        assert (np.abs(r["da"] - da64) <= bound).all(), float((np.abs(r["da"] - da64) / (bound + 1e-300)).max())
    return da64


@pytest.mark.parametrize("precision", [FP, BF])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("pixels", [1, 203, 98381])   # 98381 on 512 workgroups: the two-pixel loop twice, its second half for 77 pixels only
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_head_train(K, pixels, skip, precision):
    bf16 = precision == BF
    case = head_case(K, pixels, skip, bf16)
    r = run_head(precision, case)
    check_head_against_float64(r, case, bf16)
    v = run_head(precision, case, da_virtual=True)   # da not stored: nothing else may move
    for n in ("logits", "dlogits", "dbias", "dw"):
        np.testing.assert_array_equal(v[n], r[n])
    assert v["loss"] == r["loss"] and v["da"] is None


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_reference_operand_agrees_with_exact_fractions(K, skip):
    """With the seeds chosen the reference alone produces no flipped operand: its float64-then-fp32 fmaf equals the single rounding of
    the exact value on every element of the 203-pixel cases (computed on the host)."""
    sides = head_case(K, 203, skip, True)[0]
    triples = [(s["x"], s["scale"], s["shift"]) for s in sides]
    np.testing.assert_array_equal(ref.head_input(triples, True)[0], ref.head_input_exact(triples, True))


@pytest.mark.parametrize("precision", [FP, BF])
@pytest.mark.parametrize("K", [2, 3])
def test_head_train_flags_a_label_out_of_range(K, precision):
    case = head_case(K, 203, False, precision == BF, bad_label=True)
    r = run_head(precision, case)
    assert r["error_flag"] == 1
    assert (r["dlogits"][203 // 2] == 0).all() and (r["da"][203 // 2] == 0).all()
    check_head_against_float64(r, case, precision == BF)


def check_head_bn_sums(r, case, bf16, da_stored):
    """(sum dz*xhat, sum dz) of the input layer over the stored da.  The kernel keeps sum dz*y and sum dz in fp32 per thread and forms
    invstd * (sum dz*y - mean * sum dz) afterwards, so the existing backward bar (1e-4) applies to the magnitude of THAT form."""
    sides, want = case[0], case[6]
    s = sides[0]
    sums, mag, plain = ref.head_bn_sums(da_stored, s["x"], want["mask"], s["mean"], s["invstd"])
    err = np.abs(r["bn_sums"] - sums)
    assert (err <= 1e-4 * mag + 1e-300).all(), float((err / (mag + 1e-300)).max())
    return float((err[:, 0] / (plain + 1e-300)).max())


@pytest.mark.parametrize("pixels", [203, 98381])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_head_train_bn_sums_in_all_three_forms(K, pixels):
    case = head_case(K, pixels, False, True)
    sides, w = case[0], case[1]
    s = sides[0]
    base = run_head(BF, case)
    check_head_against_float64(base, case, True)
    same = ("logits", "dlogits", "da", "dbias", "dw")
    # partials
    p = run_head(BF, case, bn_sums=1, bn_mean=s["mean"], bn_invstd=s["invstd"])
    for n in same:
        np.testing.assert_array_equal(p[n], base[n])
    check_head_bn_sums(p, case, True, base["da"])
    assert np.isnan(p["coef"]).all()
    # table + finish, the input's arrays folded in the kernel, da stored and virtual
    for virtual in (False, True):
        t = run_head(BF, case, table_inputs=True, bn_sums=2, bn_gamma=s["gamma"], da_virtual=virtual)
        for n in same:
            if not (virtual and n == "da"):
                np.testing.assert_array_equal(t[n], base[n])
        assert t["loss"] == base["loss"]
        check_head_bn_sums(t, case, True, base["da"])
        assert_finish_is_exact(t, pixels, s["gamma"], s["invstd"])
        bound = t["workgroups"] * 2.0 ** -52 * ref.head_bn_sums(base["da"], s["x"], case[6]["mask"], s["mean"], s["invstd"])[1]
        assert (np.abs(t["bn_sums"] - p["bn_sums"]) <= bound).all()   # the same per-workgroup doubles, added as integers


def test_head_train_folds_other_layers_in_its_first_workgroups():
    jobs = fold_jobs()
    want = aa.op_bn_fold(jobs)
    for K, pixels in ((3, 98381), (2, 203)):   # 512 workgroups carry the 16 jobs; 4 workgroups do not, and the fold takes its own launch
        case = head_case(K, pixels, False, True)
        s = case[0][0]
        base = run_head(BF, case, table_inputs=True, bn_sums=2, bn_gamma=s["gamma"], da_virtual=True)
        r = run_head(BF, case, table_inputs=True, bn_sums=2, bn_gamma=s["gamma"], da_virtual=True, fold_jobs=jobs)
        assert (r["workgroups"] >= 16) == (pixels > 1000)
        for g, h in zip(r["folds"], want):
            for n in h:
                np.testing.assert_array_equal(g[n], h[n])
        for n in ("logits", "dlogits", "dbias", "dw", "bn_sums", "dgamma", "dbeta", "coef"):
            np.testing.assert_array_equal(r[n], base[n])


def test_head_train_bn_sums_of_an_input_four_deviations_off_zero():
    """The head keeps sum dz*y and sum dz and forms invstd * (sum dz*y - mean * sum dz) afterwards: with a per-channel mean of about four
    standard deviations the two terms cancel.  The bar is 1e-4 of the magnitude of that form (check_head_bn_sums); the error relative to
    sum |dz * xhat| — what a kernel that carried xhat through its loop would be held to — is a property of the design and is printed,
    not asserted.  Observed on an MI355X: 1.15e-9 (CANCELLATION_OBSERVED; a thread of the 512 workgroups adds 3 pixels there)."""
    worst = 0.0
    for K, pixels in ((3, 98381), (4, 203)):
        case = head_case(K, pixels, False, True, sigmas=4.0)
        s = case[0][0]
        assert (np.abs(s["mean"]) * s["invstd"] > 3).all()
        base = run_head(BF, case)
        for kw in (dict(bn_sums=1, bn_mean=s["mean"], bn_invstd=s["invstd"]), dict(table_inputs=True, bn_sums=2, bn_gamma=s["gamma"])):
            r = run_head(BF, case, **kw)
            worst = max(worst, check_head_bn_sums(r, case, True, base["da"]))
    print("head bn sums, input mean at 4 sigma: worst |error| / sum |dz * xhat| = %.3g" % worst)


CANCELLATION_OBSERVED = 1.15e-9   # worst |error of sum dz*xhat| / sum |dz*xhat| in the test above


@pytest.mark.parametrize("precision", [FP, BF])
@pytest.mark.parametrize("pixels", [1, 203, 4099])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_bn_backward_apply_recomputes_da_from_the_dlogits(K, pixels, precision):
    """head form of the apply pass: bit-identical to the plain apply on the da the fused head materialises from the same inputs"""
    bf16 = precision == BF
    case = head_case(K, pixels, False, bf16)
    s, w = case[0][0], case[1]
    h = run_head(precision, case)
    rng = np.random.default_rng(K)
    coef = np.stack([rng.uniform(0.5, 1.5, 32), rng.uniform(-1e-3, 1e-3, 32), rng.uniform(-1e-3, 1e-3, 32)]).astype(np.float32)
    arrays = (s["mean"], s["invstd"], s["scale"], s["shift"])
    plain = aa.op_bn_backward(precision, s["x"], *arrays, da=h["da"], stages=4, coef_in=coef)
    for out_of_place in (False, True):
        head = aa.op_bn_backward(precision, s["x"], *arrays, stages=4, coef_in=coef, head_g=h["dlogits"], head_w_tm=w, out_of_place=out_of_place)
        np.testing.assert_array_equal(head["dy"], plain["dy"])
    dy64, ev = ref.bn_bwd_apply(h["da"], s["x"], *arrays, coef)
    assert (np.abs(plain["dy"] - dy64) <= half_ulp(dy64, bf16) * 1.0001 + ev + TINY).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfused loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", [1, 2047, 2049, 6151])
@pytest.mark.parametrize("K", [3, 5, 8, 9, 64])   # loss_kernel<4>, <8>, <8>, <64>, <64>
def test_loss(K, pixels):
    rng = np.random.default_rng(K * 7 + pixels)
    z = rng.uniform(-30, 30, (pixels, K)).astype(np.float32)
    z[rng.random(pixels) < 0.5 if pixels > 1 else [True]] *= 0.1   # half the pixels undecided (a decided pixel ALONE has max |g| at fp32's resolution of 1 - p: nothing for the atol to scale from)
    labels = rng.integers(0, K, pixels).astype(np.uint16)
    labels[rng.random(pixels) < 0.05] = aa.LABEL_IGNORE
    weights = rng.uniform(0.5, 2.0, pixels).astype(np.float32)
    weights[rng.random(pixels) < 0.1] = 0
    r = aa.op_loss(z, labels, weights, 1.0 / pixels)
    g, loss, dbias, error = ref.softmax_loss(z, labels, weights, 1.0 / pixels)
    assert r["error_flag"] == 0 and not error
    measured("loss dlogits", (np.abs(r["dlogits"] - g) / (2e-3 * np.abs(g) + 2e-5 * np.abs(g).max() + 1e-300)).max())
    measured("loss loss", abs(r["loss"] - loss) / (2e-5 * max(1.0, abs(loss))))
    measured("loss dbias", (np.abs(r["dbias"] - dbias) / (2e-3 * np.abs(dbias) + 2e-5 * np.abs(dbias).max() + 1e-300)).max())
    assert (r["dlogits"][labels == aa.LABEL_IGNORE] == 0).all()
    bad = labels.copy()
    bad[pixels // 2] = K
    rb = aa.op_loss(z, bad, weights, 1.0 / pixels)
    assert rb["error_flag"] == 1 and (rb["dlogits"][pixels // 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer's table life cycle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_passes_without_an_update_leave_the_same_gradients():
    """forward_backward_device twice with no update between: the second pass finds tables that are not clean (sums and tickets of the
    first) and clears them itself.  Both gradient buckets are bit-identical, and equal to a fresh trainer's first pass."""
    import torch
    d = aa.RuntimeNet.GetRecommendedInputDimension(2, 1)
    rng = np.random.default_rng(8)
    n = 2
    img = torch.from_numpy(rng.integers(0, 256, (n, d, d, 3), dtype=np.uint8)).cuda()
    lab_h = rng.integers(0, 3, (n, d, d)).astype(np.uint16)
    lab_h[rng.random((n, d, d)) < 0.05] = aa.LABEL_IGNORE
    lab = torch.from_numpy(lab_h.view(np.int16)).cuda()
    w = torch.from_numpy(rng.uniform(0.5, 2, (n, d, d)).astype(np.float32)).cuda()

    def trainer():
        t = aa.TrainingNet(2, 3, BF, seed=1)
        t.SetNetWidth(1.0, 1); t.SetClassCount(3); t.Initialize()
        return t

    def one_pass(t):
        t.forward_backward_device(img.data_ptr(), lab.data_ptr(), w.data_ptr(), n, d, d, n)
        t.synchronize()
        return t.get_grads(), t.get_last_loss()

    t = trainer()
    g1, l1 = one_pass(t)
    g2, l2 = one_pass(t)
    g3, l3 = one_pass(trainer())
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    np.testing.assert_array_equal(g2, g1)
    np.testing.assert_array_equal(g3, g1)
    assert l1 == l2 == l3
