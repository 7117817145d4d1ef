"""The bars of tests/train_conv_ref.py, proved without a GPU: fp32 emulations of the bf16 training convolutions pass every one of them at
every shape of tests/test_gpu_train_conv.py, and each of a list of subtle kernel mistakes breaks the bar named beside it (a mistake of
the rounding mode breaks exactly the bars listed; a gross local one breaks its element bar first and may move the statistics too).

The emulations take the staged operands of the reference (bf16 values) and accumulate in fp32, in two orders each:
  forward, backward-data   torch's fp32 convolution; and blocks of 16 reduction channels, each block's sum rounded once to fp32 (a matrix-core
                           instruction's k) and added to one fp32 accumulator
  filter gradient          train_conv_ref.seq_filter_grad, one fp32 chain over all pixels in (n, y, x) order (on the accuracy subset); and
                           blocks of 16 pixels, each rounded once, chained in fp32 inside each of 7 splits, the partials then added in order
and store with round to nearest even.  The last test shows what these bars add to the earlier ones of tests/test_gpu_ops.py (one whole
bf16 ulp per element on at most 2 % of the elements; rtol 2e-3 of the largest element): which mistakes those let through.
"""
import ast
import functools

import numpy as np
import pytest

import train_conv_ref as ref
from train_ops_ref import bf16_round

F32, F64 = np.float32, np.float64
S1 = ((0, 3, 1, 1, 32, 32), 2, 21, 37)      # two 32-wide tiles, ragged in both directions, two images, 49728 outputs
UP = ((1, 3, 2, 0, 64, 32), 2, 11, 15)
SPLITS = 7


def truncate_bf16(a):
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def round_half_up_bf16(a):
    """add half a unit of the kept part and cut: differs from nearest-even on exact ties only"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) & 0xFFFF0000).astype(np.uint32).view(F32).reshape(np.shape(a))


STORES = {None: bf16_round, "truncate": truncate_bf16, "half_up": round_half_up_bf16}


def _blocks(c):
    return [slice(i, min(i + 16, c)) for i in range(0, c, 16)]


def emulate_forward(desc, x, filters, bias=None, order="torch", store=None):
    """x: the staged operand (bf16 values) -> the stored tensor"""
    w = ref.filters_q(desc, filters)
    if order == "torch":
        acc = ref.conv_forward(desc, np.asarray(x, F32), w.astype(F32))
    else:
        acc = np.zeros((), F32)
        for b in _blocks(desc[4]):
            part = ref.conv_forward(desc, np.asarray(x, F64)[..., b], w[:, b] if desc[0] == 0 else w[b])
            acc = acc + part.astype(F32)
    if bias is not None:
        return (acc + np.asarray(bias, F32)).astype(F32)     # the head's logits stay fp32
    return STORES[store](acc)


def emulate_backward(desc, dy, filters, in_hw, order="torch", store=None):
    w = ref.filters_q(desc, filters)
    if order == "torch":
        acc = ref.conv_backward(desc, np.asarray(dy, F32), w.astype(F32), in_hw)
    else:
        acc = np.zeros((), F32)
        for b in _blocks(desc[5]):
            part = ref.conv_backward(desc, np.asarray(dy, F64)[..., b], w[b] if desc[0] == 0 else w[:, b], in_hw)
            acc = acc + part.astype(F32)
    return STORES[store](acc)


def emulate_filter_grad(desc, x, dy, drop_last_split=False):
    """blocks of 16 pixels, SPLITS contiguous runs of blocks -> the canonical flat gradient"""
    views = list(ref.tap_views(desc, np.asarray(x, F64), np.asarray(dy, F64)))
    X = np.stack([v[0].reshape(-1, v[0].shape[3]) for v in views])     # [t][P][ci]
    D = np.stack([v[1].reshape(-1, v[1].shape[3]) for v in views])     # [t][P][co]
    P = X.shape[1]
    nb = -(-P // 16)
    per = -(-nb // SPLITS)
    partials = []
    for s in range(SPLITS):
        acc = np.zeros((X.shape[0], X.shape[2], D.shape[2]), F32)
        for b in range(s * per, min((s + 1) * per, nb)):
            px = slice(16 * b, min(16 * b + 16, P))
            acc = acc + np.einsum("tpi,tpo->tio", X[:, px], D[:, px], optimize=True).astype(F32)
        partials.append(acc)
    total = np.zeros_like(partials[0])
    for part in partials[:-1] if drop_last_split else partials:
        total = total + part
    return ref.to_canonical(desc, total)


@functools.lru_cache(maxsize=None)
def fwd_case(i, prologue):
    desc, n, h, w = ref.SHAPES[i]
    xa, kw, filters, rng = ref.make_inputs(desc, n, h, w, 1, prologue)
    bias = rng.uniform(-0.1, 0.1, desc[5]).astype(F32) if desc[1] == 1 else None
    x = ref.staged(xa, **kw)
    return desc, xa, kw, x, filters, bias, ref.forward(desc, x, filters, bias)


@functools.lru_cache(maxsize=None)
def bwd_case(i):
    desc, n, h, w = ref.SHAPES[i]
    _, _, filters, rng = ref.make_inputs(desc, n, h, w, 2, 0)
    dy = ref.make_dy(desc, n, h, w, rng)
    return desc, dy, filters, (h, w), ref.backward_data(desc, dy, filters, (h, w))


@functools.lru_cache(maxsize=None)
def wgrad_case(i, prologue):
    desc, n, h, w = ref.SHAPES[i]
    xa, kw, _, rng = ref.make_inputs(desc, n, h, w, 3, prologue)
    dy = ref.make_dy(desc, n, h, w, rng, 1e-3)
    x = ref.staged(xa, **kw)
    return desc, xa, kw, x, dy, ref.filter_grad(desc, x, dy), ref.seq_filter_grad(desc, x, dy)


def broken(fn, *args, **kw):
    """the bars a check finds broken ([] when it passes)"""
    try:
        fn(*args, **kw)
        return []
    except AssertionError as e:
        text = str(e)
        print(text)
        assert "broken bars: " in text, text
        start = text.index("broken bars: ") + len("broken bars: ")
        return ast.literal_eval(text[start:text.index("]", start) + 1])


# ---- the emulations pass everywhere ----------------------------------------------------------------------------------------------------
STATS_FWD = [i for i, (d, n, h, w) in enumerate(ref.SHAPES) if d[1] != 1 and n * ref.out_dim(d, h) * ref.out_dim(d, w) * d[5] >= 10 ** 4]
STATS_BWD = [i for i, (d, n, h, w) in enumerate(ref.SHAPES) if n * h * w * d[4] >= 10 ** 4]


def test_the_shape_table_claims_statistics_where_the_issue_says():
    big = {ref.SHAPES[i][0] for i in STATS_FWD}
    assert {(0, 5, 1, 2, 3, 32), (0, 3, 1, 1, 32, 32), (0, 3, 1, 1, 64, 64), (0, 3, 1, 1, 128, 128), (0, 3, 2, 0, 32, 64), (0, 3, 2, 0, 64, 128),
            (0, 3, 1, 1, 256, 256), (0, 3, 2, 0, 128, 256), (1, 3, 2, 0, 64, 32)} <= big
    d, n, h, w = ref.SHAPES[5]
    assert d == (0, 3, 2, 0, 64, 128) and n * ref.out_dim(d, h) * ref.out_dim(d, w) * d[5] == 11264
    d, n, h, w = ref.SHAPES[9]
    assert d == (0, 3, 2, 0, 128, 256) and n * ref.out_dim(d, h) * ref.out_dim(d, w) * d[5] == 12288


@pytest.mark.parametrize("order", ["torch", "blocked"])
@pytest.mark.parametrize("prologue", [0, 1, 2])
@pytest.mark.parametrize("i", range(len(ref.SHAPES)))
def test_emulated_forward_passes(i, prologue, order):
    desc, _, _, x, filters, bias, r = fwd_case(i, prologue)
    got = emulate_forward(desc, x, filters, bias, order)
    worst, mean_e, mean_abs, count = ref.check_stored(f"forward p{prologue} {desc}", got, r, stored_bf16=bias is None)
    ref.report(f"forward p{prologue} {order} {desc}", worst, mean_e, mean_abs, count)
    assert worst < 1.0
    assert (count >= ref.MIN_STAT) == (i in STATS_FWD), (count, i)
    if count:
        assert abs(mean_e) < 0.01 and 0.24 < mean_abs < 0.26, (mean_e, mean_abs)


@pytest.mark.parametrize("order", ["torch", "blocked"])
@pytest.mark.parametrize("i", range(len(ref.SHAPES)))
def test_emulated_backward_data_passes(i, order):
    desc, dy, filters, in_hw, r = bwd_case(i)
    q = emulate_backward(desc, dy, filters, in_hw, order)
    worst, mean_e, mean_abs, count = ref.check_stored(f"backward-data {desc}", q, r)
    ref.report(f"backward-data {order} {desc}", worst, mean_e, mean_abs, count)
    assert worst < 1.0
    assert (count >= ref.MIN_STAT) == (i in STATS_BWD), (count, i)
    if count:
        assert abs(mean_e) < 0.01 and 0.24 < mean_abs < 0.26, (mean_e, mean_abs)
    old = bf16_round(np.random.default_rng(6).normal(0, 1, q.shape).astype(F32))
    ref.check_accumulated(f"backward-data into a gradient {desc}", bf16_round(old + q), old, q)


@pytest.mark.parametrize("prologue", [0, 1, 2])
@pytest.mark.parametrize("i", range(len(ref.SHAPES)))
def test_emulated_filter_gradient_passes(i, prologue):
    desc, _, _, x, dy, r, seq = wgrad_case(i, prologue)
    m = seq.shape[1]
    assert seq.size >= min(ref.SUBSET, r["ref"].size)
    # the sequential chain itself, on its subset: the element bar (its rms ratio is 1 by definition)
    sub = dict(ref=r["ref"][:, :m], A=r["A"][:, :m], bound=r["bound"][:, :m])
    assert (np.abs(seq - sub["ref"]) <= sub["bound"]).all()
    worst, ratio = ref.check_filter_grad(f"filter gradient p{prologue} {desc}", desc, emulate_filter_grad(desc, x, dy), r, seq)
    ref.report(f"filter gradient p{prologue} blocked {desc}", worst, rms_ratio=ratio)
    assert worst < 0.05 and ratio < 1.5, (worst, ratio)


@functools.lru_cache(maxsize=None)
def stem_bn_case():
    desc, n, h, w = (0, 5, 1, 2, 3, 32), 3, 21, 43
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    da = bf16_round(rng.normal(0, 1, (n, h, w, 32)).astype(F32))
    y = bf16_round(rng.normal(0, 1, (n, h, w, 32)).astype(F32))
    scale, shift = rng.uniform(0.5, 1.5, 32).astype(F32), rng.uniform(-0.3, 0.3, 32).astype(F32)
    mean, invstd = rng.uniform(-0.2, 0.2, 32).astype(F32), rng.uniform(0.7, 1.4, 32).astype(F32)
    coef = np.concatenate([rng.uniform(0.5, 1.5, 32), rng.uniform(-0.01, 0.01, 32), rng.uniform(-0.01, 0.01, 32)]).astype(F32)
    return desc, img, da, y, scale, shift, mean, invstd, coef


def test_emulated_stem_filter_gradient_with_dy_formed_in_fp32_passes():
    desc, img, da, y, scale, shift, mean, invstd, coef = stem_bn_case()
    x = img.astype(F64) / 256.0
    dyq, flip = ref.stem_dy(da, y, mean, invstd, scale, shift, coef)
    allow = ref.tap_sums(desc, np.abs(x), flip)
    r = ref.filter_grad(desc, x, dyq, allow)
    # the kernel's fp32 expression (chunk_bnbwd), rounded to bf16
    k0, k1, k2 = coef[:32], coef[32:64], coef[64:]
    z = (y.astype(F64) * scale + shift).astype(F32)
    dz = np.where(z > 0, da, F32(0))
    xhat = (y - mean) * invstd
    dy32 = bf16_round(k0 * (dz - k1 - xhat * k2))
    flipped = int((dy32.astype(F64) != dyq).sum())
    assert (np.abs(dy32.astype(F64) - dyq) <= flip).all()      # every difference is one that the allowance names
    seq = ref.seq_filter_grad(desc, x, dyq)
    worst, ratio = ref.check_filter_grad("stem filter gradient, dy in the kernel", desc, emulate_filter_grad(desc, x, dy32), r, seq)
    ref.report(f"stem filter gradient, dy in the kernel ({flipped} of {dyq.size} dy round to the other side)", worst, rms_ratio=ratio)
    assert ratio < 1.5
    # without the allowance the same gradient is held to the plain bars, and a dy that ignores the relu mask breaks them
    bad = bf16_round(k0 * (da - k1 - xhat * k2))
    assert "filter element" in broken(ref.check_filter_grad, "no relu mask", desc, emulate_filter_grad(desc, x, bad), r, seq)


# ---- every mistake breaks a bar ----------------------------------------------------------------------------------------------------------
def s1_forward(prologue):
    return fwd_case(ref.SHAPES.index(S1), prologue)


def padded_forward(desc, x, filters, pad_value=None, mode=None):
    """forward of a stride-1 pad-1 layer with its padding filled by hand"""
    if mode == "edge":
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    else:
        xp = np.empty((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, x.shape[3]), F64)
        xp[:] = pad_value
        xp[:, 1:-1, 1:-1] = x
    return emulate_forward(desc[:3] + (0,) + desc[4:], xp, filters)


def test_truncating_store_breaks_the_element_bar_and_both_rounding_statistics():
    desc, _, _, x, filters, _, r = s1_forward(0)
    assert broken(ref.check_stored, "truncate", emulate_forward(desc, x, filters, store="truncate"), r) == ["element", "rounding bias", "rounding spread"]
    desc, dy, filters, in_hw, r = bwd_case(ref.SHAPES.index(S1))
    assert broken(ref.check_stored, "truncate", emulate_backward(desc, dy, filters, in_hw, store="truncate"), r) == ["element", "rounding bias", "rounding spread"]


def test_round_half_up_store_breaks_the_accumulated_bar():
    """Nearest-even and half-up differ on exact ties only.  An fp32 accumulator of hundreds of terms almost never ties, so the plain store
    cannot show the mistake — but old + q of two bf16 values ties all the time, and there the result is held bit for bit."""
    desc, dy, filters, in_hw, r = bwd_case(ref.SHAPES.index(S1))
    q = emulate_backward(desc, dy, filters, in_hw, store="half_up")
    assert broken(ref.check_stored, "half up", q, r) == []
    old = bf16_round(np.random.default_rng(6).normal(0, 1, q.shape).astype(F32))
    assert broken(ref.check_accumulated, "half up", round_half_up_bf16(old + q), old, q) == ["accumulate"]


def test_bn_padding_left_at_relu_of_shift_breaks_the_element_bar():
    desc, _, kw, x, filters, _, r = s1_forward(1)
    pad = bf16_round(np.maximum(kw["ta"], 0)).astype(F64)
    assert pad.max() > 0
    assert broken(ref.check_stored, "relu(shift) padding", padded_forward(desc, x, filters, pad_value=pad), r)[0] == "element"
    desc, _, kw, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 1)
    xp = np.empty((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, x.shape[3]), F64)
    xp[:] = bf16_round(np.maximum(kw["ta"], 0)).astype(F64)
    xp[:, 1:-1, 1:-1] = x
    got = emulate_filter_grad(desc[:3] + (0,) + desc[4:], xp, dy)
    assert broken(ref.check_filter_grad, "relu(shift) padding", desc, got, r, seq) == ["filter element", "filter rms"]


def test_clamp_to_edge_padding_breaks_the_element_bar():
    desc, _, _, x, filters, _, r = s1_forward(0)
    assert broken(ref.check_stored, "edge padding", padded_forward(desc, x, filters, mode="edge"), r)[0] == "element"


def test_a_halo_column_between_two_tiles_read_as_zero_breaks_the_element_bar():
    desc, _, _, x, filters, _, r = s1_forward(0)
    got = emulate_forward(desc, x, filters).copy()
    cut = np.array(x)
    cut[:, :, 32] = 0                       # the first tile's right halo
    got[:, :, 31] = emulate_forward(desc, cut, filters)[:, :, 31]
    assert broken(ref.check_stored, "halo column", got, r)[0] == "element"


def test_last_ragged_row_or_column_dropped_from_the_filter_gradient_breaks_both_of_its_bars():
    desc, _, _, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 0)
    for axis in (1, 2):
        cut = np.array(dy)
        cut[(slice(None),) * axis + (-1,)] = 0
        assert broken(ref.check_filter_grad, "ragged edge", desc, emulate_filter_grad(desc, x, cut), r, seq) == ["filter element", "filter rms"]


def test_dy_of_the_next_image_on_the_last_row_breaks_both_filter_gradient_bars():
    desc, _, _, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 0)
    wrong = np.array(dy)
    wrong[0, -1] = dy[1, 0]
    assert broken(ref.check_filter_grad, "image boundary", desc, emulate_filter_grad(desc, x, wrong), r, seq) == ["filter element", "filter rms"]


def test_ci_and_co_swapped_in_a_square_layer_breaks_both_filter_gradient_bars():
    desc, _, _, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 0)
    good = ref.to_tm(desc, emulate_filter_grad(desc, x, dy))
    assert broken(ref.check_filter_grad, "ci <-> co", desc, ref.to_canonical(desc, good.transpose(0, 2, 1)), r, seq) == ["filter element", "filter rms"]


def test_last_split_left_out_of_the_reduction_breaks_both_filter_gradient_bars():
    desc, _, _, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 0)
    assert broken(ref.check_filter_grad, "last split", desc, emulate_filter_grad(desc, x, dy, drop_last_split=True), r, seq) == ["filter element", "filter rms"]


def test_skip_sum_rounded_per_side_breaks_the_element_bar():
    desc, xa, kw, _, filters, _, r = s1_forward(2)
    a, b = ref.staged(xa, kw["sa"], kw["ta"]), ref.staged(kw["xb"], kw["sb"], kw["tb"])
    x = bf16_round((a + b).astype(F32)).astype(F64)
    assert "element" in broken(ref.check_stored, "skip per side", emulate_forward(desc, x, filters), r)


def test_mirrored_taps_of_a_transposed_layer_break_the_element_bar():
    desc, _, _, x, filters, _, r = fwd_case(ref.SHAPES.index(UP), 0)
    k = desc[1]
    mirrored = np.asarray(filters).reshape(desc[4], desc[5], k, k)[:, :, ::-1, ::-1].reshape(-1)
    assert "element" in broken(ref.check_stored, "mirrored taps", emulate_forward(desc, x, mirrored), r)


def truncated_prologue(xa, kw):
    z = (np.asarray(xa, F64) * kw["sa"].astype(F64) + kw["ta"].astype(F64)).astype(F32)
    return truncate_bf16(np.maximum(z, F32(0))).astype(F64)


def test_truncated_prologue_operand_breaks_the_forward_and_the_filter_gradient_bars():
    desc, xa, kw, _, filters, _, r = s1_forward(1)
    assert broken(ref.check_stored, "truncated operand", emulate_forward(desc, truncated_prologue(xa, kw), filters), r) == ["element", "rounding bias", "rounding spread"]
    desc, xa, kw, _, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 1)
    assert broken(ref.check_filter_grad, "truncated operand", desc, emulate_filter_grad(desc, truncated_prologue(xa, kw), dy), r, seq) == ["filter element", "filter rms"]


# ---- what the earlier bars let through ---------------------------------------------------------------------------------------------------
def old_ulp_clause(got, want):
    """tests/test_gpu_ops.py::assert_bf16_close, first clause: one whole bf16 ulp per element against the bf16 emulation"""
    ulp = np.abs(want) * 2.0 ** -7 + 1e-30
    return bool((np.abs(got - want) <= ulp * 1.001 + 1e-6 * np.abs(want).max()).all())


def old_fraction_clause(got, want):
    """... second clause: at most 2 % of the elements differ at all"""
    return bool((np.abs(got - want) > 0).mean() <= 0.02)


def old_filter_bar(got, want):
    """tests/test_gpu_ops.py::test_conv_backward_filter: rtol 2e-3, atol 2e-3 of the largest element"""
    return bool(np.allclose(got, want, rtol=2e-3, atol=2e-3 * np.abs(want).max()))


def test_what_the_earlier_bars_let_through():
    # a truncating store stays inside the whole ulp that the old per-element clause allows; only the clause that counts differing
    # elements sees it (half of them differ), and that clause knows nothing of size or sign
    desc, _, _, x, filters, _, _ = s1_forward(0)
    want = emulate_forward(desc, x, filters)
    got = emulate_forward(desc, x, filters, store="truncate")
    assert old_ulp_clause(got, want) and not old_fraction_clause(got, want)
    # a round-half-up store passes both clauses
    desc, dy, filters, in_hw, _ = bwd_case(ref.SHAPES.index(S1))
    q = emulate_backward(desc, dy, filters, in_hw)
    old = bf16_round(np.random.default_rng(6).normal(0, 1, q.shape).astype(F32))
    assert old_ulp_clause(round_half_up_bf16(old + q), bf16_round(old + q))
    # an operand of the one-producer prologue that is 1e-3 low in every term passes the old filter-gradient bar; the accuracy bar sees
    # it a thousand times over.  (The truncated operand is about 3e-3 low and would have tripped the old bar on a few elements in a
    # thousand — had that test ever run the one-producer prologue: it had prologues 0 and 2 only.)
    desc, _, _, x, dy, r, seq = wgrad_case(ref.SHAPES.index(S1), 1)
    low = emulate_filter_grad(desc, x * (1 - 1e-3), dy)
    assert old_filter_bar(low, emulate_filter_grad(desc, x, dy))
    assert broken(ref.check_filter_grad, "operand 1e-3 low", desc, low, r, seq) == ["filter rms"]
