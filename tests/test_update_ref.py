"""The optimiser reference of tests/update_ref.py, held to account without a GPU: its layout maps against indices written out by
hand, its update against the CPU oracle, and the share of elements its tie guard excuses against a cap."""
from types import SimpleNamespace

import numpy as np
import pytest

import update_ref as ref
from oracle.oracle import OracleNet, IGNORE

F32 = np.float32


@pytest.mark.parametrize("case", ref.CASE_NETS)
def test_layout_maps_are_bijections(case):
    shape = ref.net_shape(case)
    assert ref.param_count(shape.layers) == shape.n_params
    tm, km = ref.layout_maps(shape.layers)
    mask = ref.filter_mask(shape.layers)
    ident = np.arange(shape.n_params)
    for name, mp in (("tap-major", tm), ("k-major", km)):
        assert np.array_equal(np.sort(mp), ident), name
        assert np.array_equal(mp[~mask], ident[~mask]), name      # bias, gamma, beta map to themselves
        for _, kind, start, count in ref.segments(shape.layers):  # a segment maps onto itself
            assert mp[start:start + count].min() == start and mp[start:start + count].max() == start + count - 1, (name, kind, start)
    # the segments tile the blob without gaps or overlaps
    pos = 0
    for _, _, start, count in ref.segments(shape.layers):
        assert start == pos
        pos += count
    assert pos == shape.n_params
    # the case nets do hold what the GPU tests count on: both filter orders, a biased head, and a ragged last block
    assert {L.type for L in shape.layers} == {0, 1} and shape.layers[-1].has_bias and shape.n_params < 2 ** 24


def hand_layer(type_):
    # 2 input channels, 3 output channels, 3x3: 54 filter elements, then 3 of bias
    return SimpleNamespace(type=type_, k=3, stride=1, pad=1, cin=2, cout=3, has_bn=0, has_bias=1, w_off=0, b_off=54, g_off=0, beta_off=0)


def test_layout_maps_of_a_con_layer_by_hand():
    """canonical [co][ci][t] -> tap-major (t * 2 + ci) * 3 + co and k-major (t * 3 + co) * 2 + ci, one row per (co, ci)"""
    tm, km = ref.layout_maps([hand_layer(0)])
    want_tm = [0, 6, 12, 18, 24, 30, 36, 42, 48,      # co 0, ci 0
               3, 9, 15, 21, 27, 33, 39, 45, 51,      # co 0, ci 1
               1, 7, 13, 19, 25, 31, 37, 43, 49,      # co 1, ci 0
               4, 10, 16, 22, 28, 34, 40, 46, 52,     # co 1, ci 1
               2, 8, 14, 20, 26, 32, 38, 44, 50,      # co 2, ci 0
               5, 11, 17, 23, 29, 35, 41, 47, 53,     # co 2, ci 1
               54, 55, 56]                            # bias
    want_km = [0, 6, 12, 18, 24, 30, 36, 42, 48,
               1, 7, 13, 19, 25, 31, 37, 43, 49,
               2, 8, 14, 20, 26, 32, 38, 44, 50,
               3, 9, 15, 21, 27, 33, 39, 45, 51,
               4, 10, 16, 22, 28, 34, 40, 46, 52,
               5, 11, 17, 23, 29, 35, 41, 47, 53,
               54, 55, 56]
    assert tm.tolist() == want_tm
    assert km.tolist() == want_km


def test_layout_maps_of_a_cont_layer_by_hand():
    """canonical [ci][co][t] -> the same two targets, one row per (ci, co)"""
    tm, km = ref.layout_maps([hand_layer(1)])
    want_tm = [0, 6, 12, 18, 24, 30, 36, 42, 48,      # ci 0, co 0
               1, 7, 13, 19, 25, 31, 37, 43, 49,      # ci 0, co 1
               2, 8, 14, 20, 26, 32, 38, 44, 50,      # ci 0, co 2
               3, 9, 15, 21, 27, 33, 39, 45, 51,      # ci 1, co 0
               4, 10, 16, 22, 28, 34, 40, 46, 52,     # ci 1, co 1
               5, 11, 17, 23, 29, 35, 41, 47, 53,     # ci 1, co 2
               54, 55, 56]
    want_km = [0, 6, 12, 18, 24, 30, 36, 42, 48,
               2, 8, 14, 20, 26, 32, 38, 44, 50,
               4, 10, 16, 22, 28, 34, 40, 46, 52,
               1, 7, 13, 19, 25, 31, 37, 43, 49,
               3, 9, 15, 21, 27, 33, 39, 45, 51,
               5, 11, 17, 23, 29, 35, 41, 47, 53,
               54, 55, 56]
    assert tm.tolist() == want_tm
    assert km.tolist() == want_km


def test_to_tap_major_places_a_canonical_value_where_the_map_says():
    tm, _ = ref.layout_maps([hand_layer(1)])
    canon = np.arange(57, dtype=F32) + 100
    bucket = ref.to_tap_major(canon, tm)
    assert bucket[3] == 100 + 27 and bucket[tm[40]] == 140     # tap-major 3 = (t 0, ci 1, co 0) = canonical (1 * 3 + 0) * 9 + 0
    np.testing.assert_array_equal(bucket[tm], canon)


@pytest.mark.parametrize("case", ref.CASE_NETS)
@pytest.mark.parametrize("hyper", [ref.HYPER_DECIMAL[0], ref.HYPER_DECIMAL[1][:3] + (1.0,)])
def test_reference_equals_the_oracle_update(case, hyper):
    """The oracle's update (annonet_oracle.cpp, `upd`) is the SAME double expression, in the same order — mom * m - wd * lr * p - lr * g,
    wd = 0.0 outside the filters, rounded once to float32, then a float32 `+=` — and the oracle is compiled with -ffp-contract=off, so it
    rounds every product as numpy does.  (The oracle has no grad_scale: scale = 1 here, where lr * (g * 1) = lr * g exactly.)  Equality is
    therefore demanded on EVERY element, tie-guard set included."""
    lr, wd, mom, scale = hyper
    o = OracleNet(*case)
    shape = ref.net_shape(case)
    assert shape.n_params == o.n_params
    p, running, m, _ = ref.decimal_inputs(shape, 17)
    o.params[:], o.running[:], o.momentum[:] = p, running, m
    o.set_hyper(lr=lr, wd=wd, mom=mom, bn_window=100)
    rng = np.random.default_rng(3)
    d = o.recommended_input_dim(1)
    img = rng.integers(0, 256, (2, d, d, case[1]), dtype=np.uint8)
    lab = rng.integers(0, case[2], (2, d, d)).astype(np.uint16)
    lab[rng.random(lab.shape) < 0.05] = IGNORE
    w = rng.uniform(0.5, 1.5, lab.shape).astype(F32)
    o.train_step(img, lab, w, apply_update=False)
    g = o.grads.copy()
    np.testing.assert_array_equal(o.params, p)
    np.testing.assert_array_equal(o.momentum, m)
    assert np.abs(g).max() > 0
    o.train_step(img, lab, w)
    np.testing.assert_array_equal(o.grads, g)       # the step is deterministic: the update used these gradients
    v_ref, p_ref = ref.sgd_ref(p, m, g, ref.filter_mask(shape.layers), lr, wd, mom, scale)
    np.testing.assert_array_equal(o.momentum, v_ref)
    np.testing.assert_array_equal(o.params, p_ref)


def test_tie_guard_finds_a_planted_tie_and_nothing_else():
    # A float32 input cannot itself be a float32 midpoint, so the tie comes from the momentum coefficient: m = 1 and mom = 1 - 2^-25
    # give r = 1 - 2^-25, exactly between the floats 1 - 2^-24 and 1 (the spacing below 1 is 2^-24)
    p = np.zeros(4, F32)
    m = np.array([1.0, 1.0, 0.75, -1.0], F32)
    g = np.array([0.0, 2.0 ** -30, 0.0, 0.0], F32)
    mask = np.zeros(4, bool)
    mom = 1.0 - 2.0 ** -25
    T, lo, hi = ref.tie_guard(p, m, g, mask, 1.0, 0.0, mom, 1.0)
    assert T.tolist() == [True, False, False, True]
    assert lo.tolist() == [float(F32(1.0 - 2.0 ** -24)), -1.0] and hi.tolist() == [1.0, float(-F32(1.0 - 2.0 ** -24))]
    v, _ = ref.sgd_ref(p, m, g, mask, 1.0, 0.0, mom, 1.0)
    assert v[0] in (lo[0], hi[0]) and v[3] in (lo[1], hi[1])


@pytest.mark.parametrize("case", ref.CASE_NETS)
@pytest.mark.parametrize("hyper,g_sigma", list(zip(ref.HYPER_DECIMAL, ref.G_SIGMA_DECIMAL)))
def test_guard_share_of_the_gpu_inputs_stays_under_the_cap(case, hyper, g_sigma):
    """A condition on the inputs of tests/test_gpu_update.py, not a measurement: a guard that excused more than 0.5 % of the elements
    could hide a kernel that is wrong there."""
    shape = ref.net_shape(case)
    for seed in ref.DECIMAL_SEEDS:
        p, _, m, g = ref.decimal_inputs(shape, seed, g_sigma)
        T, _, _ = ref.tie_guard(p, m, g, ref.filter_mask(shape.layers), *hyper)
        print("net %s hyper %s seed %d: |T| / n = %d / %d = %.4f %%" % (case, hyper, seed, T.sum(), T.size, 100.0 * T.mean()))
        assert T.mean() <= ref.GUARD_SHARE_CAP


@pytest.mark.parametrize("case", ref.CASE_NETS)
@pytest.mark.parametrize("hyper", ref.HYPER_DYADIC)
def test_dyadic_inputs_make_the_update_exact(case, hyper):
    """the premise of the equality-everywhere GPU test: r is the exact real number, so its float32 rounding is unique"""
    shape = ref.net_shape(case)
    p, _, m, g = ref.dyadic_inputs(shape, ref.DYADIC_SEED)
    mask = ref.filter_mask(shape.layers)
    assert ref.is_exact(p, m, g, mask, *hyper).all()
