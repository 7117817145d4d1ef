"""The optimiser step (sgd_kernel) and get_grads (tm_to_canonical_kernel) on their own, against tests/update_ref.py.

A test places ANY gradient it likes: one minimal forward / backward makes the trainer accept an update, then the live gradient bucket
is overwritten (tap-major, through the reference's layout map, with a chosen loss in the trailing slot) and apply_update(scale) runs.
Parameters and momentum are then compared with the float64 reference EXACTLY:

  * dyadic hyperparameters on inputs of confined magnitude: r is the exact real number (asserted), its float32 rounding unique, so
    v' and p' equal the reference on every element;
  * the project's decimal hyperparameters: equality outside the tie-guard set T (update_ref.tie_guard), inside it v' is one of the
    two floats that bracket the midpoint and p' = p + v' for whichever it is.  |T| / n <= 0.5 % is asserted first.  Measured on the
    inputs used here (seed 31), per net in CASE_NETS order:
        lr 0.05, wd 0.0005, mom 0.9, scale 1,   g ~ N(0, 1e-2):  0.093 %, 0.083 %, 0.204 %, 0.063 %
        lr 0.05, wd 0.3,    mom 0.9, scale 1/3, g ~ N(0, 1e-2):  0.276 %, 0.303 %, 0.266 %, 0.313 %
        lr 0.05, wd 0,      mom 0.9, scale 1,   g ~ N(0, 8):     0.078 %, 0.105 %, 0.123 %, 0.097 %
    (with wd = 0 and g ~ N(0, 1e-2) the share is 4.6 %: update_ref.G_SIGMA_DECIMAL says why that set draws larger gradients).

No tolerance appears here other than that guard and its cap.  The case nets cover the 5x5 stem on 1 and 3 channels, 3x3 con at stride
1 and 2, cont layers, the 1x1 head with bias, bn gamma / beta, segment starts inside a 256-thread block and parameter counts that are
no multiple of 256; all are far below 2^24 parameters, which the get_grads test relies on.
"""
import functools

import numpy as np
import pytest

import annonet_amd as aa
import update_ref as ref
from annonet_amd import dist as aad

pytestmark = pytest.mark.gpu

F32 = np.float32
PRECISIONS = [aa.ANH_FP32, aa.ANH_BF16]
CASES = pytest.mark.parametrize("case", ref.CASE_NETS)
PRECS = pytest.mark.parametrize("precision", PRECISIONS, ids=["fp32", "bf16"])
DEFAULT = ref.HYPER_DECIMAL[0]
DYADIC = ref.HYPER_DYADIC[0]


@functools.lru_cache(maxsize=None)
def net(case):
    """(shape, tap-major map, filter mask) of a case net, computed once and left unchanged"""
    shape = ref.net_shape(case)
    assert shape.n_params < 2 ** 24 and shape.n_params % 256 != 0
    tm, _ = ref.layout_maps(shape.layers)
    mask = ref.filter_mask(shape.layers)
    tm.setflags(write=False)
    mask.setflags(write=False)
    return shape, tm, mask


def make_trainer(case, precision, lr, wd, mom):
    levels, in_ch, classes, scaler, minf = case
    t = aa.TrainingNet(levels, in_ch, precision)
    t.SetNetWidth(scaler, minf)
    t.SetClassCount(classes)
    t.Initialize()
    t.SetLearningRate(lr)
    t.set_sgd(wd, mom)
    return t


def device_batch(case, n, side, seed):
    import torch
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, side, side, case[1]), dtype=np.uint8)
    lab = rng.integers(0, case[2], (n, side, side)).astype(np.uint16)
    w = np.stack([aa.set_weights(lab[i], 0.5, 0.5)["weight"] for i in range(n)])
    dev = torch.device("cuda:0")
    return tuple(torch.from_numpy(a).to(dev) for a in (img, lab.view(np.int16), w)) + (n, side)


def step(t, batch):
    img, lab, w, n, side = batch
    t.forward_backward_device(img.data_ptr(), lab.data_ptr(), w.data_ptr(), n, side, side, n)
    t.synchronize()


def place(t, case, g_canonical, loss):
    """overwrite the trainer's gradient bucket: the gradient in tap-major order, the loss in the trailing slot"""
    import torch
    shape, tm, _ = net(case)
    bucket = aad.grad_bucket_tensor(t)
    assert bucket.numel() == shape.n_params + 1
    host = np.append(ref.to_tap_major(np.asarray(g_canonical, dtype=F32), tm), F32(loss))
    bucket.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()      # the copy ran on torch's stream, not the trainer's
    return bucket


def update(case, precision, hyper, p, running, m, g, loss=0.5, trainer=None):
    """one update of (p, m) by the canonical gradient g -> (p', v', trainer)"""
    lr, wd, mom, scale = hyper
    t = trainer if trainer is not None else make_trainer(case, precision, lr, wd, mom)
    t.set_params(p, running)
    t.set_momentum(m)
    step(t, device_batch(case, 1, aa.RuntimeNet.GetRecommendedInputDimension(case[0], 1), 1))
    place(t, case, g, loss)
    t.apply_update(scale)
    t.synchronize()
    return t.get_params()[0], t.get_momentum(), t


def compare(case, hyper, p, m, g, got_p, got_v, guarded):
    _, _, mask = net(case)
    v_ref, p_ref = ref.sgd_ref(p, m, g, mask, *hyper)
    if not guarded:
        np.testing.assert_array_equal(got_v, v_ref)
        np.testing.assert_array_equal(got_p, p_ref)
        return
    T, lo, hi = ref.tie_guard(p, m, g, mask, *hyper)
    print("net %s hyper %s: |T| / n = %d / %d = %.4f %%" % (case, hyper, T.sum(), T.size, 100.0 * T.mean()))
    assert T.mean() <= ref.GUARD_SHARE_CAP
    np.testing.assert_array_equal(got_v[~T], v_ref[~T])
    np.testing.assert_array_equal(got_p[~T], p_ref[~T])
    assert ((got_v[T] == lo) | (got_v[T] == hi)).all()
    np.testing.assert_array_equal(got_p[T], p[T] + got_v[T])


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- a. get_grads ----
@CASES
@PRECS
def test_get_grads_reads_the_bucket_in_canonical_order(case, precision):
    shape, tm, _ = net(case)
    p, running, m, _ = ref.decimal_inputs(shape, 31)
    t = make_trainer(case, precision, 0.05, 0.0005, 0.9)
    t.set_params(p, running)
    step(t, device_batch(case, 1, aa.RuntimeNet.GetRecommendedInputDimension(case[0], 1), 1))
    # bucket[i] = float(i), exact below 2^24: in tap-major order the canonical gradient tm reads 0, 1, 2, ...
    place(t, case, tm.astype(F32), 0.0)
    np.testing.assert_array_equal(t.get_grads(), tm.astype(F32))


# ---- b. dyadic hyperparameters: equality everywhere ----
@CASES
@PRECS
@pytest.mark.parametrize("hyper", ref.HYPER_DYADIC)
def test_update_with_dyadic_hyperparameters_is_exact(case, precision, hyper):
    shape, _, mask = net(case)
    p, running, m, g = ref.dyadic_inputs(shape, ref.DYADIC_SEED)
    assert ref.is_exact(p, m, g, mask, *hyper).all()
    got_p, got_v, _ = update(case, precision, hyper, p, running, m, g)
    compare(case, hyper, p, m, g, got_p, got_v, guarded=False)


# ---- c. the project's decimal hyperparameters ----
@CASES
@PRECS
@pytest.mark.parametrize("hyper,g_sigma", list(zip(ref.HYPER_DECIMAL, ref.G_SIGMA_DECIMAL)))
def test_update_with_decimal_hyperparameters(case, precision, hyper, g_sigma):
    shape, _, _ = net(case)
    p, running, m, g = ref.decimal_inputs(shape, ref.DECIMAL_SEEDS[0], g_sigma)
    got_p, got_v, _ = update(case, precision, hyper, p, running, m, g)
    compare(case, hyper, p, m, g, got_p, got_v, guarded=True)


# ---- d. decay reaches filters only ----
@CASES
@PRECS
def test_decay_reaches_filters_only(case, precision):
    shape, _, _ = net(case)
    p, running, _, _ = ref.decimal_inputs(shape, 31)
    zero = np.zeros(shape.n_params, F32)
    got_p, got_v, _ = update(case, precision, (0.5, 0.25, 0.0, 1.0), p, running, zero, zero)
    for li, kind, start, count in ref.segments(shape.layers):
        sl = slice(start, start + count)
        where = "layer %d %s [%d, %d)" % (li, kind, start, start + count)
        if kind == "filter":
            decay = (F32(-0.125) * p[sl]).astype(F32)      # a power of two: exact
            assert np.array_equal(got_v[sl], decay), where + ": momentum is not -0.125 p"
            assert np.array_equal(got_p[sl], p[sl] + decay), where + ": parameter is not fl32(p + fl32(-0.125 p))"
        else:
            assert np.array_equal(got_p[sl], p[sl]), where + ": decayed, or changed at all"
            assert (got_v[sl] == 0).all(), where + ": momentum is not zero"


# ---- e. tiny step ----
@CASES
@PRECS
def test_tiny_step_leaves_parameters_and_keeps_momentum(case, precision):
    shape, _, mask = net(case)
    hyper = (2.0 ** -30, 2.0 ** -5, 0.0, 1.0)
    p, running, m, _ = ref.decimal_inputs(shape, 31)
    assert (p != 0).all()
    rng = np.random.default_rng(7)
    g = (p * rng.uniform(1.0, 4.0, p.size) * rng.choice([-1.0, 1.0], p.size)).astype(F32)
    # |v'| <= 2^-30 (4 + 2^-5) |p| < 2^-27 |p|: below a quarter of the spacing on either side of p, so p + v' rounds back to p
    assert ref.is_exact(p, m, g, mask, *hyper).all()
    v_ref, p_ref = ref.sgd_ref(p, m, g, mask, *hyper)
    assert np.array_equal(bits(p_ref), bits(p)) and (v_ref != 0).all()
    assert (np.abs(v_ref.astype(np.float64)) < 0.25 * np.spacing(np.abs(p)).astype(np.float64)).all()
    got_p, got_v, _ = update(case, precision, hyper, p, running, m, g)
    np.testing.assert_array_equal(bits(got_p), bits(p))
    np.testing.assert_array_equal(got_v, v_ref)


# ---- f. non-finite gradients stay where they are ----
@CASES
@PRECS
def test_non_finite_gradients_stay_where_they_are(case, precision):
    shape, _, mask = net(case)
    n = shape.n_params
    p, running, m, g = ref.decimal_inputs(shape, 31)
    cont = next(L for L in shape.layers if L.type == 1)
    mid = int(cont.w_off) + (cont.k * cont.k * cont.cin * cont.cout) // 2 + 1
    assert 0 < mid < n - 1
    bad = g.copy()
    bad[0], bad[mid], bad[n - 1] = np.inf, np.nan, -np.inf
    fin_p, fin_v, _ = update(case, precision, DEFAULT, p, running, m, g)
    got_p, got_v, _ = update(case, precision, DEFAULT, p, running, m, bad)
    v_ref, p_ref = ref.sgd_ref(p, m, bad, mask, *DEFAULT)
    assert np.isnan(v_ref[mid]) and v_ref[0] == -np.inf and v_ref[n - 1] == np.inf     # (what the reference says of them)
    for got, want, fin in ((got_v, v_ref, fin_v), (got_p, p_ref, fin_p)):
        assert np.flatnonzero(np.isnan(got)).tolist() == [mid]
        assert got[0] == want[0] == -np.inf and got[n - 1] == want[n - 1] == np.inf
        rest = np.ones(n, bool)
        rest[[0, mid, n - 1]] = False
        np.testing.assert_array_equal(got[rest], fin[rest])


# ---- g. loss slot ----
@PRECS
def test_loss_slot_is_posted_and_steps_are_counted(precision):
    import torch
    case = ref.CASE_NETS[0]
    shape, _, _ = net(case)
    p, running, m, g = ref.dyadic_inputs(shape, ref.DYADIC_SEED)
    _, _, t = update(case, precision, DYADIC, p, running, m, g, loss=0.5)
    assert t.step_count() == 1 and t.get_last_loss() == 0.5
    bucket = aad.grad_bucket_tensor(t)
    for k, loss in enumerate((F32(1.7), F32(-3.1e-5), F32(123456.789))):
        bucket[-1] = float(loss)
        torch.cuda.synchronize()
        t.apply_update(1.0)
        t.synchronize()
        assert t.get_last_loss() == float(loss)
        assert t.step_count() == 2 + k


# ---- h. compute copies follow the update ----
@CASES
@PRECS
def test_compute_copies_follow_the_update(case, precision):
    """Trainer A updates; trainer B is GIVEN A's result (set_params refreshes its compute copies from the master blob).  If A's
    update wrote the four compute-layout copies of what it wrote to the master blob, the next step of both is the same computation:
    gradients and loss equal bit for bit (a step is reproducible run to run, as the trainer-state and crops tests already rely on)."""
    shape, _, _ = net(case)
    p, running, m, g = ref.decimal_inputs(shape, 31)
    new_p, new_v, a = update(case, precision, DEFAULT, p, running, m, g)
    assert not np.array_equal(new_p, p)
    b = make_trainer(case, precision, *DEFAULT[:3])
    b.set_params(new_p, a.get_params()[1])
    b.set_momentum(new_v)
    batch = device_batch(case, 2, aa.RuntimeNet.GetRecommendedInputDimension(case[0], 21), 5)
    step(a, batch)
    step(b, batch)
    bucket_a, bucket_b = (aad.grad_bucket_tensor(t).cpu().numpy() for t in (a, b))
    assert np.isfinite(bucket_a).all() and np.abs(bucket_a[:-1]).max() > 0 and bucket_a[-1] > 0
    np.testing.assert_array_equal(bits(bucket_a), bits(bucket_b))
    if precision == aa.ANH_BF16:
        np.testing.assert_array_equal(bits(a.GetRuntimeNet().get_params()[0]), bits(new_p))


# ---- i. arguments ----
def test_set_sgd_rejects_bad_arguments_and_the_handle_stays_usable():
    case = ref.CASE_NETS[0]
    shape, _, _ = net(case)
    lr, wd, mom, scale = DYADIC
    t = make_trainer(case, aa.ANH_FP32, lr, wd, mom)
    for bad_wd, bad_mom in ((-1e-9, 0.9), (0.0005, -0.1), (0.0005, 1.0)):
        with pytest.raises(aa.AnnonetHipError):
            t.set_sgd(bad_wd, bad_mom)
    # the rejected calls changed nothing: the update runs with the values set before them
    p, running, m, g = ref.dyadic_inputs(shape, ref.DYADIC_SEED)
    got_p, got_v, _ = update(case, aa.ANH_FP32, DYADIC, p, running, m, g, trainer=t)
    compare(case, DYADIC, p, m, g, got_p, got_v, guarded=False)
