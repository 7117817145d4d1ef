"""The float64 statement of the running statistics (tests/training_run_ref.py) proved on the CPU oracle, with no GPU.

An OracleNet with a window of 3 trains 8 steps on mini-batches whose statistics move (training_run_ref.run_batch), plain and under
the bf16 storage emulation.  From the oracle's OWN stored conv outputs the recurrence must reproduce the oracle's running blob within
the derived bars and its update counters exactly; each of the four wrong rules must miss the blob by at least 10 bars on a mean and a
variance of EVERY bn layer — at the end of the run and at every step from the first one at which the rule's factor differs.  The GPU
tests (tests/test_gpu_training_run.py) put the library's tensors through the same check_run on the same mini-batches."""
import numpy as np
import pytest

import training_run_ref as run
from conftest import random_params
from oracle.oracle import OracleNet, set_weights

WINDOW, STEPS = 3, 8


def oracle_run(levels, scaler, minf, bf16, classes=3):
    o = OracleNet(levels, 3, classes, scaler, minf)
    p, r = random_params(o, 11)
    o.params[:], o.running[:] = p, r
    o.set_hyper(lr=0.05, wd=0.0005, mom=0.9, bn_window=WINDOW)
    if bf16:
        o.set_bf16_emulation(True)
    d = o.recommended_input_dim(33)
    bn = [li for li, L in enumerate(o.layers) if L.has_bn]
    stored, observed, counters = [], [], []
    for s in range(STEPS):
        img, lab = run.run_batch(s, 2 + s % 2, d, d, classes)
        o.train_step(img, lab, np.stack([set_weights(l, 0.5, 0.5) for l in lab]))
        stored.append([o.layer_output(li, 0) for li in bn])
        observed.append(o.running.copy())
        counters.append(o.running_updates.copy())
    return o, r, stored, observed, counters


@pytest.mark.parametrize("bf16", [False, True], ids=["plain", "bf16_emulation"])
@pytest.mark.parametrize("levels,scaler,minf", [(1, 0.25, 4), (2, 0.25, 4), (2, 1.0, 1)])
def test_recurrence_reproduces_the_oracle_and_refuses_every_wrong_rule(levels, scaler, minf, bf16):
    o, r0, stored, observed, counters = oracle_run(levels, scaler, minf, bf16)
    right = run.running_recurrence(stored, WINDOW, r0)
    for s in range(STEPS):
        np.testing.assert_array_equal(right.steps[s][1], counters[s])
    assert right.counters.tolist() == [float(WINDOW)] * len(right.slices)     # the cap engaged: 8 steps, window 3
    for L, (sm, sv) in zip([L for L in o.layers if L.has_bn], right.slices):  # the blob's layout is the net's
        assert (sm.start, sv.start, sv.stop) == (L.rs_off, L.rs_off + L.cout, L.rs_off + 2 * L.cout)
    worst, weakest = run.check_run(observed, stored, WINDOW, r0)
    print("measured oracle levels %d width (%g, %d) %s: %.3g of the bar; weakest refusal of a wrong rule %.3g bars" %
          (levels, scaler, minf, "bf16" if bf16 else "fp32", worst, weakest))
    # every wrong rule is refused at the end of the run, on every bn layer (check_run asserted it from the rule's first differing step on)
    for rule in run.WRONG_RULES:
        assert run.first_step_a_rule_differs(rule, WINDOW, STEPS) is not None
        wrong = run.running_recurrence(stored, WINDOW, r0, rule=rule)
        for dm, dv in run.refusal(o.running, wrong.running, right.bar, right.slices):
            assert dm >= run.REFUSAL and dv >= run.REFUSAL, (rule, dm, dv)
        if rule != "af_one_over_count_plus_2":
            assert wrong.counters.tolist() != right.counters.tolist()


def test_the_rules_factors():
    """the switches state what their names say (window 3): the right rule settles at 1 / (window + 1)"""
    af = lambda rule: run.averaging_factors(rule, 3, 7)
    assert af(run.RIGHT) == ([1, 1 / 2, 1 / 3, 1 / 4, 1 / 4, 1 / 4, 1 / 4], 3)
    assert af("cap_at_window_minus_1") == ([1, 1 / 2, 1 / 3, 1 / 3, 1 / 3, 1 / 3, 1 / 3], 2)
    assert af("cap_at_window_plus_1") == ([1, 1 / 2, 1 / 3, 1 / 4, 1 / 5, 1 / 5, 1 / 5], 4)
    assert af("no_cap") == ([1, 1 / 2, 1 / 3, 1 / 4, 1 / 5, 1 / 6, 1 / 7], 7)
    assert af("af_one_over_count_plus_2") == ([1 / 2, 1 / 3, 1 / 4, 1 / 5, 1 / 5, 1 / 5, 1 / 5], 3)
    assert [run.first_step_a_rule_differs(r, 3, 8) for r in run.WRONG_RULES] == [4, 5, 5, 1]
    assert run.first_step_a_rule_differs("cap_at_window_plus_1", 3, 4) is None


def test_a_single_pixel_layer_and_a_start_value_that_stays():
    """P = 1: unbias is 1 and the variance 0; a counter that starts above 0 keeps the start value in the combination (and in the bar)"""
    y = [[np.array([[2.0, -4.0]], np.float32)], [np.array([[4.0, 0.0]], np.float32)]]
    r0 = np.array([1.0, 1.0, 0.5, 0.5], np.float32)
    got = run.running_recurrence(y, 3, r0, counters0=1)
    np.testing.assert_array_equal(got.counters, [3.0])
    # af = 1/2 then 1/3:  mean ((1 + 2) / 2) * 2/3 + 4/3 = 7/3 ; ((1 - 4) / 2) * 2/3 + 0 = -1 ; var 0.5 * 1/2 * 2/3 = 1/6
    np.testing.assert_allclose(got.running, [7 / 3, -1.0, 1 / 6, 1 / 6], rtol=1e-6)
    assert (got.bar[:2] >= 2 * 2.0 ** -23 * 4.0).all() and (got.bar[2:] >= 2 * 2.0 ** -23 * 0.5).all()
