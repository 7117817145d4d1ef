"""float64 statement of what a training run carries from step to step: the bn running statistics and their update counters
(tests/test_training_run_ref.py, tests/test_gpu_training_run.py).  Plain numpy; nothing here calls the library.

The rule (dlib bn_ as the engine and the oracle read it): per bn layer and training forward, on the STORED raw conv output y [P, c]

    m = sum y / P        var = max(sum y^2 / P - m^2, 0)        unbias = P / (P - 1)  (1 when P = 1)
    af = 1 / (cnt + 1)   then  cnt += 1 while cnt < window
    running_mean = (1 - af) * running_mean + af * m              running_var = (1 - af) * running_var + af * unbias * var

with the update's expression and roundings taken from train_ops_ref.fold (fp32 mean, float64 var, one fp32 rounding of each result).
Past the window the counter stays AT the window, so the steady-state factor is 1 / (window + 1).

THE BAR (derived, not measured).  Unrolled, a running value after S steps is a convex combination

    r_S = w_0 * r_0 + sum_s w_s * x_s,     w >= 0,  sum w = 1,     x_s = m_s  or  unbias_s * var_s

(w_0 = prod (1 - af_s) is 0 as soon as one step had af = 1, i.e. for every run that starts at counter 0).
  * A statistics kernel is held to 2e-5 of the MAGNITUDE sums over the stored tensor (check_forward_sums in test_gpu_train_ops.py):
    |sum y - S1| <= 2e-5 * sum |y| and |sum y^2 - S2| <= 2e-5 * sum y^2.  With A_s = sum |y| / P and Q_s = sum y^2 / P that is
    |dm_s| <= 2e-5 * A_s, and for var = Q - m^2:  |dvar_s| <= 2e-5 * Q_s + 2 |m_s| * |dm_s| = 2e-5 * (Q_s + 2 |m_s| A_s)  (first order).
    A convex combination of values that are each off by at most e_s is off by at most max_s e_s:
        mean:      2e-5 * max_s A_s                      variance:  2e-5 * max_s unbias_s * (Q_s + 2 |m_s| A_s)
  * Roundings: the step's statistic is rounded to fp32 once (2^-24 relative) and the updated value once more (2^-24 relative); an
    error already in the running value is scaled by (1 - af) <= 1 on the way.  Every value involved is bounded by the largest
    magnitude V among r_0 (while its weight is not 0) and the x_s, so S steps add at most  S * 2 * 2^-24 * V = S * 2^-23 * V.
  bar = (statistics term) + S * 2^-23 * V, per element; it is the SAME bar against the oracle (whose sums are float64: the first
  term is then pure slack) and against the device.

Four WRONG rules are switches of the same function (RULES): they are what the tests must refuse.
"""
import numpy as np

import train_ops_ref as ref

F32, F64 = np.float32, np.float64

RIGHT = "right"
WRONG_RULES = ("cap_at_window_minus_1", "cap_at_window_plus_1", "no_cap", "af_one_over_count_plus_2")
RULES = (RIGHT,) + WRONG_RULES

STATS_BAR = 2e-5     # check_forward_sums: a statistics kernel against float64 sums, relative to the magnitude sums
REFUSAL = 10.0       # a wrong rule must miss by at least this many bars


def _cap(rule, window):
    return {"cap_at_window_minus_1": window - 1, "cap_at_window_plus_1": window + 1, "no_cap": np.inf}.get(rule, window)


def averaging_factors(rule, window, steps, counter0=0.0):
    """the factors a rule uses over `steps` updates of one layer, and the counter afterwards"""
    cnt, out = float(counter0), []
    for _ in range(steps):
        out.append(1.0 / (cnt + (2.0 if rule == "af_one_over_count_plus_2" else 1.0)))
        if cnt < _cap(rule, window):
            cnt += 1.0
    return out, cnt


def first_step_a_rule_differs(rule, window, steps, counter0=0.0):
    """1-based index of the first update at which `rule` uses another factor than the right rule (None: never within `steps`)"""
    a, _ = averaging_factors(rule, window, steps, counter0)
    b, _ = averaging_factors(RIGHT, window, steps, counter0)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i + 1
    return None


class Recurrence:
    """result of running_recurrence: .running / .counters / .bar after the last step, .steps[s] = (running, counters, bar) after step s + 1,
    .slices[k] = (mean slice, variance slice) of bn layer k in the blob"""
    def __init__(self, steps, slices):
        self.steps, self.slices = steps, slices
        self.running, self.counters, self.bar = steps[-1]


def running_recurrence(stored, window, running0, counters0=0, rule=RIGHT):
    """stored[s][k]: the raw conv output of bn layer k (in layer order) at step s, any shape [..., c], as stored (TrainingNet.layer_tensor(li, 0),
    OracleNet.layer_output(li, 0)).  running0: the blob before the first step, in the net's layout (rs_off: per bn layer its c means, then
    its c variances; the layers follow each other).  counters0: a number or one per bn layer."""
    assert rule in RULES, rule
    n_bn = len(stored[0])
    run = np.array(running0, dtype=F32).copy()
    cnt = np.broadcast_to(np.asarray(counters0, dtype=F64), (n_bn,)).copy()
    slices, off = [], 0
    for y in stored[0]:
        c = y.shape[-1]
        slices.append((slice(off, off + c), slice(off + c, off + 2 * c)))
        off += 2 * c
    assert off == run.size, (off, run.size)
    stat = np.zeros(run.size, F64)            # max_s of the statistics term
    big = np.abs(run.astype(F64))             # V: largest magnitude involved so far
    w0 = np.ones(n_bn, F64)                   # weight the start value still has
    steps = []
    for s, tensors in enumerate(stored):
        assert len(tensors) == n_bn
        for k, y in enumerate(tensors):
            sm, sv = slices[k]
            y64 = np.asarray(y, F64).reshape(-1, y.shape[-1])
            pixels = y64.shape[0]
            sums = np.stack([y64.sum(0), (y64 * y64).sum(0)], 1)
            unbias = pixels / (pixels - 1.0) if pixels > 1 else 1.0
            af = 1.0 / (cnt[k] + (2.0 if rule == "af_one_over_count_plus_2" else 1.0))
            if cnt[k] < _cap(rule, window):
                cnt[k] += 1.0
            ones = np.ones(y64.shape[1], F32)
            f = ref.fold(sums, pixels, ones, ones, 1e-4, run[sm], run[sv], af=af, unbias=unbias)   # (gamma, beta, eps: not part of the running update)
            a_s, q_s = np.abs(y64).sum(0) / pixels, sums[:, 1] / pixels
            m_s = sums[:, 0] / pixels
            if w0[k] * (1.0 - af) == 0.0 and w0[k] != 0.0:   # the start value leaves the combination
                big[sm], big[sv] = 0.0, 0.0
            w0[k] *= 1.0 - af
            stat[sm] = np.maximum(stat[sm], STATS_BAR * a_s)
            stat[sv] = np.maximum(stat[sv], unbias * STATS_BAR * (q_s + 2.0 * np.abs(m_s) * a_s))
            big[sm] = np.maximum(big[sm], np.abs(m_s))
            big[sv] = np.maximum(big[sv], unbias * f["var"])
            run[sm], run[sv] = f["running_mean"], f["running_var"]
        steps.append((run.copy(), cnt.copy(), stat + (s + 1) * 2.0 ** -23 * big))
    return Recurrence(steps, slices)


def fraction_of_bar(got, want, bar):
    """worst |got - want| / bar over the blob"""
    return float((np.abs(np.asarray(got, F64) - np.asarray(want, F64)) / bar).max())


def refusal(got, wrong, bar, slices):
    """per bn layer (worst miss of a mean, worst miss of a variance) of a wrong rule's blob against the observed one, in bars"""
    miss = np.abs(np.asarray(got, F64) - np.asarray(wrong, F64)) / bar
    return [(float(miss[sm].max()), float(miss[sv].max())) for sm, sv in slices]


def check_run(observed, stored, window, running0, counters0=0):
    """The whole statement of one run: observed[s] is the running blob after step s + 1 (None: not read at that step).  Holds every observed
    blob to the right rule at its bar, and requires every wrong rule to be refused by REFUSAL bars on a mean and a variance of every bn
    layer from the first step at which its factor differs.  Returns (worst fraction of the bar, weakest refusal in bars)."""
    right = running_recurrence(stored, window, running0, counters0)
    worst, weakest = 0.0, np.inf
    wrong = {r: running_recurrence(stored, window, running0, counters0, rule=r) for r in WRONG_RULES}
    c0 = np.broadcast_to(np.asarray(counters0, F64), (len(right.slices),))
    for s, got in enumerate(observed):
        if got is None:
            continue
        want, _, bar = right.steps[s]
        frac = fraction_of_bar(got, want, bar)
        assert frac <= 1.0, ("running statistics off the recurrence", s + 1, frac)
        worst = max(worst, frac)
        for r in WRONG_RULES:
            for k, (dm, dv) in enumerate(refusal(got, wrong[r].steps[s][0], bar, right.slices)):
                since = first_step_a_rule_differs(r, window, len(stored), c0[k])
                if since is not None and s + 1 >= since:
                    assert dm >= REFUSAL and dv >= REFUSAL, ("a wrong rule passes", r, "step", s + 1, "bn layer", k, dm, dv)
                    weakest = min(weakest, dm, dv)
    return worst, weakest


# ---------------------------------------------------------------------------------------------------------------------------------
# the run's mini-batches: statistics that MOVE from step to step, so that the rules are far apart
# ---------------------------------------------------------------------------------------------------------------------------------
LABEL_IGNORE = 65535


def run_batch(step, n, h, w, classes, seed=0, channels=3):
    """mini-batch of step `step` (0-based): pixels drawn from [0, min(32 * (step + 1), 256)) — the input's mean and spread grow with the
    step — and a label mix that leans on class (step mod classes); 5 % of the labels ignored.  -> (images u8 [n,h,w,ch], labels u16 [n,h,w])"""
    rng = np.random.default_rng([seed, step, n, h, w])
    img = rng.integers(0, min(32 * (step + 1), 256), (n, h, w, channels), dtype=np.uint8)
    lean = np.full(classes, 0.4 / max(classes - 1, 1))
    lean[step % classes] = 0.6 if classes > 1 else 1.0
    lab = rng.choice(classes, size=(n, h, w), p=lean / lean.sum()).astype(np.uint16)
    lab[rng.random((n, h, w)) < 0.05] = LABEL_IGNORE
    return img, lab
