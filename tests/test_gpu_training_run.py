"""What a training run carries from one step to the next: the bn running statistics with their update counters, and the scratch a
handle keeps between steps.  The loops are in tests/helpers/run_training_run.py; the float64 statement and its bars in
tests/training_run_ref.py (proved on the CPU oracle in tests/test_training_run_ref.py).

(a) Running statistics through and past the window: window 3, 8 steps, two levels, 2-3 samples of 35 x 35 whose statistics move.
    After EVERY step the running blob is held to running_recurrence on the stored conv outputs read back from the handle, at the
    derived bar (training_run_ref: 2e-5 of the magnitude sums + S * 2^-23 of the largest value involved), and each of the four wrong
    rules (cap at window - 1 / window + 1, no cap, 1 / (count + 2)) must be refused by >= 10 bars on a mean and a variance of every
    bn layer from the first step at which its factor differs.  After step 8 the runtime snapshot's forward equals the oracle's with
    the trainer's (params, running), bit for bit.  Every engine-level caller of the update: separate statistics kernel + finalize
    (fp32), fold jobs in the fused head's first workgroups (bf16, 3 classes), bn_fold_all as a launch of the forward (6 classes),
    conv-epilogue partials + finalize (thin bf16 net; ANH_BN_TABLES=0), ANH_FUSE_BN_STATS=0, and the fused head with fewer
    workgroups than fold jobs (ANH_HEAD_BLOCKS=2: its own bn_fold_all launch in backward); the three step entry points, alone and
    alternating on one handle.
(b) A step does not depend on what the handle did before: trainer A walks a list of mini-batch geometries that grows, shrinks and
    grows again; a fresh trainer loaded from A's state reproduces each step bit for bit.
(c) The same through two replicas, whose shard sizes change from step to step.

Worst observed fraction of the derived bar over all steps (the bar is 1), and the weakest refusal of a wrong rule in bars (the
requirement is 10), per configuration on an MI355X; `pytest -s` prints them, the assertions are the bars and not these figures:
    fp32 (0.25, 4), statistics kernel + finalize                      0.0042     45
    bf16 (1.0, 1) 3 classes, tables folded in the fused head          0.0044    117
    bf16 (1.0, 1) 6 classes, tables folded by bn_fold_all             0.0048     81
    bf16 (0.25, 4), no tables                                         0.0039     44
    bf16 (1.0, 1) ANH_BN_TABLES=0                                     0.0044    117
    bf16 (1.0, 1) ANH_BN_TABLES=0 ANH_FUSE_BN_STATS=0                 0.0049    118
    bf16 (1.0, 1) ANH_HEAD_BLOCKS=2                                   0.0044    117
    bf16 (1.0, 1) crops / device / alternating entry points           0.0044    117   (bit-identical to StartTraining)
    fp32 two replicas, replica 0 on its shard (6 steps)               0.0042      -
The statistics term of the bar (2e-5 of the magnitude sums) is what the kernels' own tests allow a summation; sums kept in double
or in integer tables use a thousandth of it, so what is observed is the fp32 roundings of the update against S * 2^-23.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import annonet_amd as aa
import training_run_ref as run
from helpers import run_training_run as loop
from oracle.oracle import set_weights as oracle_set_weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

_runs = {}


def default_run(config, entries=("host",)):
    """one in-process run per (configuration, entry points), shared by the tests that compare with it and left unchanged"""
    key = (config, entries)
    if key not in _runs:
        _runs[key] = loop.stats_run(config, entries)
    return _runs[key]


def child_run(tmp_path, what, config, env, name):
    out = str(tmp_path / (name + ".npz"))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "run_training_run.py"), what, config, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def check_stats(out, name):
    """(a)'s assertions on what one run read back"""
    stored = loop.stored_of(out)
    assert len(stored) == loop.STEPS and min(y.reshape(-1, y.shape[-1]).shape[0] for y in stored[0]) > 1     # more than one pixel per channel everywhere
    assert np.isfinite(out["losses"]).all()
    assert all(run.first_step_a_rule_differs(r, loop.WINDOW, loop.STEPS) is not None for r in run.WRONG_RULES)   # every wrong rule gets its turn
    worst, weakest = run.check_run(list(out["running"]), stored, loop.WINDOW, out["running0"])
    print("measured %-28s %.3g of the bar (worst of %d steps); weakest refusal of a wrong rule %.3g bars" % (name, worst, loop.STEPS, weakest))
    np.testing.assert_array_equal(out["logits"], out["oracle_logits"])
    return [str(x) for x in out["order"]]


def test_fp32_separate_statistics_kernel_and_finalize():
    out = default_run("fp32")
    order = check_stats(out, "fp32")
    assert "bn_forward_stats" in order and "bn_forward_finalize" in order and "bn_fold_all" not in order
    # ... and the oracle stepped alongside with the same window, at the bars of test_fp32_multi_step_training_tracks_oracle
    o = loop.oracle_net("fp32")
    o.params[:], o.running[:] = loop.random_params(o, 11)
    o.set_hyper(lr=0.05, wd=0.0005, mom=0.9, bn_window=loop.WINDOW)
    for s in range(loop.STEPS):
        img, lab = run.run_batch(s, 2 + s % 2, loop.SIDE, loop.SIDE, 3)
        want = o.train_step(img, lab, np.stack([oracle_set_weights(l, 0.5, 0.5) for l in lab]))
        assert abs(out["losses"][s] - want) <= 1e-3 * max(1.0, abs(want))
        np.testing.assert_allclose(out["running"][s], o.running, rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(out["params"], o.params, rtol=2e-3, atol=2e-5)
    assert o.running_updates.tolist() == [float(loop.WINDOW)] * len(o.running_updates)


def test_bf16_tables_folded_inside_the_fused_head():
    order = check_stats(default_run("bf16"), "bf16 tables, head folds")
    assert "head_fused_fwd_loss_bwd" in order and "bn_fold_all" not in order and "bn_forward_finalize" not in order


def test_bf16_tables_folded_by_a_launch_of_the_forward():
    order = check_stats(default_run("bf16_k6"), "bf16 tables, bn_fold_all")
    assert "bn_fold_all" in order and "softmax_logloss" in order and "bn_forward_finalize" not in order


def test_bf16_channel_counts_the_table_mode_refuses():
    order = check_stats(default_run("bf16_thin"), "bf16 thin net, no tables")
    assert "bn_forward_finalize" in order and "bn_fold_all" not in order


@pytest.mark.parametrize("name,env", [
    ("partials_with_finalize", {"ANH_BN_TABLES": "0"}),
    ("separate_statistics_kernel", {"ANH_BN_TABLES": "0", "ANH_FUSE_BN_STATS": "0"}),
    ("head_with_fewer_workgroups_than_fold_jobs", {"ANH_HEAD_BLOCKS": "2"}),
])
def test_bf16_schedule_switches(tmp_path, name, env):
    order = check_stats(child_run(tmp_path, "stats", "bf16", env, name), "bf16 " + name)
    if name == "head_with_fewer_workgroups_than_fold_jobs":
        # 2 workgroups < one fold job per bn layer: the jobs cannot ride in the head kernel, backward launches bn_fold_all itself
        assert len(loop.bn_layers("bf16")) > 2 and "head_fused_fwd_loss_bwd" in order and "bn_forward_finalize" not in order
    else:
        assert "bn_forward_finalize" in order and "bn_fold_all" not in order
        if name == "separate_statistics_kernel":
            assert "bn_forward_stats" in order


@pytest.mark.parametrize("entries", [("crops",), ("device",), ("host", "crops", "device")], ids=["crops", "device", "alternating"])
def test_the_window_reaches_the_engine_on_every_step_entry_point(entries):
    """StartTraining, StartTrainingOnCrops and forward_backward_device + apply_update on the same mini-batches: the recurrence holds on
    each, and the counters of one handle do not depend on which entry point made a step — the three runs the same kernels on the same
    data, so the running blobs of every step are those of the StartTraining run bit for bit"""
    out = default_run("bf16", entries)
    check_stats(out, "bf16 " + "+".join(entries))
    want = default_run("bf16")
    np.testing.assert_array_equal(out["running"], want["running"])
    np.testing.assert_array_equal(out["params"], want["params"])
    np.testing.assert_array_equal(out["losses"], want["losses"])


# ---------------------------------------------------------------------------------------------------------------------------------
# (b), (c): changing mini-batch geometry on one handle
# ---------------------------------------------------------------------------------------------------------------------------------
def head_train_blocks(pixels):
    """kernels_generic.hip head_train_blocks: rows of the head's partial sums"""
    return max(1, min((pixels * 4 + 255) // 256, 512))


def bn_partial_blocks(pixels):
    """kernels_generic.hip bn_partial_blocks: rows of a statistics pass's partial sums"""
    ppb = min(max(((pixels + 1023) // 1024 + 63) // 64 * 64, 256), 4096)
    return (pixels + ppb - 1) // ppb


TWO_REPLICA_GEOMETRY = [(n if n >= 2 else 2, h, w) for n, h, w in loop.GEOMETRY]


def test_the_geometry_list_changes_every_row_count_between_neighbours():
    """a later edit of the sizes must not hollow (b) and (c) out: full-resolution pixel counts 3675, 8925, 4690, 4489, 7350, 3675"""
    pixels = [n * h * w for n, h, w in loop.GEOMETRY]
    assert pixels == [3675, 8925, 4690, 4489, 7350, 3675]
    assert [head_train_blocks(p) for p in pixels] == [58, 140, 74, 71, 115, 58]
    assert [bn_partial_blocks(p) for p in pixels] == [15, 35, 19, 18, 29, 15]
    for lst in (pixels, [n // 2 * h * w for n, h, w in TWO_REPLICA_GEOMETRY]):     # (replica 0's shard: samples [0, n / 2))
        for a, b in zip(lst, lst[1:]):
            assert head_train_blocks(a) != head_train_blocks(b) and bn_partial_blocks(a) != bn_partial_blocks(b)
    assert pixels[1] > pixels[0] and pixels[2] < pixels[1] and pixels[4] > pixels[3] and loop.GEOMETRY[-1] == loop.GEOMETRY[0]     # grows, shrinks, grows again
    assert any(n == 1 for n, _, _ in loop.GEOMETRY) and any(h > w for _, h, w in loop.GEOMETRY) and any(w > h for _, h, w in loop.GEOMETRY)
    assert all(n >= 2 for n, _, _ in TWO_REPLICA_GEOMETRY)


def check_geometry(out, steps, fields=("params", "momentum", "running", "loss", "lr", "steps")):
    for k in range(2, steps + 1):
        for f in fields:
            np.testing.assert_array_equal(out["b_%s_%d" % (f, k)], out["a_%s_%d" % (f, k)], err_msg="%s after step %d" % (f, k))
    assert int(out["a_steps_%d" % steps]) == steps
    assert all(np.isfinite(out["a_loss_%d" % k]) for k in range(1, steps + 1))
    assert np.abs(out["a_params_%d" % steps] - out["a_params_1"]).max() > 0


@pytest.mark.parametrize("config", ["fp32", "bf16"])
def test_a_step_does_not_depend_on_what_the_handle_did_before(tmp_path, config):
    check_geometry(loop.geometry_run(config, str(tmp_path / "state.dat")), len(loop.GEOMETRY))


def test_a_step_does_not_depend_on_what_the_handle_did_before_without_tables(tmp_path):
    check_geometry(child_run(tmp_path, "geometry", "bf16", {"ANH_BN_TABLES": "0"}, "geometry_partials"), len(loop.GEOMETRY))


def test_two_replicas_on_changing_shard_sizes(tmp_path):
    aa.set_devices([0, 0])
    try:
        out = loop.geometry_run("fp32", str(tmp_path / "state.dat"), TWO_REPLICA_GEOMETRY, replicas=2)
    finally:
        aa.set_devices([])
    steps = len(TWO_REPLICA_GEOMETRY)
    for k in range(1, steps + 1):
        np.testing.assert_array_equal(out["r0_%d" % k], out["r1_%d" % k], err_msg="replicas apart after step %d" % k)
        np.testing.assert_array_equal(out["r0_%d" % k], out["a_params_%d" % k])
    check_geometry(out, steps)     # (running: replica 0's, the one the state file carries)
    # replica 0's running statistics follow the recurrence on replica 0's stored tensors, which are its shard
    stored = loop.stored_of(out)
    for k, (n, h, w) in enumerate(TWO_REPLICA_GEOMETRY):
        lo, hi = aa.shard_range(n, 2, 0)
        assert stored[k][0].shape[:3] == (hi - lo, h, w)
    right = run.running_recurrence(stored, loop.WINDOW, out["running0"])
    worst = max(run.fraction_of_bar(out["running"][s], right.steps[s][0], right.steps[s][2]) for s in range(steps))
    print("measured %-28s %.3g of the bar (worst of %d steps)" % ("fp32 two replicas, replica 0", worst, steps))
    assert worst <= 1.0
    assert right.counters.tolist() == [float(loop.WINDOW)] * len(right.slices)
