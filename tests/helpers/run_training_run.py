"""The loops of tests/test_gpu_training_run.py: what a training run carries from one step to the next.

The test module calls stats_run / geometry_run directly for the library's default schedule.  The kernel-schedule switches are
environment variables read once per process, so every other variant runs this file as a child with the switch in its environment;
the child runs the SAME loop and saves what it read to an .npz, and the parent asserts on it.

usage: python tests/helpers/run_training_run.py stats|geometry <config> <out.npz>       (config: a key of CONFIGS)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import annonet_amd as aa  # noqa: E402
import training_run_ref as run  # noqa: E402
from conftest import random_params  # noqa: E402
from oracle.oracle import OracleNet  # noqa: E402

LEVELS, WINDOW, STEPS, SIDE = 2, 3, 8, 35     # 35 = 2 * 16 + 3: the smallest valid side for two levels
#                 precision    width      classes
CONFIGS = {
    "fp32":      (aa.ANH_FP32, (0.25, 4), 3),   # separate statistics kernel + finalize
    "bf16":      (aa.ANH_BF16, (1.0, 1), 3),    # accumulator tables, fold jobs inside the fused head kernel
    "bf16_k6":   (aa.ANH_BF16, (1.0, 1), 6),    # tables, bn_fold_all as a launch of the forward (no fused head above 4 classes)
    "bf16_thin": (aa.ANH_BF16, (0.25, 4), 3),   # channel counts the table mode refuses
}
# (n, h, w) per step: grows, shrinks and grows again, rectangular both ways, one sample, back to the first geometry
GEOMETRY = [(3, 35, 35), (5, 51, 35), (2, 35, 67), (1, 67, 67), (6, 35, 35), (3, 35, 35)]


def oracle_net(config):
    _, (scaler, minf), classes = CONFIGS[config]
    return OracleNet(LEVELS, 3, classes, scaler, minf)


def bn_layers(config):
    return [li for li, L in enumerate(oracle_net(config).layers) if L.has_bn]


def make_trainer(config, seed=5, given_params=True):
    """the reference's call order (annonet_train_main.cpp:400-410); the net of tests/test_training_run_ref.py (random_params, seed 11)"""
    precision, (scaler, minf), classes = CONFIGS[config]
    t = aa.TrainingNet(LEVELS, 3, precision, seed=seed)
    t.Initialize()
    t.SetNetWidth(scaler, minf)
    t.SetClassCount(classes)
    t.SetLearningRate(0.05)
    t.SetLearningRateShrinkFactor(0.5)
    t.SetIterationsWithoutProgressThreshold(6)
    t.SetPreviousLossValuesDumpAmount(2)
    t.SetAllBatchNormalizationRunningStatsWindowSizes(WINDOW)
    if given_params:
        t.set_params(*random_params(oracle_net(config), 11))
    return t


def host_batch(step, n, h, w, classes):
    img, lab = run.run_batch(step, n, h, w, classes)
    return img, lab, [aa.set_weights(l, 0.5, 0.5) for l in lab]


class Stepper:
    """one mini-batch through one of the three step entry points of a handle"""
    def __init__(self, t):
        self.t, self.ds, self.keep = t, None, None

    def host(self, img, lab, wl):
        self.t.StartTraining(list(img), wl)

    def crops(self, img, lab, wl):
        """the same samples as whole-image crops of a device-resident dataset (no flip, gain 1: the crop IS the image; the weights
        are cut on the device with the same class / image weight)"""
        if self.ds is None:
            self.ds = aa.Dataset(3)
        idx = [self.ds.add(i, l) for i, l in zip(img, lab)]
        self.t.StartTrainingOnCrops(self.ds, [(i, 0, 0, 0, 0, 1.0) for i in idx], img.shape[1], 0.5, 0.5)

    def device(self, img, lab, wl):
        import torch
        n, h, w = lab.shape
        self.t.synchronize()    # (the tensors of the step before may go now)
        self.keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (img, lab.view(np.int16), np.stack([x["weight"] for x in wl]))]
        torch.cuda.synchronize()
        self.t.forward_backward_device(*(a.data_ptr() for a in self.keep), n, h, w, n)
        self.t.apply_update(1.0)


def stats_run(config, entries=("host",)):
    """8 steps, window 3, 2-3 samples of 35 x 35 whose statistics move; step s goes through entries[s % len(entries)].
    -> dict: y_<s>_<k> the stored raw conv output of bn layer k after step s, running [S, n_running] the running blob after each step,
    running0, params (after the last step), losses, order (the last step's launch names), logits / oracle_logits (the runtime snapshot
    and the oracle with the trainer's parameters on one image)"""
    classes = CONFIGS[config][2]
    t = make_trainer(config)
    stepper = Stepper(t)
    bn = bn_layers(config)
    out = {"running0": t.get_params()[1]}
    running, losses = [], []
    for s in range(STEPS):
        if s == STEPS - 1:
            t.profile_enable(True)
        getattr(stepper, entries[s % len(entries)])(*host_batch(s, 2 + s % 2, SIDE, SIDE, classes))
        losses.append(t.get_last_loss())
        for k, li in enumerate(bn):
            out["y_%d_%d" % (s, k)] = t.layer_tensor(li, 0)
        running.append(t.get_params()[1])
    out["order"] = np.array(t.profile_launch_order())
    t.profile_enable(False)
    assert t.step_count() == STEPS
    p, r = t.get_params()
    img = np.random.default_rng(77).integers(0, 256, (1, SIDE, SIDE, 3), dtype=np.uint8)
    o = oracle_net(config)
    o.params[:], o.running[:] = p, r
    out.update(running=np.stack(running), losses=np.array(losses), params=p, logits=t.GetRuntimeNet(aa.ANH_FP32).Forward(img), oracle_logits=o.forward(img))
    return out


def stored_of(out):
    n_bn = len([k for k in out if k.startswith("y_0_")])
    return [[out["y_%d_%d" % (s, k)] for k in range(n_bn)] for s in range(len(out["running"]))]


def state_of(t):
    p, r = t.get_params()
    return dict(params=p, running=r, momentum=t.get_momentum(), loss=np.float64(t.get_last_loss()), lr=np.float64(t.GetLearningRate()), steps=np.int64(t.step_count()))


def geometry_run(config, state_path, geometry=GEOMETRY, replicas=1):
    """Trainer A walks the geometry list; before every step k >= 2 it saves its state, a FRESH trainer B_k (another seed, its own
    initial parameters: everything must come from the file) loads it and runs only step k.
    -> dict: a_<field>_<k> / b_<field>_<k> of state_of after step k (k from 1; b from 2), r0_<k> / r1_<k> the replicas' parameters,
    y_<k-1>_<j> replica 0's stored tensors, running / running0 as in stats_run"""
    classes = CONFIGS[config][2]
    a = make_trainer(config)
    bn = bn_layers(config)
    out = {"running0": a.get_params()[1]}
    running = []
    for k, (n, h, w) in enumerate(geometry, start=1):
        batch = host_batch(100 + k, n, h, w, classes)
        if k >= 2:
            a.save_state(state_path)
            b = make_trainer(config, seed=99, given_params=False)
            b.load_state(state_path)
            b.StartTraining(list(batch[0]), batch[2])
            for f, v in state_of(b).items():
                out["b_%s_%d" % (f, k)] = v
            del b
        a.StartTraining(list(batch[0]), batch[2])
        for f, v in state_of(a).items():
            out["a_%s_%d" % (f, k)] = v
        for r in range(replicas if replicas > 1 else 0):
            out["r%d_%d" % (r, k)] = a.replica_params(r)
        for j, li in enumerate(bn):
            out["y_%d_%d" % (k - 1, j)] = a.layer_tensor(li, 0)
        running.append(out["a_running_%d" % k])
    out["running"] = np.stack(running)
    return out


def main():
    what, config, path = sys.argv[1:4]
    out = stats_run(config) if what == "stats" else geometry_run(config, path + ".state")
    np.savez(path, **out)


if __name__ == "__main__":
    main()
