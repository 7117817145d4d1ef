#!/usr/bin/env python3
"""What held-out evaluation costs: windows per second of RuntimeNet.evaluate_device (anh_runtime_evaluate_device) on 32 windows of
227 x 227 x 3, benchmark net, bf16, against anh_runtime_forward_device alone on the same windows in the same forward batches; and the
wall time ONE anh_trainer_evaluate_device call adds to a training run, against the step time of the same session.  Everything is
device-resident, on the C ABI directly, in ONE process and alternating pass by pass: 3 warm-up passes, then the median of 10 timed
passes per form.

  python tools/evaluate_rate.py --out profiles/evaluate_rate.json
      [--windows 32 --side 227]                 the workload
      [--once]                                  one warm-up and one pass of evaluate_device, nothing else: the run to put under
                                                `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/evaluate_rate.py --once`
      [--kernel-stats FILE --timed-results FILE] add the tally kernel's row of that run's *_kernel_stats.csv to a result written
                                                earlier: its time, and (4K + 2 + 4) bytes per pixel / time as a share of 8 TB/s"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
LEVELS, CLASSES, WIDTH = 2, 3, 1.0   # bench.py's net
MAX_BATCH = 16                       # Engine::kMaxTileBatch: evaluate_device cuts its windows into forward batches no larger


def kernel_rows(path, result):
    out = {}
    for row in csv.DictReader(open(path)):
        for name in ("eval_tally_kernel", "eval_finalize_kernel"):
            if name in row["Name"]:
                out[name] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3}
    if "eval_tally_kernel" in out:
        t = out["eval_tally_kernel"]
        per_launch = result["windows"] // max(1, t["calls"] // 2)          # the profiled run makes two calls (--once)
        moved = per_launch * result["side"] ** 2 * (4 * CLASSES + 2 + 4)   # logits, label, weight of every pixel, read once
        t.update({"windows_per_launch": per_launch, "bytes": moved, "bytes_per_s": moved / (t["mean_us"] * 1e-6),
                  "share_of_8TBps": moved / (t["mean_us"] * 1e-6) / HBM_BYTES_PER_S})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=32)
    ap.add_argument("--side", type=int, default=227)
    ap.add_argument("--train-batch", type=int, default=16)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--timed-results")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.timed_results:
        result = json.load(open(a.timed_results))
        result["kernels"] = kernel_rows(a.kernel_stats, result)
        print(json.dumps(result["kernels"]))
        with open(a.out or a.timed_results, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return

    import numpy as np
    import torch

    import annonet_amd as aa
    from annonet_amd._lib import check
    N, S = a.windows, a.side
    assert aa.RuntimeNet.GetRecommendedInputDimension(LEVELS, S) == S, "the side must be an input dimension of the net"
    net = aa.RuntimeNet(aa.net_config(LEVELS, 3, CLASSES, WIDTH, 1, aa.ANH_BF16))
    L = net.L
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    labs = rng.integers(0, CLASSES, (N, S, S)).astype(np.uint16)
    labs[rng.random((N, S, S)) < 0.1] = aa.LABEL_IGNORE
    d_imgs = torch.from_numpy(imgs).cuda()
    d_labs = torch.from_numpy(labs.view(np.int16)).cuda()
    d_w = torch.ones((N, S, S), dtype=torch.float32, device="cuda")
    d_logits = torch.zeros((MAX_BATCH, CLASSES, S, S), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    per_image = np.zeros(N, aa.EVAL_DTYPE)
    confusion = np.zeros((N, CLASSES, CLASSES), np.uint64)
    batches = -(-N // MAX_BATCH)
    per = -(-N // batches)

    def forward_only():
        for first in range(0, N, per):
            check(L.anh_runtime_forward_device(net.h, d_imgs.data_ptr() + first * S * S * 3, min(per, N - first), S, S, d_logits.data_ptr()))
        net.synchronize()

    def evaluate():
        check(L.anh_runtime_evaluate_device(net.h, d_imgs.data_ptr(), d_labs.data_ptr(), d_w.data_ptr(), N, S, S, None, per_image.ctypes.data, confusion.ctypes.data, None))

    if a.once:
        evaluate()
        evaluate()
        return

    # the trainer: a step on --train-batch crops of the same side, and the same evaluation from the trainer's handle
    B = a.train_batch
    t = aa.TrainingNet(LEVELS, 3, aa.ANH_BF16, seed=1)
    t.Initialize()
    t.SetNetWidth(WIDTH, 1)
    t.SetClassCount(CLASSES)
    t.SetLearningRate(0.01)
    samples = list(imgs[:B])
    wl = [aa.set_weights(l, 0.5, 0.5) for l in labs[:B]]

    def train_steps(k=4):
        for _ in range(k):
            t.StartTraining(samples, wl)
        t.synchronize()

    def train_steps_and_evaluate(k=4):
        for _ in range(k):
            t.StartTraining(samples, wl)
        check(t.L.anh_trainer_evaluate_device(t.h, aa.ANH_BF16, d_imgs.data_ptr(), d_labs.data_ptr(), d_w.data_ptr(), N, S, S, None, per_image.ctypes.data,
                                              confusion.ctypes.data, None))
        t.synchronize()

    forms = {"forward_device": forward_only, "evaluate_device": evaluate, "train_4_steps": train_steps, "train_4_steps_and_evaluate": train_steps_and_evaluate}
    times = {name: [] for name in forms}
    for p in range(a.warmups + a.passes):
        for name, fn in forms.items():   # alternating: one pass of every form per round
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if p >= a.warmups:
                times[name].append(dt)
    med = {name: statistics.median(v) for name, v in times.items()}
    result = {"what": "held-out evaluation, benchmark net, bf16, device-resident; median of the timed passes, forms alternating in one process",
              "windows": N, "side": S, "forward_batches": batches, "train_batch": B, "warmups": a.warmups, "passes": a.passes, "pass_seconds": times,
              "forward_device_windows_per_s": N / med["forward_device"], "evaluate_device_windows_per_s": N / med["evaluate_device"],
              "evaluate_over_forward": med["evaluate_device"] / med["forward_device"],
              "evaluate_minus_forward_us": (med["evaluate_device"] - med["forward_device"]) * 1e6,
              "train_step_ms": med["train_4_steps"] / 4 * 1e3,
              "trainer_evaluate_added_ms": (med["train_4_steps_and_evaluate"] - med["train_4_steps"]) * 1e3,
              "mean_loss": float(per_image["loss_sum"].sum() / per_image["weight_sum"].sum()), "counted": int(per_image["counted"].sum())}
    result["trainer_evaluate_added_steps"] = result["trainer_evaluate_added_ms"] / result["train_step_ms"]
    print(json.dumps({k: v for k, v in result.items() if k != "pass_seconds"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
