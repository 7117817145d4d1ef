#!/usr/bin/env python3
"""Images per second of inference over a folder's worth of equal-sized frames that are one tile each: annonet_infer_batch() at n = 4, 16, 64
images per call against the per-image annonet_infer() loop a caller had before it.  Both forms are measured device-resident (images, label
maps in HBM; one synchronisation per call) and through host arrays (host image in, host label map out), on the C ABI directly, in ONE
process and alternating pass by pass: 3 warm-up passes over all images, then the median of 10 timed passes per form.

  python tools/image_batch_rate.py --out profiles/image_batch_rate.json
      [--images 256 --height 480 --width 640]   the workload (3 channels, benchmark net, bf16)
      [--once N]                                one warm-up and one pass of the device-resident batch form at n = N, nothing else: the run
                                                to put under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/image_batch_rate.py --once 16`
      [--kernel-stats FILE --timed-results FILE] add the rows of that run's *_kernel_stats.csv to a result written earlier: the new
                                                kernel's time and its bytes moved / time as a share of 8 TB/s"""
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


def kernel_rows(path, result):
    h, w, k = result["height"], result["width"], CLASSES
    out = {}
    for row in csv.DictReader(open(path)):
        if "labels_from_logits_kernel" in row["Name"]:
            calls, mean_ns = int(row["Calls"]), float(row["AverageNs"])
            per_image = h * w * (k * 4 + 2)   # the logits read once, the labels written once
            out["labels_from_logits_kernel"] = {"calls": calls, "mean_us": mean_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3, "bytes_per_image": per_image}
            n = result.get("profiled_images_per_call")
            if not n:
                out["labels_from_logits_kernel"]["note"] = "bytes_per_s needs the images per call of the profiled run (--once N)"
            else:
                moved = per_image * n
                out["labels_from_logits_kernel"].update({"bytes": moved, "bytes_per_s": moved / (mean_ns * 1e-9), "share_of_8TBps": moved / (mean_ns * 1e-9) / HBM_BYTES_PER_S})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batches", default="4,16,64")
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--timed-results")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.timed_results:
        result = json.load(open(a.timed_results))
        if a.once:
            result["profiled_images_per_call"] = a.once
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
    N, H, W = a.images, a.height, a.width
    net = aa.RuntimeNet(aa.net_config(LEVELS, 3, CLASSES, WIDTH, 1, aa.ANH_BF16))
    L = net.L
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    ov = aa.lib().anh_required_input_dim(C.byref(net.cfg))
    tp = aa.tiling.parameters(1024, 1024, ov, ov)._c()
    stream = torch.cuda.ExternalStream(net.stream_ptr())
    with torch.cuda.stream(stream):
        d_imgs = torch.from_numpy(imgs).cuda()
        d_labels = torch.zeros((N, H, W), dtype=torch.int16, device="cuda")
        d_planes = torch.zeros((CLASSES, H, W), dtype=torch.float32, device="cuda")
        stream.synchronize()
    labels = np.zeros((N, H, W), np.uint16)
    image_bytes, label_bytes = H * W * 3, H * W * 2

    def device_loop():
        for i in range(N):
            check(L.anh_infer_device(net.h, d_imgs.data_ptr() + i * image_bytes, H, W, None, C.byref(tp), None, 0, d_labels.data_ptr() + i * label_bytes, d_planes.data_ptr()))
        net.synchronize()

    def device_batch(n):
        def run():
            for i in range(0, N, n):
                m = min(n, N - i)
                check(L.anh_infer_batch_device(net.h, d_imgs.data_ptr() + i * image_bytes, m, H, W, None, C.byref(tp), d_labels.data_ptr() + i * label_bytes, None))
            net.synchronize()
        return run

    def host_loop():
        for i in range(N):
            check(L.anh_infer(net.h, imgs[i].ctypes.data, H, W, None, None, C.byref(tp), labels[i].ctypes.data, None))

    def host_batch(n):
        def run():
            for i in range(0, N, n):
                m = min(n, N - i)
                ins = (C.c_void_p * m)(*[imgs[j].ctypes.data for j in range(i, i + m)])
                outs = (C.c_void_p * m)(*[labels[j].ctypes.data for j in range(i, i + m)])
                check(L.anh_infer_batch(net.h, ins, m, H, W, None, None, C.byref(tp), outs, None))
        return run

    if a.once:
        device_batch(a.once)()
        device_batch(a.once)()
        return
    sizes = [int(x) for x in a.batches.split(",")]
    forms = {"device_loop": device_loop, "host_loop": host_loop}
    for n in sizes:
        forms[f"device_batch_{n}"] = device_batch(n)
        forms[f"host_batch_{n}"] = host_batch(n)
    checks = {}
    for name, fn in forms.items():   # every form must leave the same label maps
        labels[:] = 0
        d_labels.zero_()
        torch.cuda.synchronize()
        fn()
        got = labels.copy() if name.startswith("host") else d_labels.cpu().numpy().view(np.uint16)
        checks[name] = int(np.bitwise_xor.reduce(got.reshape(-1).astype(np.uint64) * (np.arange(got.size, dtype=np.uint64) % 65521 + 1)))
    times = {name: [] for name in forms}
    for p in range(a.warmups + a.passes):
        for name, fn in forms.items():   # alternating: one pass of every form per round
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if p >= a.warmups:
                times[name].append(dt)
    result = {"what": "images per second, single-tile frames, benchmark net, bf16; median of the timed passes, forms alternating in one process",
              "images": N, "height": H, "width": W, "warmups": a.warmups, "passes": a.passes, "same_label_maps": len(set(checks.values())) == 1,
              "pass_seconds": times}
    for name in forms:
        med = statistics.median(times[name])
        result[name + "_images_per_s"] = N / med
        result[name + "_ms_per_image"] = med / N * 1e3
    for n in sizes:
        result[f"device_speedup_{n}"] = result[f"device_batch_{n}_images_per_s"] / result["device_loop_images_per_s"]
        result[f"host_speedup_{n}"] = result[f"host_batch_{n}_images_per_s"] / result["host_loop_images_per_s"]
    print(json.dumps({k: v for k, v in result.items() if k != "pass_seconds"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
