#!/usr/bin/env python3
"""Images per second of downscaled inference over a folder's worth of equal-sized camera frames that are one tile each at the net's
resolution: annonet_infer_scaled_batch() at n = 4, 16, 64 images per call against the per-image annonet_infer_scaled() loop a caller
had before it.  Every form is measured device-resident (originals and original-size label maps in HBM; one synchronisation per pass) and
through host arrays (host image in, host label map out), on the C ABI directly.

The baseline loop comes from a library built from the PARENT commit, never from the build under test: a child process started with
ANH_LIBRARY=<that library> (as tools/ab_bench.py selects a build) measures the two loop forms; a second child on the build under test
measures its own loop forms and the batch forms, alternating pass by pass in one process.  The two children alternate for --rounds
rounds; every child runs 3 warm-up passes over all images and then its share of the --passes timed passes per form, and a form's figure
is the median over all its timed passes.

  python tools/scaled_batch_rate.py --baseline-library annonet_amd/lib_parent/libannonet_hip.so --out profiles/scaled_batch_rate.json
      [--images 256 --height 960 --width 1280 --factor 2]   the workload (3 channels, benchmark net, bf16)
      [--once N]                                 one warm-up and one pass of the device-resident batch form at n = N, nothing else: the run
                                                 to put under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/scaled_batch_rate.py --once 16`
      [--kernel-stats FILE --timed-results FILE] add the rows of that run's *_kernel_stats.csv to a result written earlier: the two
                                                 batched resizes' time and their bytes moved / time as a share of 8 TB/s"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
LEVELS, CLASSES, WIDTH = 2, 3, 1.0   # bench.py's net


def scaled_side(n, factor):
    return int((1.0 / factor) * n + 0.5)


def kernel_rows(path, result):
    h, w, f = result["height"], result["width"], result["factor"]
    small = scaled_side(h, f) * scaled_side(w, f)
    per_image = {"resize_image_bilinear_kernel": (h * w + small) * 3, "resize_labels_nearest_kernel": (small + h * w) * 2}   # source read once, destination written once
    n = result.get("profiled_images_per_call")
    out = {}
    for row in csv.DictReader(open(path)):
        for kernel, nbytes in per_image.items():
            if kernel in row["Name"]:
                calls, mean_ns = int(row["Calls"]), float(row["AverageNs"])
                entry = {"calls": calls, "mean_us": mean_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3, "bytes_per_image": nbytes}
                if n:
                    moved = nbytes * n
                    entry.update({"bytes": moved, "bytes_per_s": moved / (mean_ns * 1e-9), "share_of_8TBps": moved / (mean_ns * 1e-9) / HBM_BYTES_PER_S})
                else:
                    entry["note"] = "bytes_per_s needs the images per call of the profiled run (--once N)"
                out[kernel] = entry
    return out


def child(a):
    """the forms this process's library has, alternating pass by pass: prints {"pass_seconds": {form: [...]}, "checksums": {form: ...}}"""
    import numpy as np
    import torch

    import annonet_amd as aa
    from annonet_amd._lib import check
    N, H, W, F = a.images, a.height, a.width, a.factor
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
        stream.synchronize()
    labels = np.zeros((N, H, W), np.uint16)
    image_bytes, label_bytes = H * W * 3, H * W * 2

    def device_loop():
        for i in range(N):
            check(L.anh_infer_scaled_device(net.h, d_imgs.data_ptr() + i * image_bytes, H, W, F, None, C.byref(tp), d_labels.data_ptr() + i * label_bytes, None, None))
        net.synchronize()

    def host_loop():
        for i in range(N):
            check(L.anh_infer_scaled(net.h, imgs[i].ctypes.data, H, W, F, None, None, C.byref(tp), labels[i].ctypes.data, None, None))

    def device_batch(n):
        def run():
            for i in range(0, N, n):
                m = min(n, N - i)
                check(L.anh_infer_scaled_batch_device(net.h, d_imgs.data_ptr() + i * image_bytes, m, H, W, F, None, C.byref(tp), d_labels.data_ptr() + i * label_bytes, None, None))
            net.synchronize()
        return run

    def host_batch(n):
        def run():
            for i in range(0, N, n):
                m = min(n, N - i)
                ins = (C.c_void_p * m)(*[imgs[j].ctypes.data for j in range(i, i + m)])
                outs = (C.c_void_p * m)(*[labels[j].ctypes.data for j in range(i, i + m)])
                check(L.anh_infer_scaled_batch(net.h, ins, m, H, W, F, None, None, C.byref(tp), outs, None, None))
        return run

    if a.once:
        device_batch(a.once)()
        device_batch(a.once)()
        return
    forms = {"device_loop": device_loop, "host_loop": host_loop}
    if hasattr(L, "anh_infer_scaled_batch"):   # (the parent commit's library has the loop forms only)
        for n in [int(x) for x in a.batches.split(",")]:
            forms[f"device_batch_{n}"] = device_batch(n)
            forms[f"host_batch_{n}"] = host_batch(n)
    checks = {}
    for name, fn in forms.items():   # every form must leave the same label maps
        labels[:] = 0
        d_labels.zero_()
        torch.cuda.synchronize()
        fn()
        got = labels if name.startswith("host") else d_labels.cpu().numpy().view(np.uint16)
        checks[name] = zlib.crc32(np.ascontiguousarray(got).reshape(-1).view(np.uint8))
    times = {name: [] for name in forms}
    for p in range(a.warmups + a.passes):
        for name, fn in forms.items():   # alternating: one pass of every form per round
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if p >= a.warmups:
                times[name].append(dt)
    print("CHILD " + json.dumps({"pass_seconds": times, "checksums": checks, "gpu": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--factor", type=float, default=2.0)
    ap.add_argument("--batches", default="4,16,64")
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--passes", type=int, default=10, help="timed passes per form, over all rounds")
    ap.add_argument("--rounds", type=int, default=2, help="how often the two builds' processes alternate")
    ap.add_argument("--baseline-library", help="libannonet_hip.so built from the parent commit")
    ap.add_argument("--commit", help="the build under test's commit, where the tree is not a git checkout (default: git rev-parse HEAD)")
    ap.add_argument("--baseline-commit", help="the commit the baseline library was built from")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
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
    if a.child or a.once:
        child(a)
        return
    if not a.baseline_library or not os.path.exists(a.baseline_library):
        sys.exit("--baseline-library: the library built from the parent commit is needed (the per-image loop is never taken from the build under test)")
    per_child = -(-a.passes // a.rounds)
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--images", str(a.images), "--height", str(a.height), "--width", str(a.width), "--factor", repr(a.factor),
            "--batches", a.batches, "--warmups", str(a.warmups), "--passes", str(per_child)]
    env_under_test = {k: v for k, v in os.environ.items() if k != "ANH_LIBRARY"}
    builds = {"parent": dict(env_under_test, ANH_LIBRARY=os.path.abspath(a.baseline_library)), "this": env_under_test}
    times, checks, gpu = {}, {}, None
    for r in range(a.rounds):
        for build, env in builds.items():   # the two builds alternate
            out = subprocess.run(argv, env=env, capture_output=True, text=True)
            line = [l for l in out.stdout.splitlines() if l.startswith("CHILD ")]
            if out.returncode != 0 or not line:
                sys.exit(f"the {build} build's run failed:\n" + out.stdout[-2000:] + out.stderr[-3000:])
            got = json.loads(line[-1][6:])
            gpu = got["gpu"]
            for name, secs in got["pass_seconds"].items():
                times.setdefault(f"{build}_{name}", []).extend(secs)
                checks[f"{build}_{name}"] = got["checksums"][name]
            print(build, "round", r, {k: round(statistics.median(v), 4) for k, v in got["pass_seconds"].items()}, flush=True)
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    N = a.images
    result = {"what": "images per second of downscaled inference, single-tile frames at the net's resolution, benchmark net, bf16; median of the timed passes; "
                      "parent_*: the per-image loop on a library built from the parent commit; this_*: the build under test, its forms alternating in one process",
              "commit": commit or None, "baseline_commit": a.baseline_commit,
              "gpu": gpu, "images": N, "height": a.height, "width": a.width, "factor": a.factor, "warmups": a.warmups, "passes_per_form": per_child * a.rounds,
              "rounds": a.rounds, "same_label_maps": len(set(checks.values())) == 1, "pass_seconds": times}
    for name, secs in times.items():
        med = statistics.median(secs)
        result[name + "_images_per_s"] = N / med
        result[name + "_ms_per_image"] = med / N * 1e3
    for n in [int(x) for x in a.batches.split(",")]:
        result[f"device_speedup_{n}"] = result[f"this_device_batch_{n}_images_per_s"] / result["parent_device_loop_images_per_s"]
        result[f"host_speedup_{n}"] = result[f"this_host_batch_{n}_images_per_s"] / result["parent_host_loop_images_per_s"]
    result["loop_this_over_parent_device"] = result["this_device_loop_images_per_s"] / result["parent_device_loop_images_per_s"]
    result["loop_this_over_parent_host"] = result["this_host_loop_images_per_s"] / result["parent_host_loop_images_per_s"]
    print(json.dumps({k: v for k, v in result.items() if k != "pass_seconds"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
