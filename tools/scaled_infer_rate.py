#!/usr/bin/env python3
"""Per-image wall time of inference with a downscaled net (factor 2 by default): annonet_infer_scaled() — shrink, infer and blow the
label map up on the GPU — against the form a caller had before it: the host's bilinear, annonet_infer(), the host's nearest neighbour,
on one thread.  Both are builds of tools/scaled_infer_rate.cpp (see there); host array in, host label map out, 3 warm-up images, then the
median of 10.

  python tools/scaled_infer_rate.py --out profiles/scaled_infer_rate.json
      [--baseline-tree DIR]      a checkout of the commit to compare with (its include/ and annonet_amd/host/ are compiled against);
                                 default: this tree (the host path is unchanged by the feature)
      [--baseline-library FILE]  that commit's libannonet_hip.so (default: this tree's)
      [--timed-results FILE]     with --kernel-stats: add the kernel rows to a result this tool wrote earlier, run nothing
      [--kernel-stats FILE]      the *_kernel_stats.csv of `rocprofv3 --kernel-trace --stats -- <build dir>/scaled_new SIDE FACTOR 1 3`
                                 (a run of its own): adds each resize kernel's time and bytes moved / time as a share of 8 TB/s
The two programs run alternately, --rounds times each; the figure of a form is the median of its rounds' medians."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def compile_program(exe, tree, libdir, defines=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", *defines, "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "annonet_amd", "host"),
                           os.path.join(ROOT, "tools", "scaled_infer_rate.cpp"), "-o", exe, "-L" + libdir, "-lannonet_hip", "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lz"])
    return exe


def kernel_rows(path, side, factor):
    """name -> {calls, mean_us, bytes, share_of_8TBps} for the two resize kernels; bytes = source read once + destination written once"""
    sys.path.insert(0, ROOT)
    import annonet_amd as aa
    sh, sw = aa.scaled_dims(side, side, factor)
    moved = {"resize_image_bilinear_kernel": (side * side + sh * sw) * 3, "resize_labels_nearest_kernel": (side * side + sh * sw) * 2}
    out = {}
    for row in csv.DictReader(open(path)):
        for name, nbytes in moved.items():
            if name in row["Name"]:
                mean_ns = float(row["AverageNs"])
                out[name] = {"calls": int(row["Calls"]), "mean_us": mean_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3, "bytes": nbytes,
                             "bytes_per_s": nbytes / (mean_ns * 1e-9), "share_of_8TBps": nbytes / (mean_ns * 1e-9) / HBM_BYTES_PER_S}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--factor", type=float, default=2.0)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--baseline-tree", default=ROOT)
    ap.add_argument("--baseline-library", default=os.path.join(ROOT, "annonet_amd", "lib", "libannonet_hip.so"))
    ap.add_argument("--build-dir", default=os.path.join(ROOT, "build", "scaled_infer_rate"))
    ap.add_argument("--kernel-stats")
    ap.add_argument("--timed-results", help="a JSON this tool wrote: skip the timed runs and only add --kernel-stats to it")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.timed_results:
        result = json.load(open(a.timed_results))
        result["kernels"] = kernel_rows(a.kernel_stats, result["side"], result["factor"])
        print(json.dumps(result["kernels"]))
        with open(a.out or a.timed_results, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    os.makedirs(a.build_dir, exist_ok=True)
    new = compile_program(os.path.join(a.build_dir, "scaled_new"), ROOT, os.path.join(ROOT, "annonet_amd", "lib"), ["-DSCALED_ON_GPU"])
    old = compile_program(os.path.join(a.build_dir, "scaled_baseline"), a.baseline_tree, os.path.dirname(os.path.abspath(a.baseline_library)))
    if a.compile_only:
        return
    args = [str(a.side), repr(a.factor), str(a.warmups), str(a.images)]
    runs = {"baseline": [], "scaled": []}
    for _ in range(a.rounds):
        for name, exe in (("baseline", old), ("scaled", new)):
            r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"{exe} failed ({r.returncode}): {r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, r.stdout.strip(), flush=True)
    result = {"what": "per-image wall time, host array in, host label map out; bf16, 1024-tiles, overlap = one receptive field",
              "side": a.side, "factor": a.factor, "warmups": a.warmups, "images": a.images, "rounds": a.rounds,
              "baseline_tree": os.path.relpath(a.baseline_tree, ROOT), "baseline_library": os.path.relpath(a.baseline_library, ROOT), "runs": runs}
    for name in runs:
        result[name + "_median_ms"] = statistics.median(x["median_ms"] for x in runs[name])
    result["speedup"] = result["baseline_median_ms"] / result["scaled_median_ms"]
    result["same_label_map"] = len({x["label_checksum"] for v in runs.values() for x in v}) == 1
    if a.kernel_stats:
        result["kernels"] = kernel_rows(a.kernel_stats, a.side, a.factor)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
