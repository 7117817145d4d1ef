#!/usr/bin/env python3
"""What batching the regions buys: (1) n single anh_infer_regions calls against ONE anh_infer_regions_batch call over the same n one-tile
frames, both forms alternating in one process (warm-up runs, then the median of the timed runs; the tables of both forms must be the
same bytes); (2) the inference program on a folder of frames of a downscaled net with --write-regions, with and without --image-batch,
and another build's program (the parent commit's) on the same folder: the program's own clock ("actual inference" seconds), the runs of
the variants alternating.

  python tools/regions_batch_rate.py --out profiles/regions_batch_rate.json
      [--frames 8 --height 480 --width 640]       part 1: benchmark net, bf16, one tile per frame
      [--folder-frames 32 --factor 2 --image-batch 8 --tool-runs 3]
      [--other-tool label=path/to/annonet_infer_hip]   part 2: a program of another build, run with --write-regions alone"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LEVELS, CLASSES, WIDTH = 2, 3, 1.0   # bench.py's net


def frames_of(rng, n, h, w):
    """blocky frames with noise: blobs of many sizes"""
    import numpy as np
    out = []
    for _ in range(n):
        img = np.kron(rng.integers(0, 256, ((h + 15) // 16, (w + 15) // 16, 3)), np.ones((16, 16, 1)))[:h, :w]
        out.append(np.clip(img.astype(np.int16) + rng.integers(-20, 21, img.shape), 0, 255).astype(np.uint8))
    return out


def levels_for(aa, net, img, tp):
    """detection levels at the 98th percentile of each class's margins: few seeds, most small blobs go"""
    import numpy as np
    labels, planes = aa.annonet_infer(net, img, tiling_parameters=tp, want_blended=True)
    margins = np.take_along_axis(planes, np.minimum(labels, CLASSES - 1).astype(np.int64)[None], 0)[0] - planes[0]
    det = np.zeros(CLASSES)
    for k in range(1, CLASSES):
        if (labels == k).any():
            det[k] = max(float(np.quantile(margins[labels == k], 0.98)), 1e-6)
    return det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--folder-frames", type=int, default=32)
    ap.add_argument("--factor", type=float, default=2.0)
    ap.add_argument("--image-batch", type=int, default=8)
    ap.add_argument("--tool-runs", type=int, default=3)
    ap.add_argument("--other-tool", action="append", default=[])
    ap.add_argument("--out")
    a = ap.parse_args()

    import numpy as np

    import annonet_amd as aa
    import png_util as pu
    from annonet_amd import _lib
    from annonet_amd._lib import check
    n, H, W = a.frames, a.height, a.width
    net = aa.RuntimeNet(aa.net_config(LEVELS, 3, CLASSES, WIDTH, 1, aa.ANH_BF16))
    L = net.L
    rng = np.random.default_rng(0)
    ov = aa.lib().anh_required_input_dim(C.byref(net.cfg))
    tiling = aa.tiling.parameters(1024, 1024, ov, ov)
    tp = tiling._c()
    imgs = frames_of(rng, n, H, W)
    det = levels_for(aa, net, imgs[0], tiling)
    result = {"what": "part 1: seconds per run over `frames` one-tile frames (benchmark net, bf16), median of the timed runs, forms alternating in one process; "
                      "part 2: the inference program's own 'actual inference' seconds over a folder, median of the runs, variants alternating",
              "frames": n, "height": H, "width": W, "warmups": a.warmups, "runs": a.runs, "detection_levels": det.tolist()}

    # ---- part 1 ----
    labels = [np.zeros((H, W), np.uint16) for _ in range(n)]
    image_ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
    label_ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in labels])
    table, rows, counts = C.POINTER(_lib.Region)(), C.c_size_t(), (C.c_size_t * n)()
    seen = {}

    def single_calls():
        parts = []
        for i in range(n):
            check(L.anh_infer_regions(net.h, imgs[i].ctypes.data, H, W, None, det.ctypes.data, C.byref(tp), labels[i].ctypes.data, None, None, C.byref(table), C.byref(rows)))
            parts.append(C.string_at(table, rows.value * C.sizeof(_lib.Region)))
            L.anh_free(table)
        seen["single_calls"] = (b"".join(parts), b"".join(m.tobytes() for m in labels))

    def batch_call():
        check(L.anh_infer_regions_batch(net.h, image_ptrs, n, H, W, None, det.ctypes.data, C.byref(tp), label_ptrs, None, None, C.byref(table), counts))
        seen["batch_call"] = (C.string_at(table, sum(counts) * C.sizeof(_lib.Region)), b"".join(m.tobytes() for m in labels))
        L.anh_free(table)

    forms = {"single_calls": single_calls, "batch_call": batch_call}
    times = {name: [] for name in forms}
    for i in range(a.warmups + a.runs):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            fn()                                   # every call ends in a device synchronise: the table comes back
            if i >= a.warmups:
                times[name].append(time.perf_counter() - t0)
    result["same_tables_and_maps"] = seen["single_calls"] == seen["batch_call"]
    result["regions_of_the_frames"] = len(seen["batch_call"][0]) // C.sizeof(_lib.Region)
    result["run_seconds"] = times
    for name in forms:
        result[name + "_ms"] = statistics.median(times[name]) * 1e3
    result["batch_over_singles"] = result["batch_call_ms"] / result["single_calls_ms"]

    # ---- part 2 ----
    if a.folder_frames > 0:
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "annonet.dnn"), "wb").write(aa.dnn_envelope_pack("", a.factor, net.Serialize()))
            for i, img in enumerate(frames_of(rng, a.folder_frames, int(H * a.factor), int(W * a.factor))):
                pu.write_png(os.path.join(d, "frame%03d.png" % i), img, filter_type=1)
            mine = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
            variants = {"write_regions": (mine, []), "write_regions_image_batch_%d" % a.image_batch: (mine, ["--image-batch", str(a.image_batch)]),
                        "write_regions_host_resize": (mine, ["--host-resize"]),
                        "write_regions_host_resize_image_batch_%d" % a.image_batch: (mine, ["--host-resize", "--image-batch", str(a.image_batch)])}
            for spec in a.other_tool:
                label, path = spec.split("=", 1)
                variants[label + "_write_regions"] = (os.path.abspath(path), [])
            base = ["--dnn", os.path.join(d, "annonet.dnn"), "--precision", "bf16", "--write-regions", "--full-image-reader-thread-count", "8",
                    "--result-image-writer-thread-count", "8"] + [x for k in range(1, CLASSES) for x in ("-d", "%d:%r" % (k, float(det[k])))]
            seconds = {name: [] for name in variants}
            per_image = {name: [] for name in variants}
            wall = {name: [] for name in variants}      # the program's "processed in": reading and resizing on the CPU threads included
            csvs = {}
            for _ in range(a.tool_runs):
                for name, (tool, extra) in variants.items():
                    r = subprocess.run([tool, d] + base + extra, capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        raise RuntimeError(name + ": " + r.stdout[-2000:] + r.stderr[-2000:])
                    seconds[name].append(float(re.search(r"actual inference: ([0-9.eE+-]+) seconds", r.stdout).group(1)))
                    wall[name].append(float(re.search(r"images processed in ([0-9.eE+-]+) seconds", r.stdout).group(1)))
                    m = re.search(r"excluding the first image: average = ([0-9.eE+-]+) ms", r.stdout)
                    per_image[name].append(float(m.group(1)) if m else None)
                    csvs[name] = b"".join(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".csv") or f.endswith("_result.png"))
            result["tool"] = {"frames": a.folder_frames, "original_size": [int(H * a.factor), int(W * a.factor)], "factor": a.factor, "runs": a.tool_runs,
                              "actual_inference_seconds": seconds, "ms_per_image_after_the_first": per_image,
                              "median_actual_inference_seconds": {k: statistics.median(v) for k, v in seconds.items()},
                              "processed_in_seconds": wall, "median_processed_in_seconds": {k: statistics.median(v) for k, v in wall.items()},
                              "same_files_as_write_regions": {k: v == csvs["write_regions"] for k, v in csvs.items()}}
    print(json.dumps({k: v for k, v in result.items() if k != "run_seconds"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
