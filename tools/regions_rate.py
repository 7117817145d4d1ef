#!/usr/bin/env python3
"""What the region table costs: per-image wall time of anh_infer_regions against anh_infer with the same detection levels (the baseline is
code the region table does not touch), and anh_regions_device alone on two synthetic maps with resident planes — many compact blobs, and
one spiral blob (one long chain).  Both forms of the first part alternate in ONE process: 3 warm-up runs, then the median of 10.

  python tools/regions_rate.py --out profiles/regions_rate.json
      [--side 4096]                     the image and the synthetic maps are side x side (benchmark net, bf16, 1024-pixel tiles)
      [--warmups 3 --runs 10]
  ANH_LIBRARY=<libannonet_hip.so of another build>: a build without anh_infer_regions (the parent commit's, tools/ab_bench.py builds
  one) gives the anh_infer figures alone, for a baseline taken from that build itself."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS, CLASSES, WIDTH = 2, 3, 1.0   # bench.py's net


def spiral(h, w):
    """a one-pixel path winding inwards from (0, 0) with one pixel of background between its laps: ONE blob"""
    import numpy as np
    a = np.zeros((h, w), np.uint16)
    i = 0
    while True:
        top, bottom, left, right = i, h - 1 - i, i, w - 1 - i
        if top > bottom or left > right:
            break
        a[top, max(left - 2, 0):right + 1] = 1
        a[top:bottom + 1, right] = 1
        if bottom - top < 2 or right - left < 2:
            break
        a[bottom, left:right + 1] = 1
        a[top + 2:bottom + 1, left] = 1
        i += 2
    return a


def compact_blobs(h, w):
    """12 x 12 squares on a 16-pixel grid, labels 1 and 2 alternating"""
    import numpy as np
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (yy % 16 < 12) & (xx % 16 < 12)
    return np.where(inside, 1 + ((yy // 16 + xx // 16) % 2), 0).astype(np.uint16)


def timed(forms, warmups, runs):
    times = {name: [] for name in forms}
    for i in range(warmups + runs):
        for name, fn in forms.items():   # alternating: one run of every form per round
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i >= warmups:
                times[name].append(dt)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()

    import numpy as np
    import torch

    import annonet_amd as aa
    from annonet_amd import _lib
    from annonet_amd._lib import check
    S = a.side
    net = aa.RuntimeNet(aa.net_config(LEVELS, 3, CLASSES, WIDTH, 1, aa.ANH_BF16))
    L = net.L
    have_regions = hasattr(L, "anh_infer_regions")
    rng = np.random.default_rng(0)
    img = np.kron(rng.integers(0, 256, (S // 16, S // 16, 3)), np.ones((16, 16, 1))).astype(np.uint8)   # blocky: blobs of many sizes
    img = np.clip(img.astype(np.int16) + rng.integers(-20, 21, img.shape), 0, 255).astype(np.uint8)
    ov = aa.lib().anh_required_input_dim(C.byref(net.cfg))
    tp = aa.tiling.parameters(1024, 1024, ov, ov)._c()
    labels, planes = aa.annonet_infer(net, img, tiling_parameters=aa.tiling.parameters(1024, 1024, ov, ov), want_blended=True)
    margins = np.take_along_axis(planes, np.minimum(labels, CLASSES - 1).astype(np.int64)[None], 0)[0] - planes[0]
    det = np.zeros(CLASSES)
    for k in range(1, CLASSES):
        if (labels == k).any():
            det[k] = max(float(np.quantile(margins[labels == k], 0.98)), 1e-6)    # few seeds: most small blobs go
    del planes, margins
    out_labels = np.zeros((S, S), np.uint16)
    result = {"what": "seconds per image, side x side, benchmark net, bf16, 1024-pixel tiles; median of the timed runs, forms alternating in one process",
              "side": S, "warmups": a.warmups, "runs": a.runs, "detection_levels": det.tolist(), "library": os.path.relpath(_lib.LIB_PATH, ROOT), "has_regions": have_regions}

    def infer():
        check(L.anh_infer(net.h, img.ctypes.data, S, S, None, det.ctypes.data, C.byref(tp), out_labels.ctypes.data, None))

    table, rows = C.POINTER(_lib.Region)() if have_regions else None, C.c_size_t()
    region_rows = []

    def infer_regions():
        check(L.anh_infer_regions(net.h, img.ctypes.data, S, S, None, det.ctypes.data, C.byref(tp), out_labels.ctypes.data, None, None, C.byref(table), C.byref(rows)))
        region_rows.append(rows.value)
        L.anh_free(table)

    forms = {"anh_infer": infer}
    if have_regions:
        forms["anh_infer_regions"] = infer_regions
    maps = {}
    for name, fn in forms.items():   # both forms must leave the same label map
        out_labels[:] = 0
        fn()
        maps[name] = out_labels.copy()
    result["same_label_map"] = all((m == maps["anh_infer"]).all() for m in maps.values())
    result["filter_removed_pixels"] = int(((labels != 0) & (maps["anh_infer"] == 0)).sum())
    times = timed(forms, a.warmups, a.runs)
    result["run_seconds"] = times
    for name in forms:
        result[name + "_ms_per_image"] = statistics.median(times[name]) * 1e3
    if have_regions:
        result["regions_of_the_image"] = region_rows[-1]
        result["regions_over_infer"] = result["anh_infer_regions_ms_per_image"] / result["anh_infer_ms_per_image"]

        # anh_regions_device alone, everything resident
        synthetic = {"compact_blobs": compact_blobs(S, S), "spiral": spiral(S, S)}
        d_planes = torch.from_numpy(rng.normal(0, 2, (CLASSES, S, S)).astype(np.float32)).cuda()
        levels = np.array([0.0, 3.0, 4.5])
        device_forms = {}
        counts = {}
        keep = []
        for name, lab in synthetic.items():
            d_lab = torch.from_numpy(lab.view(np.int16)).cuda()
            keep.append(d_lab)

            def run(d_lab=d_lab, name=name):
                check(L.anh_regions_device(net.h, d_lab.data_ptr(), d_planes.data_ptr(), CLASSES, S, S, levels.ctypes.data, 0, None, C.byref(table), C.byref(rows)))
                counts[name] = rows.value
                L.anh_free(table)
            device_forms[name] = run
        torch.cuda.synchronize()
        dt = timed(device_forms, a.warmups, a.runs)
        result["regions_device"] = {name: {"regions": counts[name], "ms_per_call": statistics.median(dt[name]) * 1e3, "run_seconds": dt[name]} for name in device_forms}
    print(json.dumps({k: v for k, v in result.items() if k != "run_seconds"}))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
