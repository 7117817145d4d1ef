#!/usr/bin/env python3
"""Time of scoring on the device, milliseconds per pair of 4096^2 maps with K = 5: anh_score_batch_device (maps resident in HBM) and
anh_score_batch (host maps, uploaded at 2 B per pixel and map), n = 1 and n = 8, on smooth maps (few large regions) and on noise maps
(millions of regions); and annonet_infer() of an image of that size on the same handle, for scale.  Host clock around calls that end in a
device synchronise (every score call waits for its matrices); median and spread of the repeats.  --side / --repeats for a rehearsal."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import annonet_amd as aa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=4096)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default="")
args = ap.parse_args()
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

K, side = 5, args.side
t = aa.TrainingNet(2, 3, aa.ANH_BF16, seed=2)
t.SetNetWidth(1.0, 1); t.SetClassCount(K); t.Initialize()
net = t.GetRuntimeNet(aa.ANH_BF16)     # random-init weights of the BASELINE net
del t
rng = np.random.default_rng(3)


def smooth(seed):
    """classes in large smooth regions: a blurred field at a quarter of the side, quantised and blown up"""
    r = np.random.default_rng(seed)
    q = max(side // 4, 1)
    field = ndimage.gaussian_filter(r.normal(size=(q, q)), 12.0)
    field = (field - field.min()) / max(field.max() - field.min(), 1e-9)
    lab = np.minimum((field * K).astype(np.uint16), K - 1)
    return np.kron(lab, np.ones((side // q, side // q), np.uint16))[:side, :side].copy()


def noise(seed):
    return np.random.default_rng(seed).integers(0, K, (side, side)).astype(np.uint16)


def clock(fn):
    fn()                                   # warm-up of this shape
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


rows = []
for kind, make in (("smooth", smooth), ("noise", noise)):
    for n in (1, 8):
        truths = np.stack([make(100 + i) for i in range(n)])
        results = np.stack([make(200 + i) for i in range(n)])
        results[:, ::7, ::5] = 65535       # some all-NaN pixels
        d_t = torch.from_numpy(truths.view(np.int16)).cuda()
        d_r = torch.from_numpy(results.view(np.int16)).cuda()
        torch.cuda.current_stream().synchronize()
        dev = clock(lambda: aa.score_batch_device(net, d_t.data_ptr(), d_r.data_ptr(), n, K, side, side))
        host = clock(lambda: aa.score_batch(truths, results, K, net=net))
        a = aa.score_batch_device(net, d_t.data_ptr(), d_r.data_ptr(), n, K, side, side)
        b = aa.score_batch(truths, results, K, net=net)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        row = {"maps": kind, "n": n, "side": side, "classes": K,
               "device_ms_per_pair": statistics.median(dev) / n, "device_ms_per_pair_min_max": [min(dev) / n, max(dev) / n],
               "host_maps_ms_per_pair": statistics.median(host) / n, "host_maps_ms_per_pair_min_max": [min(host) / n, max(host) / n],
               "labelled": int(a[2].sum()), "region_votes": int(a[1].sum())}
        row["reupload_ms_per_pair"] = row["host_maps_ms_per_pair"] - row["device_ms_per_pair"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_t, d_r

img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
tp = aa.tiling.parameters(1024, 1024, 35, 35)
infer = clock(lambda: aa.annonet_infer(net, img, tiling_parameters=tp))
row = {"annonet_infer_host_path_ms": statistics.median(infer), "min_max": [min(infer), max(infer)], "side": side}
rows.append(row)
print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
