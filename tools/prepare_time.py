"""Mean preparation time per decoded image of annonet_train_hip, host against device: generates an anno directory of
`--images` square images with a few hundred labelled blobs each, runs the tool on it twice — default (the loader threads build the
point lists and run both label filters) and --device-sampling (Dataset::Prepare on the resident label image) — and prints the line
each run ends with.

    python tools/prepare_time.py --side 4096 --images 8 --steps 12
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRAIN = os.path.join(ROOT, "annonet_amd", "lib", "annonet_train_hip")


def make_directory(d, images, side, blobs, seed):
    import png_util as pu
    rng = np.random.default_rng(seed)
    for k in range(images):
        lab = np.zeros((side, side), np.uint16)
        for _ in range(blobs):
            h, w = (int(v) for v in rng.integers(side // 64, side // 8, 2))
            y, x = int(rng.integers(0, side - h)), int(rng.integers(0, side - w))
            lab[y:y + h, x:x + w] = rng.integers(1, 3)
        img = (rng.integers(0, 60, (side, side, 3)) + lab[:, :, None] * 80).astype(np.uint8)
        lab[::97, ::89] = 65535
        pu.write_png(os.path.join(d, f"img{k}.png"), img)
        pu.write_png(os.path.join(d, f"img{k}.png_mask.png"), pu.labels_to_rgba(lab))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--blobs", type=int, default=300)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--by-area", type=float, default=30.0)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        os.mkdir(data)
        make_directory(data, a.images, a.side, a.blobs, 1)
        common = [TRAIN, data, "-b", "8", "--net-width-scaler", "0.25", "--net-width-min-filter-count", "4", "--max-total-steps", str(a.steps), "--save-interval", "100000",
                  "--data-loader-thread-count", "4", "--cached-image-count", str(a.images), "--seed", "5", "--ignore-class", "2",
                  "--ignore-large-nonzero-regions-by-area", str(a.by_area)]
        for name, extra in (("host", []), ("device", ["--device-sampling"])):
            r = subprocess.run(common + extra, capture_output=True, text=True, cwd=tmp, timeout=1500)
            if r.returncode != 0:
                sys.exit(f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            print(name + ": " + " ".join(common[2:] + extra))
            for line in r.stdout.splitlines():
                if re.match(r"(steps: |mean preparation time)", line):
                    print("  " + line, flush=True)


if __name__ == "__main__":
    main()
