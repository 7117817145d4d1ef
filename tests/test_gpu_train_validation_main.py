"""annonet_train_hip --validation-directory: held-out images cut once into windows of the training input dimension on a fixed grid,
evaluated every --validation-interval steps and once after the last step (anh_trainer_evaluate_device).  The final line is rebuilt in
Python from the saved net and grid windows cut in numpy: counts and accuracy exactly, the loss to 1e-6 relative (what %.9g leaves)."""
import os
import re
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "annonet_amd", "lib", "annonet_train_hip")
DIM = 43                                                   # the input dimension of the runs below ("Actual input dimension = 43")
HELD_OUT = ((100, 120), (86, 43), (50, 60))                # sides that are no multiples of 43, and one image that is two whole windows


def write_images(d, sizes, seed):
    rng = np.random.default_rng(seed)
    d.mkdir()
    out = []
    for k, (h, w) in enumerate(sizes):
        lab = np.zeros((h, w), np.uint16)
        for _ in range(8):
            y, x = rng.integers(0, h - 20), rng.integers(0, w - 20)
            lab[y:y + rng.integers(10, 50), x:x + rng.integers(10, 50)] = rng.integers(1, 3)
        img = (rng.integers(0, 60, (h, w, 3)) + (lab[:, :, None] * 80)).astype(np.uint8)
        lab[rng.random((h, w)) < 0.1] = 65535
        pu.write_png(d / f"img{k}.png", img)
        pu.write_png(str(d / f"img{k}.png") + "_mask.png", pu.labels_to_rgba(lab))
        out.append((img, lab))
    return out


def train(cwd, d, *extra):
    return subprocess.run([TRAIN, str(d), "-b", "6", "--net-width-scaler", "0.25", "--net-width-min-filter-count", "4", "--input-dimension-multiplier", "1.2",
                           "--max-total-steps", "6", "--save-interval", "4", "--data-loader-thread-count", "3", "--cached-image-count", "2", "--seed", "5", *extra],
                          capture_output=True, text=True, timeout=900, cwd=cwd)


def grid_windows(held_out):
    """the tool's windows: from (0, 0) with step DIM, clamp-to-edge pixels, "ignore" outside the image"""
    images, labels = [], []
    for img, lab in held_out:
        h, w = lab.shape
        for top in range(0, h, DIM):
            for left in range(0, w, DIM):
                ys, xs = np.arange(top, top + DIM), np.arange(left, left + DIM)
                cy, cx = np.minimum(ys, h - 1), np.minimum(xs, w - 1)
                inside = (ys < h)[:, None] & (xs < w)[None, :]
                images.append(np.ascontiguousarray(img[cy][:, cx]))
                labels.append(np.where(inside, lab[cy][:, cx], 65535).astype(np.uint16))
    return images, labels


def test_validation_lines_and_their_rebuild_from_the_saved_net(tmp_path):
    train_dir, held_dir = tmp_path / "data", tmp_path / "held_out"
    write_images(train_dir, ((160, 200), (140, 150), (200, 170)), 11)
    held_out = write_images(held_dir, HELD_OUT, 12)
    r = train(tmp_path, train_dir, "--validation-directory", str(held_dir), "--validation-interval", "3", "--validation-precision", "fp32")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Actual input dimension = 43" in r.stdout
    images, labels = grid_windows(held_out)
    assert f"validation images: 3, windows of 43 x 43: {len(images)}" in r.stdout and len(images) == 9 + 2 + 4
    lines = re.findall(r"^validation: step (\d+)  images (\d+)  windows (\d+)  loss (\S+)  accuracy (\S+)  mean_iou (\S+)$", r.stdout, flags=re.M)
    rows = re.findall(r"^validation iou per class:((?: \S+)+)$", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [3, 6, 6] and len(rows) == 3, r.stdout       # every 3 steps, and once after the last step
    assert lines[1] == lines[2] and rows[1] == rows[2]
    assert all(l[1] == "3" and int(l[2]) == len(images) for l in lines)
    assert lines[0] != lines[1]                                                      # three more steps changed the weights

    _, _, blob = aa.dnn_envelope_unpack((tmp_path / "annonet.dnn").read_bytes())
    net = aa.RuntimeNet.Deserialize(blob, aa.ANH_FP32)
    wl = []
    for lab in labels:
        a = np.zeros(lab.shape, dtype=aa.netpimpl.WLABEL)
        a["label"], a["weight"] = lab, 1.0
        wl.append(a)
    e = net.evaluate(images, wl)
    counted = sum(int((lab != 65535).sum()) for _, lab in held_out)
    assert int(e.per_image["counted"].sum()) == counted                              # every labelled pixel of every image exactly once
    loss, accuracy, mean_iou = (float(v) for v in lines[2][3:])
    iou = e.class_iou()
    print(f"final line: loss {loss} accuracy {accuracy} mean_iou {mean_iou}; rebuilt: {e.mean_loss():.9g} {e.pixel_accuracy():.9g} {np.nanmean(iou):.9g}")
    assert abs(loss - e.mean_loss()) <= 1e-6 * abs(e.mean_loss())
    assert lines[2][4] == "%.9g" % e.pixel_accuracy()
    assert rows[2].split() == ["%.9g" % v for v in iou]
    assert lines[2][5] == "%.9g" % np.nanmean(iou)


def test_without_the_option_no_validation_line_appears(tmp_path):
    train_dir = tmp_path / "data"
    write_images(train_dir, ((160, 200), (140, 150)), 11)
    r = train(tmp_path, train_dir)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "validation" not in r.stdout and "validation" not in r.stderr
