"""annonet_infer_hip --write-regions together with --image-batch and with the GPU resize of a downscaled net: the PNGs and the CSVs are,
byte for byte, those of --write-regions alone and of --write-regions --host-resize, and the groups really run as batches."""
import os
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
import resize_util as ru
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
K = 3
OV = 35   # TrainingNet::GetRequiredInputDimension() of the tool's build (2 levels)
HEADER = "class_index,class_name,left,top,right,bottom,area,seeds,peak,downscaling_factor="
FRAME, OTHER = (60, 80), (50, 50)
# equal-sized frames and one of another size between them: groups of 2, 1 and 3 at --image-batch 3
NAMES = [("f1.png", FRAME), ("f2.png", FRAME), ("f3.png", OTHER), ("f4.png", FRAME), ("f5.png", FRAME), ("f6.png", FRAME)]
TIMING_LINE = "Processing time excluding the first image"      # printed when images came after the first image, or after the first BATCH


@pytest.fixture(scope="module")
def net():
    p, r = random_params(OracleNet(2, 3, K, 0.25, 4), 21)
    n = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    n.set_params(p, r)
    return n


def tp():
    return aa.tiling.parameters(96, 96, OV, OV)


def make_frames(d, net, factor, names):
    d.mkdir()
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", factor, net.Serialize()))
    rng = np.random.default_rng(17)
    images = {}
    for name, (h, w) in names:
        images[name] = rng.integers(0, 256, (int(h * factor), int(w * factor), 3), dtype=np.uint8)
        pu.write_png(d / name, images[name], filter_type=1)
    return images


def levels_for(net, img):
    """detection levels at the median blob peak of each class: some blobs are detected, some are not"""
    _, table = aa.annonet_infer_regions(net, img, tiling_parameters=tp())
    det = [0.0] * K
    for k in range(1, K):
        peaks = table["peak"][(table["label"] == k) & np.isfinite(table["peak"])]
        if len(peaks):
            det[k] = float(np.median(peaks.astype(np.float64))) + 1e-3
    return det


def run_tool(d, det, names, *extra):
    """stdout, {name: (png bytes, csv bytes)}; the outputs are removed again"""
    args = [TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "-w", "96", "-h", "96", "--precision", "fp32", "--full-image-reader-thread-count", "1", "--write-regions"]
    for k in range(1, K):
        args += ["-d", "%d:%r" % (k, det[k])]
    r = subprocess.run(args + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "All %d images processed" % len(names) in r.stdout and "All result images written!" in r.stdout
    out = {}
    for name, _ in names:
        files = [str(d / name) + "_result.png", str(d / name) + "_result_regions.csv"]
        out[name] = tuple(open(f, "rb").read() for f in files)
        for f in files:
            os.remove(f)
    return r.stdout, out


@pytest.mark.parametrize("factor", [1.0, 2.0])
def test_write_regions_with_image_batch_writes_the_same_files(tmp_path, net, factor):
    d = tmp_path / "frames"
    images = make_frames(d, net, factor, NAMES)
    small = {name: ru.shrink(img, factor) for name, img in images.items()}
    assert small["f1.png"].shape[:2] == FRAME
    det = levels_for(net, small["f1.png"])
    _, alone = run_tool(d, det, NAMES)
    _, batched = run_tool(d, det, NAMES, "--image-batch", "3")
    _, on_host = run_tool(d, det, NAMES, "--host-resize")
    assert batched == alone
    assert on_host == alone
    # and they are the files of annonet_infer_regions() on the image at the net's resolution
    detected = removed = 0
    for name, (png, csv) in batched.items():
        result, table = aa.annonet_infer_regions(net, small[name], detection_levels=det, tiling_parameters=tp())
        lines = csv.decode().splitlines()
        assert lines[0].startswith(HEADER) and float(lines[0][len(HEADER):]) == factor
        rows = table[table["detected"] == 1]
        assert len(lines) - 1 == len(rows)
        for line, row in zip(lines[1:], rows):
            f = line.split(",")
            assert len(f) == 9      # the nine fields
            assert [int(f[0])] + [int(v) for v in f[2:8]] == [int(row[n]) for n in ("label", "left", "top", "right", "bottom", "area", "seeds")]
            assert np.float32(f[8]) == row["peak"]
        (tmp_path / "check.png").write_bytes(png)
        h, w = images[name].shape[:2]
        np.testing.assert_array_equal(pu.read_png(str(tmp_path / "check.png")), pu.labels_to_rgba(pu.resize_nearest(result, w, h)))
        detected += int((table["detected"] == 1).sum())
        removed += int((table["detected"] == 0).sum())
    assert detected and removed


@pytest.mark.parametrize("factor", [1.0, 2.0])
def test_write_regions_runs_the_groups_as_batches(tmp_path, net, factor):
    """Three equal frames at --image-batch 3 are ONE batch: the tool charges a batch's time to its images in equal parts and "excluding the
    first image" excludes the first batch, so the timing line has nothing left to report; image by image it reports two images."""
    d = tmp_path / "one_batch"
    names = [("g%d.png" % i, FRAME) for i in range(3)]
    images = make_frames(d, net, factor, names)
    det = levels_for(net, ru.shrink(images["g0.png"], factor))
    out_alone, alone = run_tool(d, det, names)
    out_batched, batched = run_tool(d, det, names, "--image-batch", "3")
    assert TIMING_LINE in out_alone
    assert TIMING_LINE not in out_batched
    assert batched == alone
