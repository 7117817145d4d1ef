"""annonet_infer_hip --write-regions: <image>_result_regions.csv beside every result PNG holds one line per DETECTED blob of
annonet_infer_regions() on the same image (fp32 parity mode: equality); without the option the tool writes what it wrote before."""
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
NAMES = ["clean", "minor defect", "major defect"]      # parse_anno_classes' defaults for an empty json
HEADER = "class_index,class_name,left,top,right,bottom,area,seeds,peak,downscaling_factor="
IMAGES = (("a.png", (150, 130)), ("sub/b.png", (97, 131)))


def tp():
    return aa.tiling.parameters(96, 96, OV, OV)


@pytest.fixture(scope="module")
def net():
    o = OracleNet(2, 3, K, 0.25, 4)
    p, r = random_params(o, 21)
    n = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    n.set_params(p, r)
    return n


def make_dataset(d, net, factor):
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", factor, net.Serialize()))
    rng = np.random.default_rng(8)
    (d / "sub").mkdir()
    images = {}
    for name, shape in IMAGES:
        images[name] = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
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


def run_tool(d, det, *extra):
    args = [TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "-w", "96", "-h", "96", "--precision", "fp32"]
    for k in range(1, K):
        args += ["-d", "%d:%r" % (k, det[k])]
    r = subprocess.run(args + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def check_csv(path, table, factor):
    lines = open(path).read().splitlines()
    assert lines[0].startswith(HEADER) and float(lines[0][len(HEADER):]) == factor
    rows = table[table["detected"] == 1]
    assert len(lines) - 1 == len(rows)
    for line, row in zip(lines[1:], rows):
        f = line.split(",")
        assert len(f) == 9
        assert [int(f[0]), f[1]] + [int(v) for v in f[2:8]] == [int(row["label"]), NAMES[row["label"]]] + [int(row[n]) for n in ("left", "top", "right", "bottom", "area", "seeds")]
        assert np.float32(f[8]) == row["peak"]


def test_write_regions_and_unchanged_output_without_it(tmp_path, net):
    images = make_dataset(tmp_path, net, 1.0)
    det = levels_for(net, images["a.png"])
    out = run_tool(tmp_path, det, "--write-regions")
    assert "All result images written!" in out
    pngs = {}
    some_detected = some_removed = False
    for name, img in images.items():
        result, table = aa.annonet_infer_regions(net, img, detection_levels=det, tiling_parameters=tp())
        np.testing.assert_array_equal(pu.read_png(str(tmp_path / name) + "_result.png"), pu.labels_to_rgba(result))
        check_csv(str(tmp_path / name) + "_result_regions.csv", table, 1.0)
        some_detected |= bool((table["detected"] == 1).any())
        some_removed |= bool((table["detected"] == 0).any())
        pngs[name] = open(str(tmp_path / name) + "_result.png", "rb").read()
        os.remove(str(tmp_path / name) + "_result.png")
        os.remove(str(tmp_path / name) + "_result_regions.csv")
    assert some_detected and some_removed
    run_tool(tmp_path, det)        # without the option: the same PNGs and no CSV
    for name in images:
        assert open(str(tmp_path / name) + "_result.png", "rb").read() == pngs[name]
        assert not os.path.exists(str(tmp_path / name) + "_result_regions.csv")
    assert sorted(p.name for p in tmp_path.rglob("*") if p.is_file()) == sorted(["annonet.dnn"] + [os.path.basename(n) + s for n in images for s in ("", "_result.png")])


def test_write_regions_with_a_downscaled_net(tmp_path, net):
    images = make_dataset(tmp_path, net, 2.0)
    small = {name: ru.shrink(img, 2.0) for name, img in images.items()}
    det = levels_for(net, small["a.png"])
    out = run_tool(tmp_path, det, "--write-regions")      # takes the --host-resize route: the readers shrink, the table is at the net's resolution
    assert "Deserializing annonet, downscaling factor = 2" in out
    for name, img in images.items():
        result, table = aa.annonet_infer_regions(net, small[name], detection_levels=det, tiling_parameters=tp())
        check_csv(str(tmp_path / name) + "_result_regions.csv", table, 2.0)
        assert int(table["right"].max()) < small[name].shape[1] and int(table["bottom"].max()) < small[name].shape[0]
        np.testing.assert_array_equal(pu.read_png(str(tmp_path / name) + "_result.png"), pu.labels_to_rgba(pu.resize_nearest(result, img.shape[1], img.shape[0])))
