"""annonet_infer_hip --gpu-score: both confusion matrices come out of annonet_score() on the GPU, and the program prints, character for
character, the matrices the host scorer prints and writes the same PNGs — image by image and in groups of --image-batch 3, at the
net's own resolution and with a downscaled net whose resizes run on the GPU.  The folder has two sizes and one image without a mask."""
import os
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "annonet_infer_hip")
K = 3
FRAME, OTHER = (60, 80), (50, 50)
# equal-sized frames and one of another size between them: groups of 2, 1 and 3 at --image-batch 3; f5 has no mask
NAMES = [("f1.png", FRAME), ("f2.png", FRAME), ("f3.png", OTHER), ("f4.png", FRAME), ("f5.png", FRAME), ("f6.png", FRAME)]
WITHOUT_MASK = "f5.png"


@pytest.fixture(scope="module")
def net():
    p, r = random_params(OracleNet(2, 3, K, 0.25, 4), 21)
    n = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    n.set_params(p, r)
    return n


def make_folder(d, net, factor):
    d.mkdir()
    (d / "annonet.dnn").write_bytes(aa.dnn_envelope_pack("", factor, net.Serialize()))
    rng = np.random.default_rng(23)
    for name, (h, w) in NAMES:
        h, w = int(h * factor), int(w * factor)
        pu.write_png(d / name, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), filter_type=1)
        if name == WITHOUT_MASK:
            continue
        gt = np.zeros((h, w), np.uint16)      # at the ORIGINAL size: the program resizes it to the net's resolution
        for _ in range(8):
            y, x = rng.integers(0, h), rng.integers(0, w)
            gt[y:y + rng.integers(5, 40), x:x + rng.integers(5, 40)] = rng.integers(0, K)
        gt[rng.random((h, w)) < 0.2] = 65535
        pu.write_png(str(d / name) + "_mask.png", pu.labels_to_rgba(gt))


def run_tool(d, *extra):
    """({name: png bytes}, the lines from "Confusion matrix per pixel:" on); the outputs are removed again"""
    args = [TOOL, str(d), "--dnn", str(d / "annonet.dnn"), "-w", "96", "-h", "96", "--precision", "fp32", "--full-image-reader-thread-count", "1"]
    r = subprocess.run(args + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "All %d images processed" % len(NAMES) in r.stdout and "All result images written!" in r.stdout
    pngs = {}
    for name, _ in NAMES:
        pngs[name] = open(str(d / name) + "_result.png", "rb").read()
        os.remove(str(d / name) + "_result.png")
    lines = r.stdout.splitlines()
    matrices = lines[lines.index("Confusion matrix per pixel:"):]
    assert "Confusion matrix per region (two-way):" in matrices
    return pngs, matrices


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("factor", [1.0, 2.0])
def test_gpu_score_prints_the_same_matrices_and_writes_the_same_files(tmp_path, net, factor, batch):
    d = tmp_path / "frames"
    make_folder(d, net, factor)
    on_host, host_matrices = run_tool(d, "--image-batch", str(batch))
    on_gpu, gpu_matrices = run_tool(d, "--image-batch", str(batch), "--gpu-score")
    assert gpu_matrices == host_matrices
    assert on_gpu == on_host
    assert len(host_matrices) > 8 and any(ch.isdigit() and ch != "0" for line in host_matrices for ch in line)


def test_gpu_score_composes_with_host_resize_and_write_regions(tmp_path, net):
    d = tmp_path / "frames"
    make_folder(d, net, 2.0)
    _, host_matrices = run_tool(d)
    for extra in (("--host-resize",), ("--write-regions", "--image-batch", "3")):
        _, gpu_matrices = run_tool(d, "--gpu-score", *extra)
        assert gpu_matrices == host_matrices, extra
    for name, _ in NAMES:
        os.remove(str(d / name) + "_result_regions.csv")
