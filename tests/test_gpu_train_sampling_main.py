"""annonet_train_hip --device-sampling on the synthetic anno directory of test_gpu_train_main.py: the loader threads build no point lists
and run no label filter; the main thread prepares every image once on the device and the crop centres are picked there."""
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import png_util as pu
from test_gpu_train_main import TRAIN, dataset, train  # noqa: F401  (dataset is a fixture)

pytestmark = pytest.mark.gpu


def test_device_sampling_trains_and_skips_an_all_ignored_mask(tmp_path, dataset):
    rng = np.random.default_rng(2)
    pu.write_png(dataset / "void.png", rng.integers(0, 256, (64, 80, 3), dtype=np.uint8))
    pu.write_png(str(dataset / "void.png") + "_mask.png", pu.labels_to_rgba(np.full((64, 80), 65535, np.uint16)))
    r = train(tmp_path, dataset, "--device-sampling", "--ignore-class", "2", "--ignore-large-nonzero-regions-by-area", "0.5", "-l", "-u", steps=6)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    for line in ("images in dataset: 4", "Mini-batches are cut on the device from HBM-resident full images", "Crop centres are drawn on the device", "Classes to ignore = 2",
                 "steps: 6, ", "mean preparation time per decoded image: "):
        assert line in out, line
    assert "(device: Dataset::Prepare, " in out
    assert out.count("Warning: no labeled points in ") == 1 and "void.png_mask.png" in out       # once, and the image is skipped
    classes_json, factor, blob = aa.dnn_envelope_unpack((tmp_path / "annonet.dnn").read_bytes())
    net = aa.RuntimeNet.Deserialize(blob, aa.ANH_FP32)
    assert net.cfg.classes == 3 and net.cfg.levels == 2 and factor == 1.0


def test_device_sampling_excludes_host_crops_and_several_devices(tmp_path, dataset):
    for extra in (("--host-crops",), ("--devices", "0,0")):
        r = subprocess.run([TRAIN, str(dataset), "--device-sampling", *extra, "--max-total-steps", "1"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--device-sampling" in r.stderr, r.stdout + r.stderr
        assert not (tmp_path / "annonet.dnn").exists()


def test_device_sampling_learns(tmp_path, dataset):
    r = train(tmp_path, dataset, "--device-sampling", "--initial-learning-rate", "0.05", steps=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Crop centres are drawn on the device" in r.stdout
    classes_json, factor, blob = aa.dnn_envelope_unpack((tmp_path / "annonet.dnn").read_bytes())
    net = aa.RuntimeNet.Deserialize(blob, aa.ANH_FP32)
    # the classes are separable by brightness: the bar of the host-crops test on a training image
    img = pu.read_png(dataset / "img0.png")
    gt = pu.read_png(str(dataset / "img0.png") + "_mask.png")
    labels = aa.annonet_infer(net, img, tiling_parameters=aa.tiling.parameters(128, 128, 35, 35))
    want = np.full(gt.shape[:2], 65535, np.uint16)
    for k, col in enumerate(pu.DEFAULT_CLASSES):
        want[(gt == col).all(axis=2)] = k
    valid = want != 65535
    assert (labels[valid] == want[valid]).mean() > 0.8
