"""Downscaled inference, the CPU half: the host's bilinear resize (annonet_host.h resize_image_bilinear = read_sample's
dlib::resize_image(1.0 / factor, image), annonet.cpp:153) through `host_selftest resize-image` against the numpy restatement
(tests/resize_util.py), byte for byte, and the C ABI of the device path."""
import os
import re
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import resize_util as ru
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "annonet_amd", "lib", "host_selftest")

NEW_SYMBOLS = ("anh_scaled_dims", "anh_resize_image_device", "anh_resize_labels_device", "anh_infer_scaled", "anh_infer_scaled_device")


def host_resize(tmp_path, img, scale):
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    src.write_bytes(np.ascontiguousarray(img).tobytes())
    r = subprocess.run([TOOL, "resize-image", str(src), str(h), str(w), str(c), repr(float(scale)), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out_h, out_w = map(int, r.stdout.split())
    return np.frombuffer(dst.read_bytes(), np.uint8).reshape((out_h, out_w) + img.shape[2:])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape,scale", ru.CASES)
def test_host_bilinear_equals_numpy(tmp_path, shape, scale, channels):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + channels)
    img = rng.integers(0, 256, shape + (channels,), dtype=np.uint8)
    want = ru.bilinear(img, scale)
    got = host_resize(tmp_path, img, scale)
    assert got.shape == want.shape == (ru.scaled_size(shape[0], scale), ru.scaled_size(shape[1], scale), channels)
    np.testing.assert_array_equal(got, want)
    if scale == 1.0:
        np.testing.assert_array_equal(got, img)


def test_host_bilinear_refuses_an_empty_result(tmp_path):
    src = tmp_path / "in.raw"
    src.write_bytes(bytes(2 * 5 * 3))
    r = subprocess.run([TOOL, "resize-image", str(src), "2", "5", "3", "0.2", str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "too small for this downscaling factor" in r.stderr


def test_library_exports_the_scaled_inference_symbols():
    header = open(os.path.join(ROOT, "include", "annonet_hip.h")).read()
    declared = set(re.findall(r"\b(anh_[a-z0-9_]+)\s*\(", header))
    L = aa.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in annonet_hip.h"
        assert hasattr(L, name), f"{name} is declared in annonet_hip.h but not exported"
        assert name in _lib.exported_symbols()


def test_scaled_dims_needs_no_gpu():
    assert aa.scaled_dims(101, 170, 2.0) == (51, 85)
    with pytest.raises(aa.AnnonetHipError, match="downscaling factor"):
        aa.scaled_dims(101, 170, 0.0)
