"""Connected blobs and the region table, the CPU half: the C ABI of the device path (exports, argument checks, failing loudly without a
GPU), the reference labelling the GPU tests compare against (tests/blobs_ref.py) held to png_util.blobs_8 and to a transcription of
annonet_host.h: label_connected_blobs, and the C++ drop-in header (tests/cpp/regions_shim.cpp compiles against it)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import annonet_amd as aa
import blobs_ref as br
import png_util as pu
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("anh_label_blobs_device", "anh_regions_device", "anh_infer_regions")
INVALID = 1


def test_library_exports_the_region_symbols():
    header = open(os.path.join(ROOT, "include", "annonet_hip.h")).read()
    declared = set(re.findall(r"\b(anh_[a-z0-9_]+)\s*\(", header))
    L = aa.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in annonet_hip.h"
        assert hasattr(L, name), f"{name} is declared in annonet_hip.h but not exported"
        assert name in _lib.exported_symbols()
    assert "anh_region;" in header
    assert C.sizeof(_lib.Region) == aa.REGION_DTYPE.itemsize == 56
    for name, _ in _lib.Region._fields_:      # the numpy view of a table row and the ctypes one agree field by field
        assert aa.REGION_DTYPE.fields[name][1] == getattr(_lib.Region, name).offset, name
    assert tuple(aa.REGION_DTYPE.names) == br.REGION_FIELDS == tuple(n for n, _ in _lib.Region._fields_)


def _calls(h, w, classes=3):
    """the three entry points with every pointer null, on a map of h x w"""
    L = aa.lib()
    return (("anh_label_blobs_device", lambda: L.anh_label_blobs_device(None, None, h, w, None, None)),
            ("anh_regions_device", lambda: L.anh_regions_device(None, None, None, classes, h, w, None, 0, None, None, None)),
            ("anh_infer_regions", lambda: L.anh_infer_regions(None, None, h, w, None, None, None, None, None, None, None, None)))


def test_null_arguments_are_invalid():
    L = aa.lib()
    for name, call in _calls(20, 30):
        assert call() == INVALID, name
        assert b"null argument" in L.anh_last_error(), name


@pytest.mark.parametrize("h,w", [(0, 5), (5, 0), (-1, 5), (5, -3)])
def test_empty_maps_are_invalid(h, w):
    L = aa.lib()
    for name, call in _calls(h, w):
        assert call() == INVALID, name
        assert b"empty label map" in L.anh_last_error(), name


@pytest.mark.parametrize("h,w", [(1 << 16, 1 << 15), (46341, 46341), (2, 1 << 30), ((1 << 31) - 1, (1 << 31) - 1)])
def test_maps_of_two_to_the_31_pixels_are_invalid(h, w):
    assert h * w >= 2**31
    L = aa.lib()
    for name, call in _calls(h, w):
        assert call() == INVALID, name
        assert b"2^31" in L.anh_last_error(), name


def test_the_largest_accepted_size_passes_the_size_check():
    L = aa.lib()
    for name, call in _calls(46340, 46340) + _calls(1, 2**31 - 1):     # below 2^31: the next check (null pointers) answers
        assert call() == INVALID, name
        assert b"null argument" in L.anh_last_error(), name


def test_class_count_is_checked():
    L = aa.lib()
    for classes in (0, -2, 65536):
        assert L.anh_regions_device(None, None, None, classes, 4, 4, None, 0, None, None, None) == INVALID
        assert b"class count" in L.anh_last_error()


def test_region_calls_fail_loudly_without_a_gpu():
    if aa.lib().anh_device_count() > 0:
        pytest.skip("a GPU is present")
    lab = np.ones((4, 5), np.uint16)
    with pytest.raises(aa.AnnonetHipError) as e:      # the calls need a handle, and a handle needs a device
        aa.label_blobs(lab, net=aa.RuntimeNet(aa.net_config()))
    assert e.value.code == 3 and str(e.value)
    with pytest.raises((aa.AnnonetHipError, RuntimeError, AssertionError)):
        aa.label_blobs(lab)
    with pytest.raises((aa.AnnonetHipError, RuntimeError, AssertionError)):
        aa.regions(lab, np.zeros((3, 4, 5), np.float32))


# ---- the reference labelling ---------------------------------------------------------------------------------------------------
def random_map(rng, shape, values=(0, 1, 2), p=None):
    return rng.choice(np.array(values, np.uint16), size=shape, p=p)


def same_partition(a, b):
    """two labellings (0 = background) cut the map into the same sets"""
    if ((a == 0) != (b == 0)).any():
        return False
    pairs = np.unique(np.stack([a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize("seed", range(4))
def test_blobs_ref_partitions_as_blobs_8(seed):
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(30, 90)), int(rng.integers(30, 90)))
    lab = random_map(rng, shape, (0, 1, 2, 7, 65535), p=[0.4, 0.25, 0.25, 0.05, 0.05])
    blobs, count = br.blobs_ref(lab)
    ids, nxt = pu.blobs_8(lab)
    assert count == nxt and blobs.dtype == np.uint32
    assert same_partition(blobs, ids)
    assert sorted(np.unique(blobs)) == list(range(0 if (lab == 0).any() else 1, count))


@pytest.mark.parametrize("seed", range(6))
def test_blobs_ref_numbers_as_label_connected_blobs(seed):
    rng = np.random.default_rng(100 + seed)
    lab = random_map(rng, (20, 20), (0, 1, 2, 65535), p=[[0.5, 0.25, 0.2, 0.05], [0.2, 0.4, 0.35, 0.05]][seed % 2])
    blobs, count = br.blobs_ref(lab)
    want, want_count = br.flood_fill(lab)
    assert count == want_count
    np.testing.assert_array_equal(blobs, want)


def test_blobs_ref_edge_maps():
    for lab in (np.zeros((3, 4), np.uint16), np.ones((1, 1), np.uint16), np.array([[1, 0, 1], [0, 1, 0], [2, 0, 2]], np.uint16)):
        blobs, count = br.blobs_ref(lab)
        want, want_count = br.flood_fill(lab)
        assert count == want_count
        np.testing.assert_array_equal(blobs, want)


def test_region_table_reference_on_a_hand_made_map():
    lab = np.array([[1, 1, 0, 2],
                    [0, 1, 0, 2],
                    [5, 0, 0, 0]], np.uint16)
    planes = np.zeros((3, 3, 4), np.float32)
    planes[1] = [[1, 3, 0, 0], [0, np.nan, 0, 0], [0, 0, 0, 0]]
    planes[2, :, 3] = [0.5, 0.25, 0]
    t, blobs, count = br.region_table(lab, planes, levels=[0.0, 2.0, 1.0])
    assert count == 4
    np.testing.assert_array_equal(blobs, [[1, 1, 0, 2], [0, 1, 0, 2], [3, 0, 0, 0]])
    assert t["label"].tolist() == [1, 2, 5] and t["area"].tolist() == [3, 2, 1]
    assert (t["left"].tolist(), t["top"].tolist(), t["right"].tolist(), t["bottom"].tolist()) == ([0, 3, 0], [0, 0, 2], [1, 3, 0], [1, 1, 2])
    assert t["seeds"].tolist() == [1, 0, 0] and t["detected"].tolist() == [1, 0, 0]
    assert t["peak"].tolist() == [3.0, 0.5, -np.inf]
    np.testing.assert_array_equal(br.filtered(lab, blobs, t), [[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]])
    t0, _, _ = br.region_table(lab, planes)           # no level: seeds count margins above zero, nothing is undetected
    assert t0["seeds"].tolist() == [2, 2, 0] and t0["detected"].tolist() == [1, 1, 1]


# ---- the C++ drop-in header --------------------------------------------------------------------------------------------------------
def test_cpp_header_compiles_and_fails_with_a_message(tmp_path):
    exe = str(tmp_path / "regions_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regions_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "missing.bin"), str(tmp_path / "missing.raw"), "4", "4", "-", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip()          # a net file that is not there: an error message, not a crash
