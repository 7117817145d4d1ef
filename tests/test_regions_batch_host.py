"""Regions for batched and downscaled inference, the CPU half: the five new C symbols exist with the signatures the header declares,
their argument checks answer ANH_ERR_INVALID with a message before any device is touched, and the C++ drop-in header's three new
functions compile (tests/cpp/regions_batch_shim.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import annonet_amd as aa
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
# name -> the parameter types of the declaration in annonet_hip.h, qualifiers and names dropped
DECLARED = {
    "anh_label_blobs_batch_device": ["anh_runtime*", "uint16_t*", "int", "int", "int", "uint32_t*", "uint32_t*"],
    "anh_regions_batch_device": ["anh_runtime*", "uint16_t*", "float*", "int", "int", "int", "int", "double*", "int", "uint32_t*", "anh_region**", "size_t*"],
    "anh_infer_regions_batch": ["anh_runtime*", "uint8_t**", "int", "int", "int", "double*", "double*", "anh_tiling_params*", "uint16_t**", "uint32_t**", "float**",
                                "anh_region**", "size_t*"],
    "anh_infer_regions_scaled": ["anh_runtime*", "uint8_t*", "int", "int", "double", "double*", "double*", "anh_tiling_params*", "uint16_t*", "uint16_t*", "uint32_t*",
                                 "float*", "anh_region**", "size_t*"],
    "anh_infer_regions_scaled_batch": ["anh_runtime*", "uint8_t**", "int", "int", "int", "double", "double*", "double*", "anh_tiling_params*", "uint16_t**", "uint16_t**",
                                       "uint32_t**", "float**", "anh_region**", "size_t*"],
}


def header_parameters(name):
    header = open(os.path.join(ROOT, "include", "annonet_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in annonet_hip.h"
    text = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for param in text.split(","):
        words = param.replace("*", " * ").split()
        stars = words.count("*")
        words = [w for w in words if w not in ("const", "*")]
        out.append(words[0] + "*" * stars)          # the type is the first word that is left; the name follows it
    return out


def ctypes_kind(t):
    if t in (C.c_int,):
        return "int"
    if t is C.c_double:
        return "double"
    return "pointer"


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_declared_exported_and_bound_with_the_declared_signature(name):
    assert header_parameters(name) == DECLARED[name]
    L = aa.lib()
    assert hasattr(L, name), f"{name} is declared in annonet_hip.h but not exported"
    assert name in _lib.exported_symbols()
    fn = getattr(L, name)
    assert fn.restype is C.c_int
    want = ["pointer" if p.endswith("*") else p for p in DECLARED[name]]
    assert [ctypes_kind(t) for t in fn.argtypes] == want


def test_python_wrappers_exist():
    for name in ("label_blobs_batch", "regions_batch", "regions_batch_device", "annonet_infer_regions_batch", "annonet_infer_regions_scaled",
                 "annonet_infer_regions_scaled_batch"):
        assert callable(getattr(aa, name)), name


def _calls(n, h, w, factor=2.0, classes=3):
    """the five entry points with every pointer null"""
    L = aa.lib()
    return (("anh_label_blobs_batch_device", lambda: L.anh_label_blobs_batch_device(None, None, n, h, w, None, None)),
            ("anh_regions_batch_device", lambda: L.anh_regions_batch_device(None, None, None, n, classes, h, w, None, 0, None, None, None)),
            ("anh_infer_regions_batch", lambda: L.anh_infer_regions_batch(None, None, n, h, w, None, None, None, None, None, None, None, None)),
            ("anh_infer_regions_scaled", lambda: L.anh_infer_regions_scaled(None, None, h, w, factor, None, None, None, None, None, None, None, None, None)),
            ("anh_infer_regions_scaled_batch", lambda: L.anh_infer_regions_scaled_batch(None, None, n, h, w, factor, None, None, None, None, None, None, None, None, None)))


def test_null_arguments_are_invalid():
    L = aa.lib()
    for name, call in _calls(2, 20, 30):
        assert call() == INVALID, name
        assert b"null" in L.anh_last_error(), name


@pytest.mark.parametrize("n", [0, -1, -(2**31)])
def test_a_batch_needs_an_image(n):
    L = aa.lib()
    for name, call in _calls(n, 20, 30):
        if name == "anh_infer_regions_scaled":
            continue      # (the single-image form has no n)
        assert call() == INVALID, name
        assert b"at least one image" in L.anh_last_error(), name


@pytest.mark.parametrize("h,w", [(0, 5), (5, 0), (-1, 5)])
def test_empty_maps_are_invalid(h, w):
    L = aa.lib()
    for name, call in _calls(2, h, w):
        assert call() == INVALID, name
        assert b"empty" in L.anh_last_error(), name


def test_sizes_beyond_the_limits_are_invalid():
    L = aa.lib()
    # one plane of 2^31 pixels: the per-plane limit of the single-image calls (a scaled form cannot reach it: its sides stop at 32768)
    for name, call in _calls(1, 1 << 16, 1 << 15)[:3]:
        assert call() == INVALID, name
        assert b"2^31" in L.anh_last_error(), name
    # a batch whose tile-padded planes add up to 2^32 pixels: 4 x (32768 x 32768); 3 of them pass the size check (the null check answers)
    for name, call in _calls(4, 1 << 15, 1 << 15, factor=1.0):
        if name == "anh_infer_regions_scaled":
            continue
        assert call() == INVALID, name
        assert b"2^32" in L.anh_last_error(), name
    for name, call in _calls(3, 1 << 15, 1 << 15, factor=1.0):
        assert call() == INVALID, name
        assert b"null" in L.anh_last_error(), name
    # the sides are rounded up to the 32-pixel tiles of the labelling: 2^26 planes of 1 x 33 are 2^26 * 64 * 32 pixels to the widest launch
    assert L.anh_label_blobs_batch_device(None, None, 1 << 26, 1, 33, None, None) == INVALID and b"2^32" in L.anh_last_error()
    assert L.anh_label_blobs_batch_device(None, None, 1 << 20, 1, 33, None, None) == INVALID and b"null" in L.anh_last_error()


def test_class_count_and_factor_are_checked():
    L = aa.lib()
    for classes in (0, -2, 65536):
        assert L.anh_regions_batch_device(None, None, None, 2, classes, 4, 4, None, 0, None, None, None) == INVALID
        assert b"class count" in L.anh_last_error()
    for factor in (0.0, -1.0, float("nan"), float("inf")):
        for name, call in _calls(2, 20, 30, factor=factor)[3:]:
            assert call() == INVALID, name
            assert b"downscaling factor" in L.anh_last_error(), name


def test_negative_levels_are_refused_without_a_device():
    L = aa.lib()
    levels = (C.c_double * 3)(0.0, -1.0, 2.0)
    assert L.anh_regions_batch_device(None, None, None, 2, 3, 4, 4, levels, 0, None, None, None) == INVALID
    assert b"detection levels must be >= 0" in L.anh_last_error()


def test_cpp_header_compiles_and_fails_with_a_message(tmp_path):
    exe = str(tmp_path / "regions_batch_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regions_batch_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, str(tmp_path / "missing.bin"), str(tmp_path / "missing.raw"), "2", "4", "4", "2", "36", "28", "-", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip()          # a net file that is not there: an error message, not a crash
