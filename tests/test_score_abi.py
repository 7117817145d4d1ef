"""Scoring on the device, the CPU half: the four new C symbols exist with the signatures the header declares, the Python mirror exports
its four calls, and the argument checks answer ANH_ERR_INVALID with a message before any device is touched."""
import ctypes as C
import os
import re

import pytest

import annonet_amd as aa
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
# name -> the parameter types of the declaration in annonet_hip.h, qualifiers and names dropped
DECLARED = {
    "anh_score_batch_device": ["anh_runtime*", "uint16_t*", "uint16_t*", "int", "int", "int", "int", "uint64_t*", "uint64_t*", "uint64_t*"],
    "anh_score_device": ["anh_runtime*", "uint16_t*", "uint16_t*", "int", "int", "int", "uint64_t*", "uint64_t*", "uint64_t*"],
    "anh_score_batch": ["anh_runtime*", "uint16_t**", "uint16_t**", "int", "int", "int", "int", "uint64_t*", "uint64_t*", "uint64_t*"],
    "anh_score": ["anh_runtime*", "uint16_t*", "uint16_t*", "int", "int", "int", "uint64_t*", "uint64_t*", "uint64_t*"],
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


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_declared_exported_and_bound_with_the_declared_signature(name):
    assert header_parameters(name) == DECLARED[name]
    L = aa.lib()
    assert hasattr(L, name), f"{name} is declared in annonet_hip.h but not exported"
    assert name in _lib.exported_symbols()
    fn = getattr(L, name)
    assert fn.restype is C.c_int
    assert ["int" if t is C.c_int else "pointer" for t in fn.argtypes] == ["pointer" if p.endswith("*") else p for p in DECLARED[name]]


def test_python_wrappers_exist():
    for name in ("score", "score_batch", "score_device", "score_batch_device"):
        assert callable(getattr(aa, name)), name


def _calls(n, classes, h, w):
    """the four entry points with every pointer null (the single-image forms have no n)"""
    L = aa.lib()
    return (("anh_score_batch_device", lambda: L.anh_score_batch_device(None, None, None, n, classes, h, w, None, None, None)),
            ("anh_score_batch", lambda: L.anh_score_batch(None, None, None, n, classes, h, w, None, None, None)),
            ("anh_score_device", lambda: L.anh_score_device(None, None, None, classes, h, w, None, None, None)),
            ("anh_score", lambda: L.anh_score(None, None, None, classes, h, w, None, None, None)))


def test_null_arguments_are_invalid():
    L = aa.lib()
    for name, call in _calls(2, 3, 20, 30):
        assert call() == INVALID, name
        assert b"null" in L.anh_last_error(), name


@pytest.mark.parametrize("n", [0, -1, -(2**31)])
def test_a_batch_needs_an_image(n):
    L = aa.lib()
    for name, call in _calls(n, 3, 20, 30)[:2]:
        assert call() == INVALID, name
        assert b"at least one image" in L.anh_last_error(), name


@pytest.mark.parametrize("classes", [0, -2, 65536])
def test_the_class_count_is_checked(classes):
    L = aa.lib()
    for name, call in _calls(1, classes, 4, 4):
        assert call() == INVALID, name
        assert b"class count" in L.anh_last_error(), name


@pytest.mark.parametrize("h,w", [(0, 5), (5, 0), (-1, 5)])
def test_empty_maps_are_invalid(h, w):
    L = aa.lib()
    for name, call in _calls(2, 3, h, w):
        assert call() == INVALID, name
        assert b"empty" in L.anh_last_error(), name


def test_sizes_beyond_the_limits_are_invalid():
    L = aa.lib()
    for name, call in _calls(1, 3, 1 << 16, 1 << 15):            # one plane of 2^31 pixels
        assert call() == INVALID, name
        assert b"2^31" in L.anh_last_error(), name
    # truth and result maps are labelled as ONE stack of 2n maps: 2 pairs of 32768 x 32768 are 2^32 pixels, 1 pair passes the size check
    for name, call in _calls(2, 3, 1 << 15, 1 << 15)[:2]:
        assert call() == INVALID, name
        assert b"2^32" in L.anh_last_error(), name
    for name, call in _calls(1, 3, 1 << 15, 1 << 15):
        assert call() == INVALID, name
        assert b"null" in L.anh_last_error(), name
    # n so large that 2n no longer fits an int
    assert L.anh_score_batch_device(None, None, None, 2**31 - 1, 3, 1, 1, None, None, None) == INVALID and b"2^32" in L.anh_last_error()
