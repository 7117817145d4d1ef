"""Dataset preparation and crop-centre sampling, the CPU half: the C ABI (exports, the ctypes mirror held to the header by a compiled
probe, argument checks that answer without a GPU) and anh_resolve_pick, which is host logic, against Python integers."""
import ctypes as C
import os
import re
import subprocess

import pytest

import annonet_amd as aa
import dataset_ref as ref
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "annonet_hip.h")
# the entry points this feature declares (the header's three new structs are checked below)
NEW_SYMBOLS = ("anh_dataset_prepare", "anh_dataset_scratch_bytes", "anh_dataset_labels", "anh_resolve_pick", "anh_dataset_pick", "anh_dataset_crop_batch_picked", "anh_trainer_step_crops_picked")
INVALID = 1

SCALARS = {"int": C.c_int, "double": C.c_double, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "long": C.c_long}
STRUCTS = {"anh_dataset_info": _lib.DatasetInfo, "anh_crop_spec": _lib.CropSpec, "anh_crop_draw": _lib.CropDraw, "anh_crop_pick": _lib.CropPick}


def declared_parameters(name):
    """the parameter types of `name` as the header declares them: [(base type, is pointer)]"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in annonet_hip.h"
    out = []
    for param in m.group(1).split(","):
        words = param.replace("*", " * ").split()
        pointer = "*" in words
        words = [w for w in words if w not in ("const", "*")]
        out.append((words[0], pointer))
    return out


def test_library_exports_the_symbols():
    L = aa.lib()
    for name in NEW_SYMBOLS:
        declared_parameters(name)
        assert hasattr(L, name), f"{name} is declared in annonet_hip.h but not exported"
        assert name in _lib.exported_symbols()


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_signatures_match_the_header(name):
    res, args = _lib._SIGNATURES[name]
    params = declared_parameters(name)
    assert res is C.c_int and len(args) == len(params), (name, params)
    for k, ((base, pointer), arg) in enumerate(zip(params, args)):
        where = f"{name} argument {k} ({base}{'*' if pointer else ''})"
        if not pointer:
            assert arg is SCALARS[base], where
        elif base in STRUCTS:
            assert arg is C.POINTER(STRUCTS[base]), where
        elif base in ("uint16_t", "uint64_t") and arg is not C.c_void_p:
            assert arg is C.POINTER({"uint16_t": C.c_uint16, "uint64_t": C.c_uint64}[base]), where
        else:
            assert arg is C.c_void_p, where


def test_struct_mirrors_match_the_compiled_header(tmp_path):
    fields = [(c_name, mirror, [f for f, _ in mirror._fields_]) for c_name, mirror in STRUCTS.items()]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "annonet_hip.h"', "int main(void) {"]
    for c_name, _, names in fields:
        lines.append(f'  printf("{c_name} %zu", sizeof({c_name}));')
        for f in names:
            lines.append(f'  printf(" %zu", offsetof({c_name}, {f}));')
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        words = line.split()
        got[words[0]] = [int(v) for v in words[1:]]
    for c_name, mirror, names in fields:
        assert got[c_name] == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in names], c_name


def info_of(classes, counts):
    info = _lib.DatasetInfo()
    info.present = len(classes)
    for i, (c, n) in enumerate(zip(classes, counts)):
        info.classes[i], info.counts[i] = c, n
    return info


@pytest.mark.parametrize("classes,counts", [([0, 1, 2, 3], [7, 4, 4, 1]), ([5], [2 ** 31 - 1]), ([0, 63], [1, 3 * 2 ** 40 + 17]), (list(range(64)), list(range(1, 65)))])
def test_resolve_pick_against_python_integers(classes, counts):
    info = info_of(classes, counts)
    draws = [(0, 0), (1, 1), (2 ** 32 - 1, 2 ** 64 - 1), (2 ** 32 - 1, 0), (0, 2 ** 64 - 1), (123456789, 0xDEADBEEFCAFEF00D), (2 ** 31, 2 ** 63), (7, 2 ** 32)]
    for class_draw, point_draw in draws:
        assert aa.resolve_pick(info, class_draw, point_draw) == ref.resolve(classes, counts, class_draw, point_draw), (class_draw, point_draw)


def test_resolve_pick_single_class_and_extreme_draws():
    info = info_of([9], [5])                                            # present = 1: every class draw lands on it
    for class_draw in (0, 1, 2 ** 32 - 1):
        assert aa.resolve_pick(info, class_draw, 2 ** 64 - 1) == (9, (2 ** 64 - 1) % 5)


def test_resolve_pick_rejects_what_it_cannot_draw_from():
    L = aa.lib()
    label, k = C.c_uint16(), C.c_uint64()
    for info in (info_of([], []), info_of([3, 4], [5, 0])):             # present = 0; a present class without pixels (slot 1)
        assert L.anh_resolve_pick(C.byref(info), 1, 7, C.byref(label), C.byref(k)) == INVALID
        assert L.anh_last_error()
    bad = info_of([1], [1])
    bad.present = 65
    assert L.anh_resolve_pick(C.byref(bad), 0, 0, C.byref(label), C.byref(k)) == INVALID
    bad.present = -1
    assert L.anh_resolve_pick(C.byref(bad), 0, 0, C.byref(label), C.byref(k)) == INVALID
    ok = info_of([1], [1])
    assert L.anh_resolve_pick(None, 0, 0, C.byref(label), C.byref(k)) == INVALID and b"null argument" in L.anh_last_error()
    assert L.anh_resolve_pick(C.byref(ok), 0, 0, None, C.byref(k)) == INVALID and b"null argument" in L.anh_last_error()
    assert L.anh_resolve_pick(C.byref(ok), 0, 0, C.byref(label), None) == INVALID and b"null argument" in L.anh_last_error()


def test_null_arguments_are_invalid_without_a_gpu():
    L = aa.lib()
    info = _lib.DatasetInfo()
    spec, draw, pick = (_lib.CropSpec * 1)(), (_lib.CropDraw * 1)(), (_lib.CropPick * 1)()
    inf = float("inf")
    calls = (("anh_dataset_prepare", lambda: L.anh_dataset_prepare(None, 0, None, 0, inf, inf, inf, 35, C.byref(info))),
             ("anh_dataset_labels", lambda: L.anh_dataset_labels(None, 0, None)),
             ("anh_dataset_scratch_bytes", lambda: L.anh_dataset_scratch_bytes(None, None)),
             ("anh_dataset_pick", lambda: L.anh_dataset_pick(None, spec, draw, 1, 35, pick)),
             ("anh_dataset_crop_batch_picked", lambda: L.anh_dataset_crop_batch_picked(None, spec, None, 1, 35, 3, 0.5, 0.5, None, None, None)),
             ("anh_trainer_step_crops_picked", lambda: L.anh_trainer_step_crops_picked(None, None, spec, draw, 1, 35, 0.5, 0.5)))
    for name, call in calls:
        assert call() == INVALID, name
        assert b"null argument" in L.anh_last_error(), name


def test_dataset_calls_fail_loudly_without_a_gpu():
    if aa.lib().anh_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(aa.AnnonetHipError) as e:      # the calls need a dataset, and a dataset needs a device
        aa.Dataset(3)
    assert e.value.code == 3 and str(e.value)
