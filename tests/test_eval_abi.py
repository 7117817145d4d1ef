"""Held-out evaluation, the CPU half: the five C symbols exist with the signatures the header declares, the Python mirror has its calls
and result type, the size checks answer ANH_ERR_INVALID before a device is touched, and without a GPU every entry point is
ANH_ERR_DEVICE."""
import ctypes as C

import numpy as np
import pytest

import annonet_amd as aa
from annonet_amd import _lib
from test_score_abi import header_parameters

INVALID, DEVICE = 1, 3
OUT = ["double*", "anh_eval_image*", "uint64_t*", "uint16_t*"]      # gains, per_image, confusion, predicted
DECLARED = {
    "anh_eval_logits_device": ["anh_runtime*", "float*", "uint16_t*", "float*", "int", "int", "int", "int"] + OUT,
    "anh_runtime_evaluate_device": ["anh_runtime*", "uint8_t*", "uint16_t*", "float*", "int", "int", "int"] + OUT,
    "anh_runtime_evaluate": ["anh_runtime*", "uint8_t**", "anh_wlabel**", "int", "int", "int"] + OUT,
    "anh_trainer_evaluate": ["anh_trainer*", "int", "uint8_t**", "anh_wlabel**", "int", "int", "int"] + OUT,
    "anh_trainer_evaluate_device": ["anh_trainer*", "int", "uint8_t*", "uint16_t*", "float*", "int", "int", "int"] + OUT,
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_declared_exported_and_bound_with_the_declared_signature(name):
    assert header_parameters(name) == DECLARED[name]
    L = aa.lib()
    assert hasattr(L, name) and name in _lib.exported_symbols()
    fn = getattr(L, name)
    assert fn.restype is C.c_int
    assert ["int" if t is C.c_int else "pointer" for t in fn.argtypes] == ["pointer" if p.endswith("*") else p for p in DECLARED[name]]


def test_python_mirror():
    assert C.sizeof(_lib.EvalImage) == 32 == aa.EVAL_DTYPE.itemsize
    assert [n for n, _ in _lib.EvalImage._fields_] == list(aa.EVAL_DTYPE.names)
    assert callable(aa.eval_logits_device)
    for cls in (aa.RuntimeNet, aa.TrainingNet):
        assert callable(cls.evaluate) and callable(cls.evaluate_device)
    per_image = np.zeros(2, aa.EVAL_DTYPE)
    per_image["loss_sum"], per_image["weight_sum"], per_image["counted"] = [2.0, 4.0], [1.0, 2.0], [6, 4]
    r = aa.EvalResult(per_image, np.array([[[3, 1], [0, 2]], [[1, 0], [2, 1]]], np.uint64))
    assert r.mean_loss() == 2.0 and r.pixel_accuracy() == 7 / 10
    np.testing.assert_allclose(r.class_iou(), [4 / 7, 3 / 6])


def _calls(n, h, w, classes=3):
    L = aa.lib()
    return (("anh_eval_logits_device", lambda: L.anh_eval_logits_device(None, None, None, None, n, classes, h, w, None, None, None, None)),
            ("anh_runtime_evaluate_device", lambda: L.anh_runtime_evaluate_device(None, None, None, None, n, h, w, None, None, None, None)),
            ("anh_runtime_evaluate", lambda: L.anh_runtime_evaluate(None, None, None, n, h, w, None, None, None, None)),
            ("anh_trainer_evaluate", lambda: L.anh_trainer_evaluate(None, 0, None, None, n, h, w, None, None, None, None)),
            ("anh_trainer_evaluate_device", lambda: L.anh_trainer_evaluate_device(None, 0, None, None, None, n, h, w, None, None, None, None)))


@pytest.mark.parametrize("n,h,w,word", [(0, 4, 4, b"at least one image"), (-1, 4, 4, b"at least one image"), (2, 0, 5, b"empty"), (2, 5, -1, b"empty")])
def test_sizes_are_checked_first(n, h, w, word):
    L = aa.lib()
    for name, call in _calls(n, h, w):
        assert call() == INVALID, name
        assert word in L.anh_last_error(), name


def test_null_arguments_are_invalid_where_a_gpu_is_and_a_device_error_where_none_is():
    L = aa.lib()
    for name, call in _calls(2, 35, 35):
        if L.anh_device_count() == 0:
            assert call() == DEVICE, name
            assert L.anh_last_error(), name
        else:
            assert call() == INVALID, name
            assert b"null" in L.anh_last_error(), name
