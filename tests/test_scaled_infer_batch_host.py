"""Batched downscaled inference (anh_infer_scaled_batch and its companions): what needs no GPU.  The four symbols are declared in the
header, exported by the library and registered in the Python mirror; the argument checks that come before the handle is touched answer
on a machine with no GPU; a factor that scales a side below one pixel is refused as anh_scaled_dims refuses it."""
import ctypes as C
import os
import re

import annonet_amd as aa
from annonet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANH_ERR_INVALID = 1
SYMBOLS = ["anh_resize_image_batch_device", "anh_resize_labels_batch_device", "anh_infer_scaled_batch", "anh_infer_scaled_batch_device"]


def message():
    return aa.lib().anh_last_error().decode()


def test_the_four_symbols_are_declared_exported_and_registered():
    header = open(os.path.join(ROOT, "include", "annonet_hip.h")).read()
    L = aa.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.exported_symbols(), name
        assert getattr(L, name).argtypes is not None, name
    for name in ("annonet_infer_scaled_batch", "annonet_infer_scaled_batch_device", "resize_image_batch", "resize_labels_batch"):
        assert callable(getattr(aa, name))


def test_the_batch_rejects_an_empty_batch_and_a_null_list_without_a_gpu():
    L = aa.lib()
    image = (C.c_uint8 * 48)()
    result = (C.c_uint16 * 16)()
    images = (C.c_void_p * 1)(C.addressof(image))
    results = (C.c_void_p * 1)(C.addressof(result))
    assert L.anh_infer_scaled_batch(None, images, 0, 4, 4, 2.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "at least one image" in message()
    assert L.anh_infer_scaled_batch(None, images, -3, 4, 4, 2.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "at least one image" in message()
    assert L.anh_infer_scaled_batch(None, None, 1, 4, 4, 2.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "null image or result list" in message()
    assert L.anh_infer_scaled_batch(None, images, 1, 4, 4, 2.0, None, None, None, None, None, None) == ANH_ERR_INVALID and "null image or result list" in message()
    assert L.anh_infer_scaled_batch(None, images, 1, 4, 4, 2.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "null handle" in message()
    # the device form checks n >= 1 before anything else, as anh_infer_batch_device does
    assert L.anh_infer_scaled_batch_device(None, None, 0, 4, 4, 2.0, None, None, None, None, None) == ANH_ERR_INVALID and "at least one image" in message()
    assert L.anh_infer_scaled_batch_device(None, None, 1, 4, 4, 2.0, None, None, None, None, None) == ANH_ERR_INVALID and "null argument" in message()


def test_the_batched_resizes_reject_an_empty_batch_and_null_arrays_without_a_gpu():
    L = aa.lib()
    for fn, args in ((L.anh_resize_image_batch_device, lambda n: (None, n, 3, 4, 4, None, 2, 2, None)),
                     (L.anh_resize_labels_batch_device, lambda n: (None, n, 4, 4, None, 2, 2, None))):
        assert fn(*args(0)) == ANH_ERR_INVALID and "at least one" in message()
        assert fn(*args(2)) == ANH_ERR_INVALID and "null argument" in message()


def test_a_factor_that_scales_a_side_below_one_pixel_is_refused_as_scaled_dims_refuses_it():
    # The checks run in the order of anh_infer_batch (count, lists, null handle, empty image) and then the factor's, all before the
    # handle is used for the first time: `placeholder` stands in for a handle that no machine without a GPU can create.  It passes the
    # null check and is never looked into, because the factor is refused first.
    L = aa.lib()
    sh, sw = C.c_int(), C.c_int()
    image = (C.c_uint8 * (3 * 90 * 3))()
    result = (C.c_uint16 * (3 * 90))()
    images = (C.c_void_p * 1)(C.addressof(image))
    results = (C.c_void_p * 1)(C.addressof(result))
    placeholder = (C.c_uint8 * 4096)()
    for h, w, factor, needle in ((3, 90, 8.0, "too small for this downscaling factor"), (90, 1, 2.5, "too small for this downscaling factor"),
                                 (3, 90, 0.0, "positive finite"), (3, 90, float("nan"), "positive finite"), (3, 90, 1e-5, "beyond 32768")):
        assert L.anh_scaled_dims(h, w, factor, C.byref(sh), C.byref(sw)) == ANH_ERR_INVALID
        want = message()
        assert needle in want
        assert L.anh_infer_scaled_batch(placeholder, images, 1, h, w, factor, None, None, None, results, None, None) == ANH_ERR_INVALID
        assert message() == want
        assert L.anh_infer_scaled_batch_device(placeholder, image, 1, h, w, factor, None, None, result, None, None) == ANH_ERR_INVALID
        assert message() == want
    assert L.anh_infer_scaled_batch(placeholder, images, 1, 0, 90, 2.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "empty image" in message()
    # NULL handle: refused for the handle, before the factor is looked at
    assert L.anh_infer_scaled_batch(None, images, 1, 3, 90, 8.0, None, None, None, results, None, None) == ANH_ERR_INVALID and "null handle" in message()
