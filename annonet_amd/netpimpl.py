"""Host-side mirror of the reference's NetPimpl interface (dlib-dnn-pimpl-wrapper/NetPimpl.h, known from its call
sites: annonet_infer.cpp:49-100, annonet_train_main.cpp:376-410,558-609, annonet_infer_main.cpp:347-351) plus
annonet_infer() (annonet_infer.h:34-42), set_weights() and tiling::get_tiles, over the C ABI.

Method names follow the C++ ones so that tests read like the reference's own host code.  numpy arrays stand in for
dlib::matrix (row-major, u8 HWC images, u16 label images).
"""
import atexit
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ANH_BF16, ANH_FP32, LABEL_IGNORE, AnnonetHipError, NetConfig, check

label_to_ignore = LABEL_IGNORE


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def net_config(levels=2, in_channels=3, classes=3, width_scaler=1.0, min_filters=1, precision=ANH_BF16):
    return NetConfig(levels, in_channels, classes, width_scaler, min_filters, precision)


def set_devices(devices):
    """anh_set_devices: handles created afterwards on this thread hold one replica per listed device ([] = back to one device)."""
    arr = (C.c_int * max(len(devices), 1))(*devices)
    check(_lib.lib().anh_set_devices(arr, len(devices)))


def shard_range(n, world, rank):
    lo, hi = C.c_int64(), C.c_int64()
    check(_lib.lib().anh_shard_range(n, world, rank, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def cross_replica_overlaps(tiles, world, width, height):
    """tiles: list of (full, unique) rectangles -> sorted list of (l, t, r, b): where tiles of different replicas overlap"""
    arr = (_lib.Tile * max(len(tiles), 1))()
    for i, (full, uniq) in enumerate(tiles):
        arr[i].full_rect = _lib.Rect(*full)
        arr[i].unique_rect = _lib.Rect(*uniq)
    rects, n = C.POINTER(_lib.Rect)(), C.c_size_t()
    check(_lib.lib().anh_cross_replica_overlaps(arr, len(tiles), world, width, height, C.byref(rects), C.byref(n)))
    try:
        return [rects[i].tuple() for i in range(n.value)]
    finally:
        _lib.lib().anh_free(rects)


def net_layers(cfg):
    L = _lib.lib()
    n = L.anh_net_layer_count(C.byref(cfg))
    if n < 0:
        check(1)
    out = []
    for i in range(n):
        d = _lib.LayerDesc()
        check(L.anh_net_layer(C.byref(cfg), i, C.byref(d)))
        out.append(d)
    return out


class tiling:
    """tiling::parameters / tiling::get_tiles (annonet_infer.cpp:42, annonet_infer_main.cpp:423-427)."""

    class parameters:
        def __init__(self, max_tile_width=1024, max_tile_height=1024, overlap_x=0, overlap_y=0):
            self.max_tile_width, self.max_tile_height = max_tile_width, max_tile_height
            self.overlap_x, self.overlap_y = overlap_x, overlap_y

        def _c(self):
            return _lib.TilingParams(self.max_tile_width, self.max_tile_height, self.overlap_x, self.overlap_y)

    @staticmethod
    def get_tiles(width, height, params):
        L = _lib.lib()
        arr = C.POINTER(_lib.Tile)()
        n = C.c_size_t(0)
        p = params._c()
        check(L.anh_get_tiles(width, height, C.byref(p), C.byref(arr), C.byref(n)))
        try:
            return [(arr[i].full_rect.tuple(), arr[i].unique_rect.tuple()) for i in range(n.value)]
        finally:
            L.anh_free(arr)


WLABEL = np.dtype([("label", np.uint16), ("weight", np.float32)], align=True)   # NetPimpl::training_label_type's element


def set_weights(unweighted_label_image, class_weight, image_weight):
    """set_weights() (annonet_train.h:20-83) -> (labels u16, weights f32) = NetPimpl::training_label_type."""
    lab = np.ascontiguousarray(unweighted_label_image, dtype=np.uint16)
    out = np.zeros(lab.shape, dtype=WLABEL)
    assert out.itemsize == C.sizeof(_lib.WLabel)
    check(_lib.lib().anh_set_weights(_ptr(lab), lab.shape[0], lab.shape[1], class_weight, image_weight, _ptr(out)))
    return out


def random_rect_containing_point(draw_x, draw_y, px, py, width, height):
    r = _lib.Rect()
    check(_lib.lib().anh_random_rect_containing_point(draw_x, draw_y, px, py, width, height, C.byref(r)))
    return r.tuple()


def outpaint(img, inside):
    img = np.ascontiguousarray(img, dtype=np.uint8).copy()
    ch = 1 if img.ndim == 2 else img.shape[2]
    r = _lib.Rect(*inside)
    check(_lib.lib().anh_outpaint(_ptr(img), img.shape[0], img.shape[1], ch, C.byref(r)))
    return img


def ignore_large_nonzero_regions(label_image, receptive_field_side, by_area=float("inf"), by_width=float("inf"), by_height=float("inf")):
    """annonet_train_main.cpp:434-502: returns (label image with the too-large blobs set to LABEL_IGNORE, pixels ignored)."""
    lab = np.ascontiguousarray(label_image, dtype=np.uint16).copy()
    n = C.c_int64(0)
    check(_lib.lib().anh_ignore_large_nonzero_regions(_ptr(lab), lab.shape[0], lab.shape[1], by_area, by_width, by_height, receptive_field_side, C.byref(n)))
    return lab, n.value


class Dataset:
    """Full images + label images resident in HBM; training crops are cut on the device (randomly_crop_image,
    annonet_train_main.cpp:110-232, draws supplied by the caller).
    A crop spec is (image index, left, top, flip_left_right, flip_upside_down, brightness_change) optionally followed by
    (further_downscaling_factor, noise_level, noise_seed, (red, green, blue) colour offsets)."""

    def __init__(self, channels=3):
        self.L = _lib.lib()
        self.channels = channels
        self.h = C.c_void_p()
        check(self.L.anh_dataset_create(channels, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.anh_dataset_destroy(self.h)
            self.h = None

    def add(self, image, labels):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        lab = np.ascontiguousarray(labels, dtype=np.uint16)
        assert img.shape[:2] == lab.shape and (img.ndim == 2) == (self.channels == 1)
        idx = C.c_int()
        check(self.L.anh_dataset_add(self.h, _ptr(img), _ptr(lab), lab.shape[0], lab.shape[1], C.byref(idx)))
        return idx.value

    def remove(self, index):
        """frees that image's HBM; its index is handed out again by a later add()"""
        check(self.L.anh_dataset_remove(self.h, int(index)))

    def resident_bytes(self):
        n = C.c_uint64()
        check(self.L.anh_dataset_resident_bytes(self.h, C.byref(n)))
        return int(n.value)

    @staticmethod
    def _specs(specs):
        arr = (_lib.CropSpec * len(specs))()
        for a, s in zip(arr, specs):   # (image, left, top, flip_lr, flip_ud, brightness[, further downscaling, noise level, noise seed, (dr, dg, db)])
            a.image, a.left, a.top, a.flip_left_right, a.flip_upside_down, a.brightness_change = int(s[0]), int(s[1]), int(s[2]), int(s[3]), int(s[4]), float(s[5])
            if len(s) > 6:
                a.further_downscaling_factor, a.noise_level, a.noise_seed = float(s[6]), int(s[7]), int(s[8])
                for k in range(3):
                    a.color_offset[k] = int(s[9][k])
        return arr

    def crop_batch(self, specs, dim, classes, class_weight=0.5, image_weight=0.5):
        """-> (images n x dim x dim [x 3] u8, labels n x dim x dim u16, weights n x dim x dim f32)"""
        n = len(specs)
        shape = (n, dim, dim) if self.channels == 1 else (n, dim, dim, self.channels)
        img = np.empty(shape, dtype=np.uint8)
        wl = np.empty((n, dim, dim), dtype=WLABEL)
        check(self.L.anh_dataset_crop_batch(self.h, self._specs(specs), n, dim, classes, class_weight, image_weight, _ptr(img), _ptr(wl)))
        return img, wl["label"].copy(), wl["weight"].copy()

    # ---- preparation and crop-centre sampling on the device ----
    def prepare(self, index, classes_to_ignore=(), by_area=float("inf"), by_width=float("inf"), by_height=float("inf"), receptive_field_side=1):
        """ignore_classes_to_ignore + ignore_large_nonzero_regions (annonet_train_main.cpp:414-502) on the resident label image, then its point
        index.  -> dict(ignored_by_class, ignored_by_size, classes (ascending), counts)"""
        ign = np.ascontiguousarray(list(classes_to_ignore), dtype=np.uint16)
        info = _lib.DatasetInfo()
        check(self.L.anh_dataset_prepare(self.h, int(index), _ptr(ign) if ign.size else None, int(ign.size), float(by_area), float(by_width), float(by_height),
                                         int(receptive_field_side), C.byref(info)))
        return {"ignored_by_class": info.ignored_by_class, "ignored_by_size": info.ignored_by_size,
                "classes": [int(info.classes[i]) for i in range(info.present)], "counts": [int(info.counts[i]) for i in range(info.present)], "info": info}

    def scratch_bytes(self):
        """bytes of prepare()'s scratch the dataset holds (index counts; with a finite size limit also parents, blob map, region table)"""
        n = C.c_uint64()
        check(self.L.anh_dataset_scratch_bytes(self.h, C.byref(n)))
        return int(n.value)

    def labels(self, index, shape):
        """the resident label image as it stands; shape = (height, width) as added"""
        out = np.empty(shape, dtype=np.uint16)
        check(self.L.anh_dataset_labels(self.h, int(index), _ptr(out)))
        return out

    @staticmethod
    def _draws(draws):
        arr = (_lib.CropDraw * len(draws))()
        for a, d in zip(arr, draws):   # (class draw, point draw, rect draw x, rect draw y)
            a.class_draw, a.point_draw, a.rect_draw_x, a.rect_draw_y = int(d[0]), int(d[1]), int(d[2]), int(d[3])
        return arr

    @staticmethod
    def _picks(arr):
        return [(p.label, p.x, p.y, p.left, p.top) for p in arr]

    def pick(self, specs, draws, dim):
        """-> [(label, x, y, left, top)]: the pixel each draw selects and the corner of the rectangle drawn around it"""
        assert len(specs) == len(draws)
        out = (_lib.CropPick * len(specs))()
        check(self.L.anh_dataset_pick(self.h, self._specs(specs), self._draws(draws), len(specs), dim, out))
        return self._picks(out)

    def crop_batch_picked(self, specs, draws, dim, classes, class_weight=0.5, image_weight=0.5):
        """crop_batch with the rectangles picked on the device (the specs' left / top are ignored) -> (images, labels, weights, picks)"""
        assert len(specs) == len(draws)
        n = len(specs)
        shape = (n, dim, dim) if self.channels == 1 else (n, dim, dim, self.channels)
        img = np.empty(shape, dtype=np.uint8)
        wl = np.empty((n, dim, dim), dtype=WLABEL)
        picks = (_lib.CropPick * n)()
        check(self.L.anh_dataset_crop_batch_picked(self.h, self._specs(specs), self._draws(draws), n, dim, classes, class_weight, image_weight, _ptr(img), _ptr(wl), picks))
        return img, wl["label"].copy(), wl["weight"].copy(), self._picks(picks)


def resolve_pick(info, class_draw, point_draw):
    """annonet_train_main.cpp:121,131 on an anh_dataset_info (Dataset.prepare(...)["info"]): -> (label, k)"""
    label, k = C.c_uint16(), C.c_uint64()
    check(_lib.lib().anh_resolve_pick(C.byref(info), class_draw, point_draw, C.byref(label), C.byref(k)))
    return label.value, k.value


def dnn_envelope_pack(anno_classes_json, downscaling_factor, serialized_runtime_net):
    """The bytes of annonet.dnn (annonet_train_main.cpp:557-565): dlib serialize of (string, double, string)."""
    L = _lib.lib()
    js = anno_classes_json.encode() if isinstance(anno_classes_json, str) else bytes(anno_classes_json)
    net = bytes(serialized_runtime_net)
    out, n = C.c_void_p(), C.c_size_t()
    check(L.anh_dnn_envelope_pack(js, len(js), float(downscaling_factor), C.create_string_buffer(net, len(net)), len(net), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        L.anh_free(out)


def dnn_envelope_unpack(file_bytes):
    """annonet_infer_main.cpp:340-351: (anno_classes_json bytes, downscaling factor, serialized RuntimeNet bytes)."""
    L = _lib.lib()
    data = bytes(file_bytes)
    js, jn, f, net, nn = C.c_void_p(), C.c_size_t(), C.c_double(), C.c_void_p(), C.c_size_t()
    check(L.anh_dnn_envelope_unpack(C.create_string_buffer(data, len(data)), len(data), C.byref(js), C.byref(jn), C.byref(f), C.byref(net), C.byref(nn)))
    try:
        return C.string_at(js, jn.value), f.value, C.string_at(net, nn.value)
    finally:
        L.anh_free(js); L.anh_free(net)


def count_steps_without_decrease(values, probability_of_decrease=0.51):
    v = np.ascontiguousarray(values, dtype=np.float64)
    return _lib.lib().anh_count_steps_without_decrease(_ptr(v), v.size, probability_of_decrease)


class _Profiled:
    _is_trainer = 0

    def profile_enable(self, on=True):
        check(self.L.anh_profile_enable(self.h, self._is_trainer, int(on)))

    def profile_set_filter(self, substring=""):
        check(self.L.anh_profile_set_filter(self.h, self._is_trainer, (substring or "").encode()))

    def profile_set_sampling(self, every=1):
        check(self.L.anh_profile_set_sampling(self.h, self._is_trainer, int(every)))

    def profile_reset(self):
        check(self.L.anh_profile_reset(self.h, self._is_trainer))

    def profile_launch_order(self):
        """Entry names of the most recent pass in host enqueue order (one per kernel-class launch)."""
        need = C.c_size_t()
        check(self.L.anh_profile_launch_order(self.h, self._is_trainer, None, 0, C.byref(need)))
        buf = C.create_string_buffer(max(need.value, 1))
        check(self.L.anh_profile_launch_order(self.h, self._is_trainer, buf, need.value, None))
        return [x for x in buf.value.decode().split("\n") if x]

    def profile(self):
        n = self.L.anh_profile_count(self.h, self._is_trainer)
        if n < 0:
            check(1)
        out = []
        for i in range(n):
            name = C.create_string_buffer(128)
            ms, cnt, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            check(self.L.anh_profile_entry(self.h, self._is_trainer, i, name, 128, C.byref(ms), C.byref(cnt), C.byref(fl), C.byref(by)))
            out.append({"name": name.value.decode(), "total_ms": ms.value, "launches": cnt.value, "flops": fl.value, "bytes": by.value})
        return out


class RuntimeNet(_Profiled):
    """NetPimpl::RuntimeNet."""

    def __init__(self, cfg=None, _handle=None):
        self.L = _lib.lib()
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
        else:
            cfg = cfg or net_config()
            check(self.L.anh_runtime_create(C.byref(cfg), C.byref(self.h)))
        c = NetConfig()
        check(self.L.anh_runtime_config(self.h, C.byref(c)))
        self.cfg = c
        self.n_params = self.L.anh_net_param_count(C.byref(c))
        self.n_running = self.L.anh_net_running_count(C.byref(c))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.anh_runtime_destroy(self.h)
            self.h = None

    @staticmethod
    def GetRecommendedInputDimension(levels, n):
        return _lib.lib().anh_recommended_input_dim(levels, n)

    def set_params(self, params, running):
        p = np.ascontiguousarray(params, dtype=np.float32)
        r = np.ascontiguousarray(running, dtype=np.float32)
        check(self.L.anh_runtime_set_params(self.h, _ptr(p), p.size, _ptr(r), r.size))

    def get_params(self):
        p = np.empty(self.n_params, np.float32)
        r = np.empty(self.n_running, np.float32)
        check(self.L.anh_runtime_get_params(self.h, _ptr(p), p.size, _ptr(r), r.size))
        return p, r

    def Serialize(self):
        blob, n = C.c_void_p(), C.c_size_t()
        check(self.L.anh_runtime_serialize(self.h, C.byref(blob), C.byref(n)))
        try:
            return C.string_at(blob, n.value)
        finally:
            self.L.anh_free(blob)

    @classmethod
    def Deserialize(cls, data, precision=ANH_BF16):
        L = _lib.lib()
        h = C.c_void_p()
        buf = C.create_string_buffer(data, len(data))
        check(L.anh_runtime_deserialize(buf, len(data), precision, C.byref(h)))
        return cls(_handle=h)

    def Forward(self, input_tile):
        """u8 [H,W,C] (or [N,H,W,C]) -> fp32 [K,H,W] (or [N,K,H,W]); the returned array is a copy."""
        img = np.ascontiguousarray(input_tile, dtype=np.uint8)
        single = img.ndim != 4
        if img.ndim == 2:
            img = img[None, :, :, None]
        elif img.ndim == 3:
            img = img[None]
        n, h, w, c = img.shape
        if c != self.cfg.in_channels:
            raise AnnonetHipError(1, "channel count does not match the net input")
        out = C.POINTER(C.c_float)()
        k, nr, nc = C.c_int(), C.c_int(), C.c_int()
        check(self.L.anh_runtime_forward(self.h, _ptr(img), n, h, w, C.byref(out), C.byref(k), C.byref(nr), C.byref(nc)))
        arr = np.ctypeslib.as_array(out, shape=(n, k.value, nr.value, nc.value)).copy()
        return arr[0] if single else arr

    def synchronize(self):
        check(self.L.anh_runtime_synchronize(self.h))

    def set_stream(self, stream_ptr):
        """Launch on the caller's (non-default) HIP stream.  The legacy default stream (0) cannot be named through this call:
        0 / None means "back to a stream of the handle's own".  To order torch work with the handle, use stream_ptr()."""
        check(self.L.anh_runtime_set_stream(self.h, stream_ptr or None))

    def stream_ptr(self):
        s = C.c_void_p()
        check(self.L.anh_runtime_get_stream(self.h, C.byref(s)))
        return s.value or 0

    def stores_activations(self):
        """whether the handle's last inference pass stored post-activation tensors (anh_runtime_stores_activations)"""
        yes = C.c_int()
        check(self.L.anh_runtime_stores_activations(self.h, C.byref(yes)))
        return bool(yes.value)

    def layer_tensor(self, layer):
        """fp32 [n,h,w,c]: the tensor bn layer `layer` stored in the handle's last inference pass (anh_runtime_layer_tensor); raises
        for a layer that pass did not store"""
        dims = (C.c_int * 4)()
        check(self.L.anh_runtime_layer_tensor(self.h, layer, None, 0, dims))
        out = np.empty(tuple(dims), np.float32)
        check(self.L.anh_runtime_layer_tensor(self.h, layer, _ptr(out), out.size, dims))
        return out

    def evaluate(self, samples, labels, gains=None, want_predicted=False):
        """anh_runtime_evaluate on host samples: a list of u8 [H,W,C] and a list of (label, weight) arrays as set_weights() returns
        them -> EvalResult"""
        imgs, labs, ip, lp, n, h, w = _eval_samples(samples, labels)
        per_image, confusion = _eval_outputs(n, self.cfg.classes, None)
        predicted = np.empty((n, h, w), np.uint16) if want_predicted else None
        check(self.L.anh_runtime_evaluate(self.h, ip, lp, n, h, w, _ptr(_eval_gains(gains, self.cfg.classes)), _ptr(per_image), _ptr(confusion), _ptr(predicted)))
        return EvalResult(per_image, confusion, predicted)

    def evaluate_device(self, d_images_ptr, d_labels_ptr, d_weights_ptr, n, height, width, gains=None, d_predicted_ptr=0, prefill=None):
        """anh_runtime_evaluate_device on resident windows [n,H,W,C] u8, labels [n,H,W] u16 and weights [n,H,W] fp32 (0 = ones), device
        pointers as ints -> EvalResult (the predicted maps stay on the device, at d_predicted_ptr)"""
        per_image, confusion = _eval_outputs(n, self.cfg.classes, prefill)
        check(self.L.anh_runtime_evaluate_device(self.h, d_images_ptr or None, d_labels_ptr or None, d_weights_ptr or None, n, height, width,
                                                 _ptr(_eval_gains(gains, self.cfg.classes)), _ptr(per_image), _ptr(confusion), d_predicted_ptr or None))
        return EvalResult(per_image, confusion)


# ---- what the inference wrappers share: their arguments as the C ABI takes them ----
def _f64(values):
    return np.ascontiguousarray(values, dtype=np.float64) if values is not None else None


def _images(net, input_images):
    """u8 images of ONE size -> (contiguous [H,W,C] arrays, H, W); a [H,W] image gets its channel axis"""
    imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in input_images]
    imgs = [im[:, :, None] if im.ndim == 2 else im for im in imgs]
    if imgs and any(im.shape != imgs[0].shape for im in imgs):
        raise AnnonetHipError(1, "the images of a batch must have one size and channel count")
    H, W, c = imgs[0].shape if imgs else (0, 0, net.cfg.in_channels)
    if c != net.cfg.in_channels:
        raise AnnonetHipError(1, "channel count does not match the net input")
    return imgs, H, W


def _per_class(net, gains, detection_levels):
    """gains and detection levels as f64 arrays (or None), one value per class of the net"""
    g, d = _f64(gains), _f64(detection_levels)
    if g is not None and g.size != net.cfg.classes or d is not None and d.size != net.cfg.classes:
        raise AnnonetHipError(1, "gains / detection levels need one value per class")
    return g, d


def _tiling_ref(tiling_parameters):
    """anh_tiling_params by reference (None: the image is one tile)"""
    return C.byref(tiling_parameters._c()) if tiling_parameters is not None else None


def _tile_array(tiles):
    """list of (full, unique) rectangles -> anh_tile[]"""
    arr = (_lib.Tile * max(len(tiles), 1))()
    for i, (full, uniq) in enumerate(tiles):
        arr[i].full_rect = _lib.Rect(*full)
        arr[i].unique_rect = _lib.Rect(*uniq)
    return arr


def _per_image(want, n):
    """a want_* argument, one boolean for all images or a list with one per image -> list of n"""
    return list(want) if isinstance(want, (list, tuple)) else [bool(want)] * n


def _outputs(want, shape, dtype):
    return [np.empty(shape, dtype) if w else None for w in want]


def _ptrs(arrays, n):
    """the arrays' addresses as a void*[n] (NULL where an entry is None)"""
    return (C.c_void_p * max(n, 1))(*[a.ctypes.data if a is not None else None for a in arrays])


def annonet_infer(net, input_image, gains=None, detection_levels=None, tiling_parameters=None, want_blended=False):
    """annonet_infer() (annonet_infer.h:34-42): returns the u16 label image (and the blended class planes)."""
    (img,), H, W = _images(net, [input_image])
    g, d = _per_class(net, gains, detection_levels)
    res = np.empty((H, W), np.uint16)
    bl = np.empty((net.cfg.classes, H, W), np.float32) if want_blended else None
    check(net.L.anh_infer(net.h, _ptr(img), H, W, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptr(res), _ptr(bl)))
    return (res, bl) if want_blended else res


def annonet_infer_device(net, d_image_ptr, height, width, d_labels_ptr, d_blended_ptr, gains=None, tiling_parameters=None, tiles=None):
    """annonet_infer() with the image, the label map and the blended planes resident in HBM (device pointers as ints).
    `tiles` (list of (full, unique) rects) restricts the call to a shard of the tile list (multi-GPU inference)."""
    arr, n = (_tile_array(tiles), len(tiles)) if tiles is not None else (None, 0)
    check(net.L.anh_infer_device(net.h, d_image_ptr, height, width, _ptr(_f64(gains)), _tiling_ref(tiling_parameters), arr, n, d_labels_ptr, d_blended_ptr))


def annonet_infer_batch(net, input_images, gains=None, detection_levels=None, tiling_parameters=None, want_blended=False):
    """annonet_infer() over several images of ONE size in one call (anh_infer_batch): a list of u8 images (or an array [n,H,W,C]) ->
    list of u16 label images (and, with want_blended, the list of their blended class planes).  want_blended may also be a list of
    booleans, one per image.  Every image's result equals annonet_infer() of that image alone, bit for bit."""
    g, d = _per_class(net, gains, detection_levels)
    imgs, H, W = _images(net, input_images)
    n = len(imgs)
    want = _per_image(want_blended, n)
    res = _outputs([True] * n, (H, W), np.uint16)
    bl = _outputs(want, (net.cfg.classes, H, W), np.float32)
    check(net.L.anh_infer_batch(net.h, _ptrs(imgs, n), n, H, W, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptrs(res, n), _ptrs(bl, n) if any(want) else None))
    return (res, bl) if any(want) or want_blended else res


def annonet_infer_batch_device(net, d_images_ptr, n, height, width, d_labels_ptr, d_blended_ptr=0, gains=None, tiling_parameters=None):
    """annonet_infer_batch with the images [n,H,W,C], the label maps [n,H,W] and (optionally) the planes [n,K,H,W] resident in HBM
    (device pointers as ints); enqueued on the handle's stream, not synchronised."""
    check(net.L.anh_infer_batch_device(net.h, d_images_ptr, n, height, width, _ptr(_f64(gains)), _tiling_ref(tiling_parameters), d_labels_ptr, d_blended_ptr or None))


def labels_from_logits_device(net, d_logits_ptr, count, classes, win_height, win_width, top, left, height, width, d_labels_ptr, gains=None):
    """find_label straight from the logits [count,classes,win_height,win_width] of whole-image tiles whose window starts at (left, top):
    label maps [count,height,width] (anh_labels_from_logits_device)."""
    check(net.L.anh_labels_from_logits_device(net.h, d_logits_ptr, count, classes, win_height, win_width, top, left, height, width, _ptr(_f64(gains)), d_labels_ptr))


def infer_batch_plan(tiles, n_images, levels, cap):
    """anh_infer_batch_plan: tiles = one image's list of (full, unique) rectangles -> the forward batches, each a list of (image, tile)."""
    arr = _tile_array(tiles)
    pairs, sizes, nb = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.c_size_t()
    L = _lib.lib()
    check(L.anh_infer_batch_plan(arr, len(tiles), n_images, levels, cap, C.byref(pairs), C.byref(sizes), C.byref(nb)))
    try:
        out, k = [], 0
        for b in range(nb.value):
            out.append([(pairs[2 * (k + j)], pairs[2 * (k + j) + 1]) for j in range(sizes[b])])
            k += sizes[b]
        return out
    finally:
        L.anh_free(pairs)
        L.anh_free(sizes)


def scaled_dims(height, width, downscaling_factor):
    """anh_scaled_dims: (scaled height, scaled width) = the size dlib::resize_image(1.0 / factor, img) gives (annonet.cpp:153)."""
    sh, sw = C.c_int(), C.c_int()
    check(_lib.lib().anh_scaled_dims(height, width, downscaling_factor, C.byref(sh), C.byref(sw)))
    return sh.value, sw.value


def annonet_infer_scaled(net, input_image, downscaling_factor, gains=None, detection_levels=None, tiling_parameters=None, want_scaled=False, want_blended=False):
    """read_sample's resize (annonet.cpp:153) + annonet_infer() + resize_label_image (annonet_infer_main.cpp:413) on the device: the image
    comes at its original size, the label map comes back at that size.  Returns the map, then (when asked for) the map at the net's
    resolution and the blended class planes at the net's resolution."""
    (img,), H, W = _images(net, [input_image])
    g, d = _per_class(net, gains, detection_levels)
    sh, sw = scaled_dims(H, W, downscaling_factor)
    res = np.empty((H, W), np.uint16)
    scaled = np.empty((sh, sw), np.uint16) if want_scaled else None
    bl = np.empty((net.cfg.classes, sh, sw), np.float32) if want_blended else None
    check(net.L.anh_infer_scaled(net.h, _ptr(img), H, W, downscaling_factor, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptr(res), _ptr(scaled), _ptr(bl)))
    out = (res,) + ((scaled,) if want_scaled else ()) + ((bl,) if want_blended else ())
    return out if len(out) > 1 else res


def annonet_infer_scaled_device(net, d_image_ptr, height, width, downscaling_factor, d_labels_ptr, d_scaled_labels_ptr=0, d_blended_ptr=0, gains=None, tiling_parameters=None):
    """annonet_infer_scaled with the original-size image, the original-size label map and (optionally) the map and the planes at the
    net's resolution resident in HBM (device pointers as ints); enqueued on the handle's stream, not synchronised."""
    check(net.L.anh_infer_scaled_device(net.h, d_image_ptr, height, width, downscaling_factor, _ptr(_f64(gains)), _tiling_ref(tiling_parameters),
                                        d_labels_ptr, d_scaled_labels_ptr or None, d_blended_ptr or None))


def annonet_infer_scaled_batch(net, input_images, downscaling_factor, gains=None, detection_levels=None, tiling_parameters=None, want_scaled=False, want_blended=False):
    """annonet_infer_scaled over several images of ONE original size in one call (anh_infer_scaled_batch): one batched shrink, the
    forward batches of annonet_infer_batch at the net's resolution, one batched blow-up.  Returns the list of original-size label maps,
    then (when asked for) the list of maps at the net's resolution and the list of blended class planes at the net's resolution.
    want_scaled / want_blended may also be lists of booleans, one per image (None where not asked for).  Every image's results equal
    annonet_infer_scaled() of that image alone, bit for bit."""
    g, d = _per_class(net, gains, detection_levels)
    imgs, H, W = _images(net, input_images)
    n = len(imgs)
    sh, sw = scaled_dims(H, W, downscaling_factor) if n else (0, 0)
    ws, wb = _per_image(want_scaled, n), _per_image(want_blended, n)
    res = _outputs([True] * n, (H, W), np.uint16)
    sc = _outputs(ws, (sh, sw), np.uint16)
    bl = _outputs(wb, (net.cfg.classes, sh, sw), np.float32)
    check(net.L.anh_infer_scaled_batch(net.h, _ptrs(imgs, n), n, H, W, downscaling_factor, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters),
                                       _ptrs(res, n), _ptrs(sc, n) if any(ws) else None, _ptrs(bl, n) if any(wb) else None))
    out = (res,) + ((sc,) if any(ws) or want_scaled else ()) + ((bl,) if any(wb) or want_blended else ())
    return out if len(out) > 1 else res


def annonet_infer_scaled_batch_device(net, d_images_ptr, n, height, width, downscaling_factor, d_labels_ptr, d_scaled_labels_ptr=0, d_blended_ptr=0, gains=None,
                                      tiling_parameters=None):
    """annonet_infer_scaled_batch with the original-size images [n,H,W,C], the original-size label maps [n,H,W] and (optionally) the maps
    [n,sh,sw] and the planes [n,K,sh,sw] at the net's resolution resident in HBM (device pointers as ints); enqueued on the handle's
    stream, not synchronised."""
    check(net.L.anh_infer_scaled_batch_device(net.h, d_images_ptr, n, height, width, downscaling_factor, _ptr(_f64(gains)), _tiling_ref(tiling_parameters),
                                              d_labels_ptr, d_scaled_labels_ptr or None, d_blended_ptr or None))


def _through_device(src, out_shape, dtype, prefill, launch):
    """host array -> HBM -> `launch(src_ptr, dst_ptr, stream)` -> host array (torch moves the bytes)"""
    import torch
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1)).cuda()
    n = int(np.prod(out_shape)) * np.dtype(dtype).itemsize
    d_dst = torch.empty(n, dtype=torch.uint8, device="cuda") if prefill is None else torch.full((n,), int(prefill) & 255, dtype=torch.uint8, device="cuda")
    launch(d_src.data_ptr(), d_dst.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return d_dst.cpu().numpy().view(dtype).reshape(out_shape)


def resize_image(img, out_h, out_w, prefill=None):
    """The device's bilinear resize (anh_resize_image_device) on a host u8 image [H,W] / [H,W,1] / [H,W,3]; `prefill`: byte the
    destination is filled with before the kernel runs (tests: every output element must be written)."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    c = 1 if a.ndim == 2 else a.shape[2]
    L = _lib.lib()
    return _through_device(a, (out_h, out_w) + a.shape[2:], np.uint8, prefill,
                           lambda s, d, st: check(L.anh_resize_image_device(s, c, a.shape[0], a.shape[1], d, out_h, out_w, st)))


def resize_labels(lab, out_w, out_h, prefill=None):
    """The device's nearest-neighbour resize (anh_resize_labels_device) on a host u16 label map; arguments as resize_label_image
    (annonet.cpp:134: target width, then target height)."""
    a = np.ascontiguousarray(lab, dtype=np.uint16)
    L = _lib.lib()
    return _through_device(a, (out_h, out_w), np.uint16, prefill,
                           lambda s, d, st: check(L.anh_resize_labels_device(s, a.shape[0], a.shape[1], d, out_h, out_w, st)))


def resize_image_batch(images, out_h, out_w, prefill=None):
    """The device's bilinear resize over a batch by ONE launch (anh_resize_image_batch_device): host u8 images [n,H,W] / [n,H,W,1] /
    [n,H,W,3] -> [n,out_h,out_w(,C)]; `prefill` as for resize_image."""
    a = np.ascontiguousarray(images, dtype=np.uint8)
    if a.ndim not in (3, 4) or a.shape[0] < 1:
        raise AnnonetHipError(1, "resize_image_batch: an array [n,H,W] or [n,H,W,C] with n >= 1")
    c = 1 if a.ndim == 3 else a.shape[3]
    L = _lib.lib()
    return _through_device(a, (a.shape[0], out_h, out_w) + a.shape[3:], np.uint8, prefill,
                           lambda s, d, st: check(L.anh_resize_image_batch_device(s, a.shape[0], c, a.shape[1], a.shape[2], d, out_h, out_w, st)))


def resize_labels_batch(maps, out_w, out_h, prefill=None):
    """The device's nearest-neighbour resize over a batch by ONE launch (anh_resize_labels_batch_device): host u16 label maps [n,H,W]
    -> [n,out_h,out_w]; target width, then target height, as for resize_labels."""
    a = np.ascontiguousarray(maps, dtype=np.uint16)
    if a.ndim != 3 or a.shape[0] < 1:
        raise AnnonetHipError(1, "resize_labels_batch: an array [n,H,W] with n >= 1")
    L = _lib.lib()
    return _through_device(a, (a.shape[0], out_h, out_w), np.uint16, prefill,
                           lambda s, d, st: check(L.anh_resize_labels_batch_device(s, a.shape[0], a.shape[1], a.shape[2], d, out_h, out_w, st)))


REGION_DTYPE = np.dtype({"names": ["blob", "label", "detected", "left", "top", "right", "bottom", "first_row", "first_col", "area", "seeds", "peak"],
                         "formats": ["<u4", "<u2", "<u2", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i8", "<i8", "<f4"],
                         "offsets": [0, 4, 6, 8, 12, 16, 20, 24, 28, 32, 40, 48], "itemsize": C.sizeof(_lib.Region)})   # anh_region

_blob_net = None


def _net_for_blobs(net):
    """the handle whose stream the labelling runs on: the caller's, or a smallest net of the module's own (the labelling uses no weights)"""
    global _blob_net
    if net is not None:
        return net
    if _blob_net is None:
        _blob_net = RuntimeNet(net_config(1, 3, 3, 0.25, 4, ANH_FP32))
        atexit.register(_drop_blob_net)   # released while the interpreter and the HIP runtime are still whole
    return _blob_net


def _drop_blob_net():
    global _blob_net
    _blob_net = None


def _take_regions(L, table, n):
    """the malloc'd table of a regions call -> numpy structured array (REGION_DTYPE); releases the block"""
    try:
        # (a view of the bytes as they came: numpy's copy of a structured array leaves the padding of its rows undefined)
        return np.frombuffer(bytearray(C.string_at(table, n * REGION_DTYPE.itemsize)), REGION_DTYPE) if n else np.zeros(0, REGION_DTYPE)
    finally:
        L.anh_free(table)


def label_blobs(label_map, prefill=None, net=None):
    """The device's connected-blob labelling (anh_label_blobs_device) on a host u16 label map: (u32 blob map, count), count = blobs + 1 as
    label_connected_blobs returns it.  `prefill`: byte the blob map is filled with before the kernels run (tests: every element must be
    written)."""
    a = np.require(label_map, dtype=np.uint16, requirements=["C", "W"])   # (torch wants a writable source)
    if a.ndim != 2:
        raise AnnonetHipError(1, "label_blobs: a label map [H,W]")
    net = _net_for_blobs(net)
    count = C.c_uint32()

    def launch(s, d, st):
        import torch
        torch.cuda.current_stream().synchronize()   # the upload and the prefill ran on torch's stream; the labelling runs on the handle's
        check(net.L.anh_label_blobs_device(net.h, s, a.shape[0], a.shape[1], d, C.byref(count)))
    blobs = _through_device(a, a.shape, np.uint32, prefill, launch)
    return blobs, count.value


def regions_device(net, d_labels_ptr, d_blended_ptr, classes, height, width, detection_levels=None, apply_filter=False, d_blobs_ptr=0):
    """anh_regions_device on resident buffers (device pointers as ints): the region table as a numpy structured array (REGION_DTYPE)."""
    d = _f64(detection_levels)
    if d is not None and d.size != classes:
        raise AnnonetHipError(1, "detection levels need one value per class")
    table, n = C.POINTER(_lib.Region)(), C.c_size_t()
    check(net.L.anh_regions_device(net.h, d_labels_ptr, d_blended_ptr, classes, height, width, _ptr(d), 1 if apply_filter else 0, d_blobs_ptr or None,
                                   C.byref(table), C.byref(n)))
    return _take_regions(net.L, table, n.value)


def regions(label_map, blended, detection_levels=None, apply_filter=False, prefill=None, net=None):
    """anh_regions_device on host arrays (torch moves the bytes): u16 label map [H,W] and fp32 planes [K,H,W] ->
    (region table, u32 blob map, the label map as the call leaves it)."""
    import torch
    lab = np.require(label_map, dtype=np.uint16, requirements=["C", "W"])
    planes = np.require(blended, dtype=np.float32, requirements=["C", "W"])
    if lab.ndim != 2 or planes.ndim != 3 or planes.shape[1:] != lab.shape:
        raise AnnonetHipError(1, "regions: a label map [H,W] and planes [K,H,W]")
    net = _net_for_blobs(net)
    H, W = lab.shape
    d_lab = torch.from_numpy(lab.view(np.uint8).reshape(-1)).cuda()
    d_planes = torch.from_numpy(planes).cuda()
    n = H * W * 4
    d_blobs = torch.empty(n, dtype=torch.uint8, device="cuda") if prefill is None else torch.full((n,), int(prefill) & 255, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    table = regions_device(net, d_lab.data_ptr(), d_planes.data_ptr(), planes.shape[0], H, W, detection_levels, apply_filter, d_blobs.data_ptr())
    return table, d_blobs.cpu().numpy().view(np.uint32).reshape(H, W), d_lab.cpu().numpy().view(np.uint16).reshape(H, W)


def detection_filter_device(net, d_labels_ptr, d_blended_ptr, classes, height, width, detection_levels):
    """anh_detection_filter_device on resident buffers (device pointers as ints): annonet_infer's flood filter on the map, in place;
    returns the host rounds it made (0 when no level is positive: the map is untouched)."""
    d = _f64(detection_levels)
    if d is not None and d.size != classes:
        raise AnnonetHipError(1, "detection levels need one value per class")
    rounds = C.c_int(-1)
    check(net.L.anh_detection_filter_device(net.h, d_labels_ptr or None, d_blended_ptr or None, classes, height, width, _ptr(d), C.byref(rounds)))
    return rounds.value


def detection_filter(label_map, blended, detection_levels, net=None, prefill_scratch=None):
    """anh_detection_filter_device on host arrays (torch moves the bytes): u16 label map [H,W] and fp32 planes [K,H,W] ->
    (the filtered map, host rounds).  `prefill_scratch` (tests: the filter must not read what an earlier call left): a shape (h, w), or
    True for the map's own; the handle first filters a throwaway map of that shape in which every pixel is a seed, which leaves every
    flag byte of the scratch it covers at 1."""
    import torch
    lab = np.require(label_map, dtype=np.uint16, requirements=["C", "W"])
    planes = np.require(blended, dtype=np.float32, requirements=["C", "W"])
    if lab.ndim != 2 or planes.ndim != 3 or planes.shape[1:] != lab.shape:
        raise AnnonetHipError(1, "detection_filter: a label map [H,W] and planes [K,H,W]")
    net = _net_for_blobs(net)
    H, W = lab.shape
    if prefill_scratch is not None and prefill_scratch is not False:
        h, w = (H, W) if prefill_scratch is True else prefill_scratch
        d_ones = torch.ones(h * w, dtype=torch.int16, device="cuda")           # label 1 everywhere, margin 0 > -1: all seeds
        d_zero = torch.zeros(2 * h * w, dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        detection_filter_device(net, d_ones.data_ptr(), d_zero.data_ptr(), 2, h, w, [1.0, 0.0])
    d_lab = torch.from_numpy(lab.view(np.uint8).reshape(-1)).cuda()
    d_planes = torch.from_numpy(planes).cuda()
    torch.cuda.current_stream().synchronize()
    rounds = detection_filter_device(net, d_lab.data_ptr(), d_planes.data_ptr(), planes.shape[0], H, W, detection_levels)
    return d_lab.cpu().numpy().view(np.uint16).reshape(H, W), rounds


def annonet_infer_regions(net, input_image, gains=None, detection_levels=None, tiling_parameters=None, want_blobs=False, want_blended=False):
    """annonet_infer() plus the region table of its unfiltered label map (anh_infer_regions): returns (label map, table as a numpy
    structured array of REGION_DTYPE), followed by the u32 blob map and the blended planes when asked for."""
    (img,), H, W = _images(net, [input_image])
    g, d = _per_class(net, gains, detection_levels)
    res = np.empty((H, W), np.uint16)
    blobs = np.empty((H, W), np.uint32) if want_blobs else None
    bl = np.empty((net.cfg.classes, H, W), np.float32) if want_blended else None
    table, n = C.POINTER(_lib.Region)(), C.c_size_t()
    check(net.L.anh_infer_regions(net.h, _ptr(img), H, W, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptr(res), _ptr(blobs), _ptr(bl),
                                  C.byref(table), C.byref(n)))
    out = [res, _take_regions(net.L, table, n.value)]
    if want_blobs:
        out.append(blobs)
    if want_blended:
        out.append(bl)
    return tuple(out)


def _take_regions_per_image(L, table, counts):
    """the ONE malloc'd table of a batched regions call -> list of numpy structured arrays, one per image; releases the block"""
    rows = _take_regions(L, table, int(sum(counts)))
    ends = np.cumsum([0] + [int(c) for c in counts])
    return [rows[ends[i]:ends[i + 1]] for i in range(len(counts))]


def label_blobs_batch(label_maps, prefill=None, net=None):
    """anh_label_blobs_batch_device on host u16 label maps [n,H,W]: (u32 blob maps [n,H,W], list of n counts, blobs + 1 each).  Blob
    numbers restart at 1 in every image.  `prefill` as for label_blobs."""
    a = np.require(label_maps, dtype=np.uint16, requirements=["C", "W"])
    if a.ndim != 3 or a.shape[0] < 1:
        raise AnnonetHipError(1, "label_blobs_batch: label maps [n,H,W] with n >= 1")
    net = _net_for_blobs(net)
    counts = (C.c_uint32 * a.shape[0])()

    def launch(s, d, st):
        import torch
        torch.cuda.current_stream().synchronize()
        check(net.L.anh_label_blobs_batch_device(net.h, s, a.shape[0], a.shape[1], a.shape[2], d, counts))
    blobs = _through_device(a, a.shape, np.uint32, prefill, launch)
    return blobs, list(counts)


def regions_batch_device(net, d_labels_ptr, d_blended_ptr, n, classes, height, width, detection_levels=None, apply_filter=False, d_blobs_ptr=0):
    """anh_regions_batch_device on resident buffers (device pointers as ints): the list of the n images' region tables."""
    d = _f64(detection_levels)
    if d is not None and d.size != classes:
        raise AnnonetHipError(1, "detection levels need one value per class")
    table, counts = C.POINTER(_lib.Region)(), (C.c_size_t * max(n, 1))()
    check(net.L.anh_regions_batch_device(net.h, d_labels_ptr, d_blended_ptr, n, classes, height, width, _ptr(d), 1 if apply_filter else 0, d_blobs_ptr or None,
                                         C.byref(table), counts))
    return _take_regions_per_image(net.L, table, list(counts)[:n])


def regions_batch(label_maps, blended, detection_levels=None, apply_filter=False, prefill=None, net=None):
    """anh_regions_batch_device on host arrays (torch moves the bytes): u16 label maps [n,H,W] and fp32 planes [n,K,H,W] ->
    (list of n region tables, u32 blob maps [n,H,W], the label maps as the call leaves them)."""
    import torch
    lab = np.require(label_maps, dtype=np.uint16, requirements=["C", "W"])
    planes = np.require(blended, dtype=np.float32, requirements=["C", "W"])
    if lab.ndim != 3 or lab.shape[0] < 1 or planes.ndim != 4 or planes.shape[:1] + planes.shape[2:] != lab.shape:
        raise AnnonetHipError(1, "regions_batch: label maps [n,H,W] and planes [n,K,H,W]")
    net = _net_for_blobs(net)
    n, H, W = lab.shape
    d_lab = torch.from_numpy(lab.view(np.uint8).reshape(-1)).cuda()
    d_planes = torch.from_numpy(planes).cuda()
    size = n * H * W * 4
    d_blobs = torch.empty(size, dtype=torch.uint8, device="cuda") if prefill is None else torch.full((size,), int(prefill) & 255, dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    tables = regions_batch_device(net, d_lab.data_ptr(), d_planes.data_ptr(), n, planes.shape[1], H, W, detection_levels, apply_filter, d_blobs.data_ptr())
    return tables, d_blobs.cpu().numpy().view(np.uint32).reshape(n, H, W), d_lab.cpu().numpy().view(np.uint16).reshape(n, H, W)


def _score_outputs(n, classes, prefill):
    """per_pixel, per_region [n,K,K] and labelled [n], u64; `prefill`: byte they are filled with before the call (tests: every
    element must be overwritten)"""
    shapes = ((n, classes, classes), (n, classes, classes), (n,))
    if prefill is None:
        return [np.empty(s, np.uint64) for s in shapes]
    return [np.full(int(np.prod(s)) * 8, int(prefill) & 255, np.uint8).view(np.uint64).reshape(s) for s in shapes]


def score_batch_device(net, d_truth_ptr, d_result_ptr, n, classes, height, width, prefill=None):
    """anh_score_batch_device on resident u16 maps [n,H,W] (device pointers as ints), on the handle's stream: (per_pixel [n,K,K],
    per_region [n,K,K], labelled [n]) as u64 arrays, first index ground truth."""
    out = _score_outputs(max(n, 0), max(classes, 0), prefill)
    check(net.L.anh_score_batch_device(net.h, d_truth_ptr or None, d_result_ptr or None, n, classes, height, width, *[_ptr(a) for a in out]))
    return tuple(out)


def score_device(net, d_truth_ptr, d_result_ptr, classes, height, width, prefill=None):
    """anh_score_device on one resident pair of maps: (per_pixel [K,K], per_region [K,K], labelled)."""
    pp, pr, lab = _score_outputs(1, max(classes, 0), prefill)
    check(net.L.anh_score_device(net.h, d_truth_ptr or None, d_result_ptr or None, classes, height, width, _ptr(pp), _ptr(pr), _ptr(lab)))
    return pp[0], pr[0], int(lab[0])


def score_batch(truth_maps, result_maps, classes, prefill=None, net=None):
    """anh_score_batch on host u16 maps [n,H,W] (the library uploads them): (per_pixel [n,K,K], per_region [n,K,K], labelled [n]).
    `net`: the handle whose stream the call runs on (default: a smallest net of the module's own; scoring uses no weights)."""
    t = np.ascontiguousarray(truth_maps, dtype=np.uint16)
    r = np.ascontiguousarray(result_maps, dtype=np.uint16)
    if t.ndim != 3 or t.shape[0] < 1 or r.shape != t.shape:
        raise AnnonetHipError(1, "score_batch: truth and result maps [n,H,W] of one shape with n >= 1")
    net = _net_for_blobs(net)
    n = t.shape[0]
    out = _score_outputs(n, max(classes, 0), prefill)
    check(net.L.anh_score_batch(net.h, _ptrs(list(t), n), _ptrs(list(r), n), n, classes, t.shape[1], t.shape[2], *[_ptr(a) for a in out]))
    return tuple(out)


def score(truth_map, result_map, classes, prefill=None, net=None):
    """anh_score on one host pair of u16 maps [H,W]: (per_pixel [K,K], per_region [K,K], labelled)."""
    t = np.ascontiguousarray(truth_map, dtype=np.uint16)
    r = np.ascontiguousarray(result_map, dtype=np.uint16)
    if t.ndim != 2 or r.shape != t.shape:
        raise AnnonetHipError(1, "score: a truth and a result map [H,W] of one shape")
    net = _net_for_blobs(net)
    pp, pr, lab = _score_outputs(1, max(classes, 0), prefill)
    check(net.L.anh_score(net.h, _ptr(t), _ptr(r), classes, t.shape[0], t.shape[1], _ptr(pp), _ptr(pr), _ptr(lab)))
    return pp[0], pr[0], int(lab[0])


# ---- held-out evaluation: loss sums and confusion counts per window (anh_eval_logits_device, anh_runtime_evaluate*, anh_trainer_evaluate*) ----
EVAL_DTYPE = np.dtype([("loss_sum", np.float64), ("weight_sum", np.float64), ("counted", np.uint64), ("unclassified", np.uint64)])   # anh_eval_image


class EvalResult:
    """What an evaluation call returns: per_image [n] (EVAL_DTYPE), confusion [n,K,K] u64 (first index ground truth) and, where the call
    was asked for it, predicted [n,H,W] u16."""

    def __init__(self, per_image, confusion, predicted=None):
        self.per_image, self.confusion, self.predicted = per_image, confusion, predicted

    def matrix(self):
        return self.confusion.sum(axis=0, dtype=np.uint64)

    def mean_loss(self):
        return float(self.per_image["loss_sum"].sum() / self.per_image["weight_sum"].sum())

    def pixel_accuracy(self):
        return float(np.trace(self.matrix())) / float(self.per_image["counted"].sum())

    def class_iou(self):
        """per class: hits / (pixels of the class in the truth + predicted as the class - hits); nan for a class that never occurs"""
        m = self.matrix().astype(np.float64)
        hits = np.diag(m)
        union = m.sum(axis=1) + m.sum(axis=0) - hits
        return np.where(union > 0, hits / np.where(union > 0, union, 1.0), np.nan)


def _eval_outputs(n, classes, prefill):
    """per_image [n] and confusion [n,K,K]; `prefill`: byte they are filled with before the call (tests: every element is overwritten)"""
    fill = 0 if prefill is None else int(prefill) & 255
    per_image = np.full(max(n, 0) * EVAL_DTYPE.itemsize, fill, np.uint8).view(EVAL_DTYPE)
    confusion = np.full(max(n, 0) * max(classes, 0) ** 2 * 8, fill, np.uint8).view(np.uint64).reshape(max(n, 0), max(classes, 0), max(classes, 0))
    return per_image, confusion


def _eval_gains(gains, classes):
    g = _f64(gains)
    if g is not None and g.size != classes:
        raise AnnonetHipError(1, "gains need one value per class")
    return g


def _eval_samples(samples, labels):
    """host samples as StartTraining takes them -> (image arrays, label arrays, their pointer lists, n, H, W)"""
    n = len(samples)
    if n == 0 or n != len(labels):
        raise AnnonetHipError(1, "samples and labels must be non-empty and of equal length")
    imgs = [np.ascontiguousarray(s, dtype=np.uint8) for s in samples]
    labs = [np.ascontiguousarray(l) for l in labels]
    h, w = imgs[0].shape[:2]
    for im, lb in zip(imgs, labs):
        if im.shape[:2] != (h, w) or lb.shape != (h, w) or lb.itemsize != C.sizeof(_lib.WLabel):
            raise AnnonetHipError(1, "all samples and weighted label images of a call must share one size")
    return imgs, labs, (C.c_void_p * n)(*[im.ctypes.data for im in imgs]), (C.c_void_p * n)(*[lb.ctypes.data for lb in labs]), n, h, w


def eval_logits_device(net, d_logits_ptr, d_labels_ptr, d_weights_ptr, n, classes, height, width, gains=None, d_predicted_ptr=0, prefill=None):
    """anh_eval_logits_device: the tally alone on resident fp32 logits [n,K,H,W], u16 labels [n,H,W] and fp32 weights [n,H,W] (0 = ones),
    device pointers as ints, on the handle's stream -> EvalResult (the predicted maps stay on the device, at d_predicted_ptr)."""
    per_image, confusion = _eval_outputs(n, classes, prefill)
    g = _eval_gains(gains, classes)
    check(net.L.anh_eval_logits_device(net.h, d_logits_ptr or None, d_labels_ptr or None, d_weights_ptr or None, n, classes, height, width, _ptr(g),
                                       _ptr(per_image), _ptr(confusion), d_predicted_ptr or None))
    return EvalResult(per_image, confusion)


def _regions_outputs(out, tables, wanted):
    """(results..., tables) followed by the optional lists that were asked for"""
    return tuple(out) + (tables,) + tuple(arrays for want, arrays in wanted if want)


def annonet_infer_regions_batch(net, input_images, gains=None, detection_levels=None, tiling_parameters=None, want_blobs=False, want_blended=False):
    """annonet_infer_regions over several images of ONE size in one call (anh_infer_regions_batch): returns (list of label maps, list of
    region tables), followed by the list of u32 blob maps and the list of blended planes when asked for.  want_blobs / want_blended may
    also be lists of booleans, one per image (None where not asked for).  Every image's results equal annonet_infer_regions() of that
    image alone, bit for bit."""
    g, d = _per_class(net, gains, detection_levels)
    imgs, H, W = _images(net, input_images)
    n = len(imgs)
    wb, wp = _per_image(want_blobs, n), _per_image(want_blended, n)
    res = _outputs([True] * n, (H, W), np.uint16)
    blobs = _outputs(wb, (H, W), np.uint32)
    bl = _outputs(wp, (net.cfg.classes, H, W), np.float32)
    table, counts = C.POINTER(_lib.Region)(), (C.c_size_t * max(n, 1))()
    check(net.L.anh_infer_regions_batch(net.h, _ptrs(imgs, n), n, H, W, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptrs(res, n),
                                        _ptrs(blobs, n) if any(wb) else None, _ptrs(bl, n) if any(wp) else None, C.byref(table), counts))
    tables = _take_regions_per_image(net.L, table, list(counts)[:n])
    return _regions_outputs([res], tables, [(any(wb) or want_blobs, blobs), (any(wp) or want_blended, bl)])


def annonet_infer_regions_scaled(net, input_image, downscaling_factor, gains=None, detection_levels=None, tiling_parameters=None, want_scaled=False, want_blobs=False,
                                 want_blended=False):
    """annonet_infer_scaled plus the region table of the unfiltered map at the net's resolution (anh_infer_regions_scaled): returns
    (original-size label map, table), followed by the map, the u32 blob map and the blended planes at the net's resolution when asked for."""
    (img,), H, W = _images(net, [input_image])
    g, d = _per_class(net, gains, detection_levels)
    sh, sw = scaled_dims(H, W, downscaling_factor)
    res = np.empty((H, W), np.uint16)
    scaled = np.empty((sh, sw), np.uint16) if want_scaled else None
    blobs = np.empty((sh, sw), np.uint32) if want_blobs else None
    bl = np.empty((net.cfg.classes, sh, sw), np.float32) if want_blended else None
    table, n = C.POINTER(_lib.Region)(), C.c_size_t()
    check(net.L.anh_infer_regions_scaled(net.h, _ptr(img), H, W, downscaling_factor, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptr(res), _ptr(scaled),
                                         _ptr(blobs), _ptr(bl), C.byref(table), C.byref(n)))
    return _regions_outputs([res], _take_regions(net.L, table, n.value), [(want_scaled, scaled), (want_blobs, blobs), (want_blended, bl)])


def annonet_infer_regions_scaled_batch(net, input_images, downscaling_factor, gains=None, detection_levels=None, tiling_parameters=None, want_scaled=False,
                                       want_blobs=False, want_blended=False):
    """annonet_infer_scaled_batch plus the region tables (anh_infer_regions_scaled_batch): returns (list of original-size label maps, list
    of region tables), followed by the lists of maps, u32 blob maps and blended planes at the net's resolution when asked for.  The
    want_* arguments may also be lists of booleans, one per image.  Every image's results equal annonet_infer_regions_scaled() of that
    image alone, bit for bit."""
    g, d = _per_class(net, gains, detection_levels)
    imgs, H, W = _images(net, input_images)
    n = len(imgs)
    sh, sw = scaled_dims(H, W, downscaling_factor) if n else (0, 0)
    ws, wb, wp = _per_image(want_scaled, n), _per_image(want_blobs, n), _per_image(want_blended, n)
    res = _outputs([True] * n, (H, W), np.uint16)
    sc = _outputs(ws, (sh, sw), np.uint16)
    blobs = _outputs(wb, (sh, sw), np.uint32)
    bl = _outputs(wp, (net.cfg.classes, sh, sw), np.float32)
    table, counts = C.POINTER(_lib.Region)(), (C.c_size_t * max(n, 1))()
    check(net.L.anh_infer_regions_scaled_batch(net.h, _ptrs(imgs, n), n, H, W, downscaling_factor, _ptr(g), _ptr(d), _tiling_ref(tiling_parameters), _ptrs(res, n),
                                               _ptrs(sc, n) if any(ws) else None, _ptrs(blobs, n) if any(wb) else None, _ptrs(bl, n) if any(wp) else None,
                                               C.byref(table), counts))
    tables = _take_regions_per_image(net.L, table, list(counts)[:n])
    return _regions_outputs([res], tables, [(any(ws) or want_scaled, sc), (any(wb) or want_blobs, blobs), (any(wp) or want_blended, bl)])


def argmax_device(net, d_blended_ptr, height, width, row0, row1, d_labels_ptr, gains=None):
    """find_label (annonet_infer.cpp:170-185) over rows [row0, row1) of device-resident blended planes."""
    check(net.L.anh_argmax_device(net.h, d_blended_ptr, height, width, row0, row1, _ptr(_f64(gains)), d_labels_ptr))


class TrainingNet(_Profiled):
    """NetPimpl::TrainingNet (annonet_train_main.cpp:396-410)."""
    _is_trainer = 1

    def __init__(self, levels=2, in_channels=3, precision=ANH_BF16, seed=0):
        self.L = _lib.lib()
        self.h = C.c_void_p()
        check(self.L.anh_trainer_create(C.byref(self.h)))
        check(self.L.anh_trainer_set_levels(self.h, levels))
        check(self.L.anh_trainer_set_input_channels(self.h, in_channels))
        check(self.L.anh_trainer_set_precision(self.h, precision))
        check(self.L.anh_trainer_set_seed(self.h, seed))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.anh_trainer_destroy(self.h)
            self.h = None

    @property
    def cfg(self):
        c = NetConfig()
        check(self.L.anh_trainer_config(self.h, C.byref(c)))
        return c

    @property
    def n_params(self):
        c = self.cfg
        return self.L.anh_net_param_count(C.byref(c))

    @property
    def n_running(self):
        c = self.cfg
        return self.L.anh_net_running_count(C.byref(c))

    def GetRequiredInputDimension(self):
        c = self.cfg
        return self.L.anh_required_input_dim(C.byref(c))

    def Initialize(self):
        check(self.L.anh_trainer_initialize(self.h))

    def SetNetWidth(self, scaler, min_filter_count):
        check(self.L.anh_trainer_set_net_width(self.h, scaler, min_filter_count))

    def SetClassCount(self, n):
        check(self.L.anh_trainer_set_class_count(self.h, n))

    def SetLearningRate(self, lr):
        check(self.L.anh_trainer_set_learning_rate(self.h, lr))

    def SetLearningRateShrinkFactor(self, f):
        check(self.L.anh_trainer_set_learning_rate_shrink_factor(self.h, f))

    def SetIterationsWithoutProgressThreshold(self, n):
        check(self.L.anh_trainer_set_iterations_without_progress_threshold(self.h, n))

    def SetPreviousLossValuesDumpAmount(self, n):
        check(self.L.anh_trainer_set_previous_loss_values_dump_amount(self.h, n))

    def SetAllBatchNormalizationRunningStatsWindowSizes(self, n):
        check(self.L.anh_trainer_set_all_bn_running_stats_window_sizes(self.h, n))

    def SetSynchronizationFile(self, path, seconds):
        check(self.L.anh_trainer_set_synchronization_file(self.h, path.encode(), float(seconds)))

    def BeVerbose(self):
        check(self.L.anh_trainer_be_verbose(self.h))

    def set_sgd(self, weight_decay=0.0005, momentum=0.9):
        check(self.L.anh_trainer_set_sgd(self.h, weight_decay, momentum))

    def GetLearningRate(self):
        return self.L.anh_trainer_get_learning_rate(self.h)

    def get_last_loss(self):
        return self.L.anh_trainer_get_last_loss(self.h)

    def step_count(self):
        return self.L.anh_trainer_get_step_count(self.h)

    def StartTraining(self, samples, labels):
        """samples: list of u8 [H,W,C]; labels: list of structured (label, weight) arrays from set_weights()."""
        n = len(samples)
        if n == 0 or n != len(labels):
            raise AnnonetHipError(1, "samples and labels must be non-empty and of equal length")
        imgs = [np.ascontiguousarray(s, dtype=np.uint8) for s in samples]
        labs = [np.ascontiguousarray(l) for l in labels]
        h, w = imgs[0].shape[:2]
        for im, lb in zip(imgs, labs):
            if im.shape[:2] != (h, w) or lb.shape != (h, w) or lb.itemsize != C.sizeof(_lib.WLabel):
                raise AnnonetHipError(1, "all samples and label images of a mini-batch must share one size")
        ip = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        lp = (C.c_void_p * n)(*[lb.ctypes.data for lb in labs])
        check(self.L.anh_trainer_step(self.h, ip, lp, n, h, w))

    # ---- device-resident, data-parallel-friendly form ----
    def StartTrainingOnCrops(self, dataset, specs, dim, class_weight=0.5, image_weight=0.5):
        """StartTraining on crops cut on the device from `dataset` (no host mini-batch)."""
        check(self.L.anh_trainer_step_crops(self.h, dataset.h, Dataset._specs(specs), len(specs), dim, class_weight, image_weight))

    def StartTrainingOnPickedCrops(self, dataset, specs, draws, dim, class_weight=0.5, image_weight=0.5):
        """StartTrainingOnCrops with every rectangle picked on the device from the image's point index (Dataset.prepare)."""
        if len(specs) != len(draws):
            raise AnnonetHipError(1, "one draw per crop spec")
        check(self.L.anh_trainer_step_crops_picked(self.h, dataset.h, Dataset._specs(specs), Dataset._draws(draws), len(specs), dim, class_weight, image_weight))

    def forward_backward_device(self, d_images, d_labels, d_weights, n, h, w, loss_scale_n):
        check(self.L.anh_trainer_forward_backward_device(self.h, d_images, d_labels, d_weights, n, h, w, float(loss_scale_n)))

    def apply_update(self, grad_scale=1.0):
        check(self.L.anh_trainer_apply_update(self.h, float(grad_scale)))

    def grad_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        check(self.L.anh_trainer_grad_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def get_params(self):
        p = np.empty(self.n_params, np.float32)
        r = np.empty(self.n_running, np.float32)
        check(self.L.anh_trainer_get_params(self.h, _ptr(p), p.size, _ptr(r), r.size))
        return p, r

    def set_params(self, params, running):
        p = np.ascontiguousarray(params, dtype=np.float32)
        r = np.ascontiguousarray(running, dtype=np.float32)
        check(self.L.anh_trainer_set_params(self.h, _ptr(p), p.size, _ptr(r), r.size))

    def replicas(self):
        return self.L.anh_handle_replicas(self.h, 1)

    def exchange_stats(self):
        """anh_trainer_exchange_stats as a dict: host time per StartTraining, sampled all-reduce times on replica 0, worker wake-ups."""
        st = _lib.ExchangeStats()
        check(self.L.anh_trainer_exchange_stats(self.h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.ExchangeStats._fields_}

    def reset_exchange_stats(self):
        self.L.anh_trainer_reset_exchange_stats(self.h)

    def replica_params(self, replica):
        p = np.empty(self.n_params, np.float32)
        check(self.L.anh_trainer_replica_params(self.h, replica, _ptr(p), p.size))
        return p

    def get_grads(self):
        g = np.empty(self.n_params, np.float32)
        check(self.L.anh_trainer_get_grads(self.h, _ptr(g), g.size))
        return g

    def get_momentum(self):
        m = np.empty(self.n_params, np.float32)
        check(self.L.anh_trainer_get_momentum(self.h, _ptr(m), m.size))
        return m

    def set_momentum(self, m):
        m = np.ascontiguousarray(m, dtype=np.float32)
        check(self.L.anh_trainer_set_momentum(self.h, _ptr(m), m.size))

    def GetRuntimeNet(self, precision=None):
        h = C.c_void_p()
        check(self.L.anh_trainer_snapshot_runtime(self.h, self.cfg.precision if precision is None else precision, C.byref(h)))
        return RuntimeNet(_handle=h)

    def evaluate(self, samples, labels, precision=None, gains=None, want_predicted=False):
        """anh_trainer_evaluate: RuntimeNet.evaluate with the parameters as they stand after the last step, on the inference net the
        handle keeps for it; the training state is left untouched"""
        imgs, labs, ip, lp, n, h, w = _eval_samples(samples, labels)
        K = self.cfg.classes
        per_image, confusion = _eval_outputs(n, K, None)
        predicted = np.empty((n, h, w), np.uint16) if want_predicted else None
        check(self.L.anh_trainer_evaluate(self.h, self.cfg.precision if precision is None else precision, ip, lp, n, h, w, _ptr(_eval_gains(gains, K)),
                                          _ptr(per_image), _ptr(confusion), _ptr(predicted)))
        return EvalResult(per_image, confusion, predicted)

    def evaluate_device(self, d_images_ptr, d_labels_ptr, d_weights_ptr, n, height, width, precision=None, gains=None, d_predicted_ptr=0, prefill=None):
        """anh_trainer_evaluate_device: the same on windows resident on the trainer's first device (see RuntimeNet.evaluate_device)"""
        K = self.cfg.classes
        per_image, confusion = _eval_outputs(n, K, prefill)
        check(self.L.anh_trainer_evaluate_device(self.h, self.cfg.precision if precision is None else precision, d_images_ptr or None, d_labels_ptr or None,
                                                 d_weights_ptr or None, n, height, width, _ptr(_eval_gains(gains, K)), _ptr(per_image), _ptr(confusion),
                                                 d_predicted_ptr or None))
        return EvalResult(per_image, confusion)

    def save_state(self, path):
        check(self.L.anh_trainer_save_state(self.h, path.encode()))

    def load_state(self, path):
        check(self.L.anh_trainer_load_state(self.h, path.encode()))

    def synchronize(self):
        check(self.L.anh_trainer_synchronize(self.h))

    def set_stream(self, stream_ptr):
        """As RuntimeNet.set_stream: 0 / None = a stream of the handle's own, never the legacy default stream."""
        check(self.L.anh_trainer_set_stream(self.h, stream_ptr or None))

    def stream_ptr(self):
        s = C.c_void_p()
        check(self.L.anh_trainer_get_stream(self.h, C.byref(s)))
        return s.value or 0

    def early_grads(self):
        """first element of the gradient bucket's EARLY part: [first, n_params + 1) is final before backward has finished
        (anh_trainer_early_grads); first > n_params means there is none"""
        first = C.c_int64()
        check(self.L.anh_trainer_early_grads(self.h, C.byref(first)))
        return int(first.value)

    def step_graph_stats(self):
        """(captures, launches) of the captured backward graph (ANH_STEP_GRAPH=1); (0, 0) when off"""
        c, l = C.c_int64(0), C.c_int64(0)
        check(self.L.anh_trainer_step_graph_stats(self.h, C.byref(c), C.byref(l)))
        return int(c.value), int(l.value)

    def wait_early_grads(self, stream_ptr):
        """makes the caller's HIP stream wait until the early part of the bucket is final"""
        check(self.L.anh_trainer_wait_early_grads(self.h, stream_ptr))

    def layer_tensor(self, layer, which=0):
        dims = (C.c_int * 4)()
        check(self.L.anh_trainer_layer_tensor(self.h, layer, which, None, 0, dims))
        out = np.empty(tuple(dims), np.float32)
        check(self.L.anh_trainer_layer_tensor(self.h, layer, which, _ptr(out), out.size, dims))
        return out


# ---- single-layer ops (include/annonet_hip.h "single-layer ops"): kernel-level parity tests and micro-benchmarks ----
def _op_input(x, scale, shift, keep):
    if x is None:
        return None
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    t = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    keep.extend([x, s, t])
    return _lib.OpInput(x.ctypes.data, s.ctypes.data if s is not None else None, t.ctypes.data if t is not None else None)


def _out_dim(desc, n):
    type_, k, stride, pad = desc[:4]
    if stride <= 0:
        return 0  # the library rejects the descriptor
    return (n + 2 * pad - k) // stride + 1 if type_ == 0 else stride * (n - 1) + k - 2 * pad


def op_conv_forward(precision, desc, xa, sa=None, ta=None, xb=None, sb=None, tb=None, filters=None, bias=None):
    """desc = (type, k, stride, pad, cin, cout).  Returns (y [N,Ho,Wo,Cout] fp32, used_mfma)."""
    keep = []
    a = _op_input(xa, sa, ta, keep)
    b = _op_input(xb, sb, tb, keep)
    n, h, w, _ = keep[0].shape
    d = _lib.ConvDesc(*desc)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    y = np.empty((n, _out_dim(desc, h), _out_dim(desc, w), desc[5]), np.float32)
    used = C.c_int(0)
    check(_lib.lib().anh_op_conv_forward(precision, C.byref(d), n, h, w, C.byref(a), C.byref(b) if b is not None else None,
                                         _ptr(f), _ptr(bi), _ptr(y), C.byref(used)))
    return y, bool(used.value)


def op_conv_backward_data(precision, desc, dy, filters, in_hw):
    d = _lib.ConvDesc(*desc)
    g = np.ascontiguousarray(dy, dtype=np.float32)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    n = g.shape[0]
    dx = np.empty((n, in_hw[0], in_hw[1], desc[4]), np.float32)
    used = C.c_int(0)
    check(_lib.lib().anh_op_conv_backward_data(precision, C.byref(d), n, in_hw[0], in_hw[1], _ptr(g), _ptr(f), _ptr(dx), C.byref(used)))
    return dx, bool(used.value)


def op_conv_forward_stats(precision, desc, xa, sa=None, ta=None, xb=None, sb=None, tb=None, filters=None):
    """Forward conv with the fused bn-statistics epilogue.  Returns (y, sums [cout, 2] = (sum y, sum y^2), fused)."""
    keep = []
    a = _op_input(xa, sa, ta, keep)
    b = _op_input(xb, sb, tb, keep)
    n, h, w, _ = keep[0].shape
    d = _lib.ConvDesc(*desc)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    y = np.empty((n, _out_dim(desc, h), _out_dim(desc, w), desc[5]), np.float32)
    sums = np.empty((desc[5], 2), np.float64)
    fused = C.c_int(0)
    check(_lib.lib().anh_op_conv_forward_stats(precision, C.byref(d), n, h, w, C.byref(a), C.byref(b) if b is not None else None,
                                               _ptr(f), _ptr(y), _ptr(sums), C.byref(fused)))
    return y, sums, bool(fused.value)


def op_conv_backward_data_bn(precision, desc, dy, filters, in_hw, y_prev, scale, shift, mean, invstd, dx_init=None):
    """Backward-data conv (+= dx_init) with the fused bn + relu backward reduction of the layer that receives dx.
    Returns (dx, sums [cin, 2] = (sum dz*xhat, sum dz), fused)."""
    d = _lib.ConvDesc(*desc)
    g = np.ascontiguousarray(dy, dtype=np.float32)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    n = g.shape[0]
    arrs = [np.ascontiguousarray(v, dtype=np.float32) for v in (y_prev, scale, shift, mean, invstd)]
    init = None if dx_init is None else np.ascontiguousarray(dx_init, dtype=np.float32)
    dx = np.empty((n, in_hw[0], in_hw[1], desc[4]), np.float32)
    sums = np.empty((desc[4], 2), np.float64)
    fused = C.c_int(0)
    check(_lib.lib().anh_op_conv_backward_data_bn(precision, C.byref(d), n, in_hw[0], in_hw[1], _ptr(g), _ptr(f), _ptr(init),
                                                  *[_ptr(v) for v in arrs], _ptr(dx), _ptr(sums), C.byref(fused)))
    return dx, sums, bool(fused.value)


def op_conv_backward_filter_bn(precision, desc, image_u8, da, y, scale, shift, mean, invstd, coef):
    """Stem filter gradient with dy = bn + relu backward of (da, y) computed while staging.  Returns (dw, in_kernel)."""
    d = _lib.ConvDesc(*desc)
    img = np.ascontiguousarray(image_u8, dtype=np.uint8)
    n, h, w, _ = img.shape
    arrs = [np.ascontiguousarray(v, dtype=np.float32) for v in (da, y, scale, shift, mean, invstd, coef)]
    bn = _lib.OpBnDy(*[v.ctypes.data for v in arrs])
    dw = np.empty(desc[1] * desc[1] * desc[4] * desc[5], np.float32)
    flag = C.c_int(0)
    check(_lib.lib().anh_op_conv_backward_filter_bn(precision, C.byref(d), n, h, w, _ptr(img), C.byref(bn), _ptr(dw), C.byref(flag)))
    return dw, bool(flag.value)


def op_conv_backward_filter(precision, desc, xa, sa=None, ta=None, xb=None, sb=None, tb=None, dy=None):
    keep = []
    a = _op_input(xa, sa, ta, keep)
    b = _op_input(xb, sb, tb, keep)
    n, h, w, _ = keep[0].shape
    d = _lib.ConvDesc(*desc)
    g = np.ascontiguousarray(dy, dtype=np.float32)
    dw = np.empty(desc[1] * desc[1] * desc[4] * desc[5], np.float32)
    used = C.c_int(0)
    check(_lib.lib().anh_op_conv_backward_filter(precision, C.byref(d), n, h, w, C.byref(a), C.byref(b) if b is not None else None,
                                                 _ptr(g), _ptr(dw), C.byref(used)))
    return dw, bool(used.value)


# ---- table mode and the training kernels that are not convolutions (include/annonet_hip.h, tests/test_gpu_train_ops.py) ----
def _f32(a, keep):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    keep.append(a)
    return a.ctypes.data


def _bn_layer(spec, keep):
    """spec: dict(c, pixels, gamma, beta, eps[, sums, running_mean, running_var, af, unbias]) -> (OpBnLayer, outputs dict)"""
    c = int(spec["c"])
    out = {n: np.full(c, np.nan, np.float32) for n in ("mean", "invstd", "scale", "shift")}
    out["var"] = np.full(c, np.nan, np.float64)
    L = _lib.OpBnLayer()
    L.c, L.pixels, L.eps, L.af, L.unbias = c, float(spec["pixels"]), float(spec.get("eps", 1e-4)), float(spec.get("af", 1.0)), float(spec.get("unbias", 1.0))
    if spec.get("sums") is not None:
        sums = np.ascontiguousarray(spec["sums"], dtype=np.float64)
        assert sums.shape == (c, 2)
        keep.append(sums)
        L.sums = sums.ctypes.data
    L.gamma, L.beta = _f32(spec["gamma"], keep), _f32(spec["beta"], keep)
    if spec.get("running_mean") is not None:
        out["running_mean"] = np.array(spec["running_mean"], dtype=np.float32)
        out["running_var"] = np.array(spec["running_var"], dtype=np.float32)
        L.running_mean, L.running_var = out["running_mean"].ctypes.data, out["running_var"].ctypes.data
    for n in ("mean", "invstd", "scale", "shift", "var"):
        setattr(L, n, out[n].ctypes.data)
    return L, out


def op_bn_fold(jobs, spread_seed=1):
    """ONE bn_fold_all launch over up to 16 jobs (dicts as _bn_layer takes, with sums [c, 2] = (sum y, sum y^2)).
    Returns one dict per job: mean, invstd, scale, shift, var[, running_mean, running_var]."""
    keep, outs = [], []
    arr = (_lib.OpBnLayer * len(jobs))()
    for i, j in enumerate(jobs):
        arr[i], o = _bn_layer(j, keep)
        outs.append(o)
    check(_lib.lib().anh_op_bn_fold(arr, len(jobs), spread_seed))
    return outs


def op_bn_forward_stats(precision, y, gamma, beta, eps=1e-4, running_mean=None, running_var=None, af=1.0, unbias=1.0):
    """The partials form: statistics kernel over y [P, C] + finalize.  Returns (arrays dict as op_bn_fold, sums [C, 2])."""
    keep = []
    yy = np.ascontiguousarray(y, dtype=np.float32)
    p, c = yy.shape
    L, out = _bn_layer(dict(c=c, pixels=p, gamma=gamma, beta=beta, eps=eps, running_mean=running_mean, running_var=running_var, af=af, unbias=unbias), keep)
    sums = np.empty((c, 2), np.float64)
    check(_lib.lib().anh_op_bn_forward_stats(precision, _ptr(yy), C.byref(L), _ptr(sums)))
    return out, sums


def _bn_input(spec, keep):
    """spec: dict(x, scale, shift) or dict(x, sums, gamma, beta[, eps]) (table form)"""
    if spec is None:
        return None
    i = _lib.OpBnInput()
    i.x = _f32(spec["x"], keep)
    if spec.get("sums") is not None:
        sums = np.ascontiguousarray(spec["sums"], dtype=np.float64)
        keep.append(sums)
        i.sums, i.gamma, i.beta, i.eps = sums.ctypes.data, _f32(spec["gamma"], keep), _f32(spec["beta"], keep), float(spec.get("eps", 1e-4))
    else:
        i.scale, i.shift = _f32(spec["scale"], keep), _f32(spec["shift"], keep)
    return i


def op_conv_forward_stats_table(precision, desc, a=None, b=None, image=None, filters=None, tables=True):
    """Forward conv with its bn statistics added into a table (tables) or left as partials; a / b as _bn_input takes, or a u8 image (the stem).
    Returns dict(y, sums [cout, 2], poison, ticket, workgroups)."""
    keep = []
    ia, ib = _bn_input(a, keep), _bn_input(b, keep)
    img = None if image is None else np.ascontiguousarray(image, dtype=np.uint8)
    n, h, w, _ = img.shape if img is not None else np.shape(a["x"])
    d = _lib.ConvDesc(*desc)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    y = np.empty((n, _out_dim(desc, h), _out_dim(desc, w), desc[5]), np.float32)
    sums = np.empty((desc[5], 2), np.float64)
    poison, ticket, wgs = C.c_int64(-1), C.c_int64(-1), C.c_int(0)
    check(_lib.lib().anh_op_conv_forward_stats_table(precision, C.byref(d), n, h, w, _ptr(img), C.byref(ia) if ia is not None else None,
                                                     C.byref(ib) if ib is not None else None, _ptr(f), int(bool(tables)), _ptr(y), _ptr(sums),
                                                     C.byref(poison), C.byref(ticket), C.byref(wgs)))
    return dict(y=y, sums=sums, poison=poison.value, ticket=ticket.value, workgroups=wgs.value)


def op_conv_backward_data_bn_table(precision, desc, dy, filters, in_hw, y_prev, scale, shift, mean, invstd, gamma, dx_init=None):
    """op_conv_backward_data_bn with the sums in a table and the finish by the launch's last workgroup.
    Returns dict(dx, sums [cin, 2], dgamma, dbeta, coef [3, cin], ticket, workgroups)."""
    d = _lib.ConvDesc(*desc)
    g = np.ascontiguousarray(dy, dtype=np.float32)
    f = np.ascontiguousarray(filters, dtype=np.float32)
    n, cin = g.shape[0], desc[4]
    arrs = [np.ascontiguousarray(v, dtype=np.float32) for v in (y_prev, scale, shift, mean, invstd, gamma)]
    init = None if dx_init is None else np.ascontiguousarray(dx_init, dtype=np.float32)
    dx = np.empty((n, in_hw[0], in_hw[1], cin), np.float32)
    sums = np.empty((cin, 2), np.float64)
    dgamma, dbeta, coef = np.empty(cin, np.float32), np.empty(cin, np.float32), np.empty((3, cin), np.float32)
    ticket, wgs = C.c_int64(-1), C.c_int(0)
    check(_lib.lib().anh_op_conv_backward_data_bn_table(precision, C.byref(d), n, in_hw[0], in_hw[1], _ptr(g), _ptr(f), _ptr(init), *[_ptr(v) for v in arrs],
                                                        _ptr(dx), _ptr(sums), _ptr(dgamma), _ptr(dbeta), _ptr(coef), C.byref(ticket), C.byref(wgs)))
    return dict(dx=dx, sums=sums, dgamma=dgamma, dbeta=dbeta, coef=coef, ticket=ticket.value, workgroups=wgs.value)


def op_bn_backward(precision, y, mean, invstd, scale, shift, da=None, gamma=None, tables=False, out_of_place=False, stages=7, coef_in=None,
                   head_g=None, head_w_tm=None):
    """bn + relu backward on (da, y) [P, C]: stages & 1 reduce, & 2 finalize, & 4 apply (see anh_op_bn_bwd).
    Returns dict(sums [C, 2], dgamma, dbeta, coef [3, C], dy [P, C], ticket, workgroups)."""
    keep = []
    yy = np.ascontiguousarray(y, dtype=np.float32)
    p, c = yy.shape
    o = _lib.OpBnBwd()
    o.c, o.pixels, o.y = c, p, yy.ctypes.data
    o.da, o.gamma, o.mean, o.invstd, o.scale, o.shift = (_f32(v, keep) for v in (da, gamma, mean, invstd, scale, shift))
    o.coef_in, o.head_g, o.head_w_tm = (_f32(v, keep) for v in (coef_in, head_g, head_w_tm))
    o.head_k = 0 if head_g is None else np.shape(head_g)[1]
    o.tables, o.out_of_place, o.stages = int(bool(tables)), int(bool(out_of_place)), stages
    out = dict(sums=np.full((c, 2), np.nan, np.float64), dgamma=np.empty(c, np.float32), dbeta=np.empty(c, np.float32), coef=np.empty((3, c), np.float32),
               dy=np.full((p, c), np.nan, np.float32))
    for n in ("sums", "dgamma", "dbeta", "coef", "dy"):
        setattr(o, n, out[n].ctypes.data)
    check(_lib.lib().anh_op_bn_backward(precision, C.byref(o)))
    out.update(ticket=o.ticket, workgroups=o.workgroups)
    return out


def op_head_train(precision, a, b, w_tm, bias, labels, weights, scale, da_virtual=False, bn_sums=0, bn_mean=None, bn_invstd=None, bn_gamma=None,
                  fold_jobs=()):
    """The fused tail of a training step (anh_op_head).  a / b as _bn_input takes, x = [P, 32]; w_tm [32, K]; bn_sums 0 / 1 (partials) / 2 (table + finish).
    Returns dict(logits, dlogits [P, K], da [P, 32] or None, loss, dbias, dw [32, K], bn_sums [32, 2], dgamma, dbeta, coef [3, 32], error_flag, ticket,
    workgroups, folds = one dict per fold job)."""
    keep = []
    ia, ib = _bn_input(a, keep), _bn_input(b, keep)
    p = np.shape(a["x"])[0]
    w = np.ascontiguousarray(w_tm, dtype=np.float32)
    k = w.shape[1]
    lab = np.ascontiguousarray(labels, dtype=np.uint16)
    o = _lib.OpHead()
    o.k, o.pixels, o.scale = k, p, float(scale)
    o.a = C.pointer(ia)
    if ib is not None:
        o.b = C.pointer(ib)
    o.w_tm, o.bias, o.labels, o.weights = w.ctypes.data, _f32(bias, keep), lab.ctypes.data, _f32(weights, keep)
    o.da_virtual, o.bn_sums = int(bool(da_virtual)), bn_sums
    o.bn_mean, o.bn_invstd, o.bn_gamma = (_f32(v, keep) for v in (bn_mean, bn_invstd, bn_gamma))
    jobs = (_lib.OpBnLayer * max(len(fold_jobs), 1))()
    folds = []
    for i, j in enumerate(fold_jobs):
        jobs[i], fo = _bn_layer(j, keep)
        folds.append(fo)
    o.fold_jobs, o.n_fold_jobs = jobs, len(fold_jobs)
    out = dict(logits=np.empty((p, k), np.float32), dlogits=np.empty((p, k), np.float32), da=None if da_virtual else np.empty((p, 32), np.float32),
               loss=np.empty(1, np.float64), dbias=np.empty(k, np.float32), dw=np.empty((32, k), np.float32), bn_sums=np.full((32, 2), np.nan, np.float64),
               dgamma=np.empty(32, np.float32), dbeta=np.empty(32, np.float32), coef=np.empty((3, 32), np.float32))
    for n in ("logits", "dlogits", "loss", "dbias", "dw", "dgamma", "dbeta", "coef"):
        setattr(o, n, out[n].ctypes.data)
    o.bn_sums_out = out["bn_sums"].ctypes.data
    if not da_virtual:
        o.da = out["da"].ctypes.data
    check(_lib.lib().anh_op_head_train(precision, C.byref(o)))
    out.update(loss=float(out["loss"][0]), error_flag=o.error_flag, ticket=o.ticket, workgroups=o.workgroups, folds=folds)
    return out


def op_loss(logits, labels, weights, scale):
    """The unfused loss kernel on fp32 logits [P, K].  Returns dict(dlogits, loss, dbias, error_flag)."""
    z = np.ascontiguousarray(logits, dtype=np.float32)
    p, k = z.shape
    lab = np.ascontiguousarray(labels, dtype=np.uint16)
    wgt = np.ascontiguousarray(weights, dtype=np.float32)
    g, loss, dbias, err = np.empty((p, k), np.float32), np.empty(1, np.float64), np.empty(k, np.float32), C.c_int(0)
    check(_lib.lib().anh_op_loss(_ptr(z), _ptr(lab), _ptr(wgt), p, k, float(scale), _ptr(g), _ptr(loss), _ptr(dbias), C.byref(err)))
    return dict(dlogits=g, loss=float(loss[0]), dbias=dbias, error_flag=err.value)
