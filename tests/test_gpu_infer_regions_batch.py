"""Regions for batched and downscaled inference through the net (anh_infer_regions_batch, anh_infer_regions_scaled,
anh_infer_regions_scaled_batch and their mirrors): image i of a call equals, bit for bit, what annonet_infer_regions() returns for that
image alone (for a scaled call: for the shrunk image, the result map blown up nearest-neighbour), and labels and planes equal what
annonet_infer_batch() / annonet_infer_scaled(_batch)() return for the same arguments.  fp32 parity mode: every comparison is equality.
What annonet_infer_regions() itself computes is held against the oracle and blobs_ref in test_gpu_infer_regions.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import annonet_amd as aa
import blobs_ref as br
import png_util as pu
import resize_util as ru
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
ORIGINAL = (80, 112)      # at factor 2: 40 x 56
SHAPE = (40, 56)
FACTOR = 2.0
N = 5


def tp(tiled):
    """2 x 2 tiles on a 40 x 56 image, or the image as one tile"""
    return aa.tiling.parameters(36, 28, 10, 10) if tiled else None


def levels_between_peaks(tables):
    """det[k] strictly between two distinct blob peaks of class k (0 where the class has fewer than two), as test_gpu_infer_regions.py chooses them"""
    det = [0.0] * K
    for k in range(1, K):
        peaks = np.unique(np.concatenate([t["peak"][(t["label"] == k) & np.isfinite(t["peak"])] for t in tables]).astype(np.float64))
        if len(peaks) >= 2:
            m = len(peaks) // 2
            det[k] = float(peaks[m - 1] + peaks[m]) / 2.0
            assert peaks[m - 1] < det[k] < peaks[m]
    return det


@pytest.fixture(scope="module")
def setup():
    p, r = random_params(OracleNet(2, 3, K, 0.25, 4), 21)
    net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    net.set_params(p, r)
    originals = np.random.default_rng(9).integers(0, 256, (N,) + ORIGINAL + (3,), dtype=np.uint8)
    shrunk = np.stack([ru.shrink(img, FACTOR) for img in originals])
    assert shrunk.shape[1:3] == SHAPE and len(aa.tiling.get_tiles(SHAPE[1], SHAPE[0], tp(True))) == 4
    # levels from the single-image call (the reference of this file), so that across the stack some blobs are detected and some removed
    plain = [aa.annonet_infer_regions(net, img, tiling_parameters=tp(True)) for img in shrunk]
    det = levels_between_peaks([t for _, t in plain])
    s = {"net": net, "params": (p, r), "originals": originals, "shrunk": shrunk, "det": det, "cache": {}}
    detected = np.concatenate([single(s, i, True, det)[1]["detected"] for i in range(N)])
    assert max(det) > 0 and (detected == 1).any() and (detected == 0).any()
    return s


def single(s, i, tiled, levels, gains=None):
    """(result, table, blobs, planes) of annonet_infer_regions() on shrunk image i alone: computed once per argument set, never changed"""
    key = (i, tiled, None if levels is None else tuple(levels), None if gains is None else tuple(gains))
    if key not in s["cache"]:
        out = aa.annonet_infer_regions(s["net"], s["shrunk"][i], gains=gains, detection_levels=levels, tiling_parameters=tp(tiled), want_blobs=True, want_blended=True)
        for a in out:
            a.setflags(write=False)
        s["cache"][key] = out
    return s["cache"][key]


def assert_same(got, want, what):
    """(result, table, blobs, planes), bit for bit; a None in `got` was not asked for"""
    for name, g, w in zip(("result", "table", "blobs", "planes"), got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def blown_up(labels):
    return pu.resize_nearest(labels, ORIGINAL[1], ORIGINAL[0])


# ---- 1. annonet_infer_regions_batch against annonet_infer_regions of each image ---------------------------------------------------------
@pytest.mark.parametrize("tiled", [True, False], ids=["tiles2x2", "one_tile"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_regions_batch_equals_the_single_call_image_by_image(setup, n, tiled):
    net, det = setup["net"], setup["det"]
    res, tables, blobs, planes = aa.annonet_infer_regions_batch(net, setup["shrunk"][:n], detection_levels=det, tiling_parameters=tp(tiled), want_blobs=True, want_blended=True)
    labels, label_planes = aa.annonet_infer_batch(net, setup["shrunk"][:n], detection_levels=det, tiling_parameters=tp(tiled), want_blended=True)
    for i in range(n):
        assert_same((res[i], tables[i], blobs[i], planes[i]), single(setup, i, tiled, det), i)
        assert tables[i]["blob"].tolist() == list(range(1, len(tables[i]) + 1))       # the numbers restart at 1 in every image
        assert res[i].tobytes() == labels[i].tobytes() and planes[i].tobytes() == label_planes[i].tobytes()
    # without the optional outputs: the same maps and tables
    only, only_tables = aa.annonet_infer_regions_batch(net, setup["shrunk"][:n], detection_levels=det, tiling_parameters=tp(tiled))
    assert [a.tobytes() for a in only] == [a.tobytes() for a in res] and [t.tobytes() for t in only_tables] == [t.tobytes() for t in tables]


# ---- 2. annonet_infer_regions_scaled -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [True, False], ids=["tiles2x2", "one_tile"])
def test_regions_scaled_equals_regions_of_the_shrunk_image(setup, tiled):
    net, det = setup["net"], setup["det"]
    for i in (0, 3):
        res, table, scaled, blobs, planes = aa.annonet_infer_regions_scaled(net, setup["originals"][i], FACTOR, detection_levels=det, tiling_parameters=tp(tiled),
                                                                            want_scaled=True, want_blobs=True, want_blended=True)
        want = single(setup, i, tiled, det)
        assert_same((scaled, table, blobs, planes), want, i)                         # table and blob map at the net's resolution
        np.testing.assert_array_equal(res, blown_up(want[0]))
        labels, label_scaled, label_planes = aa.annonet_infer_scaled(net, setup["originals"][i], FACTOR, detection_levels=det, tiling_parameters=tp(tiled),
                                                                    want_scaled=True, want_blended=True)
        assert res.tobytes() == labels.tobytes() and scaled.tobytes() == label_scaled.tobytes() and planes.tobytes() == label_planes.tobytes()
        only, only_table = aa.annonet_infer_regions_scaled(net, setup["originals"][i], FACTOR, detection_levels=det, tiling_parameters=tp(tiled))
        assert only.tobytes() == res.tobytes() and only_table.tobytes() == table.tobytes()


# ---- 3. annonet_infer_regions_scaled_batch against both -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tiled", [True, False], ids=["tiles2x2", "one_tile"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_regions_scaled_batch_equals_the_single_calls_image_by_image(setup, n, tiled):
    net, det = setup["net"], setup["det"]
    res, tables, scaled, blobs, planes = aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:n], FACTOR, detection_levels=det, tiling_parameters=tp(tiled),
                                                                               want_scaled=True, want_blobs=True, want_blended=True)
    labels, label_scaled, label_planes = aa.annonet_infer_scaled_batch(net, setup["originals"][:n], FACTOR, detection_levels=det, tiling_parameters=tp(tiled),
                                                                       want_scaled=True, want_blended=True)
    for i in range(n):
        want = single(setup, i, tiled, det)
        assert_same((scaled[i], tables[i], blobs[i], planes[i]), want, i)
        np.testing.assert_array_equal(res[i], blown_up(want[0]))
        assert res[i].tobytes() == labels[i].tobytes() and scaled[i].tobytes() == label_scaled[i].tobytes() and planes[i].tobytes() == label_planes[i].tobytes()
    one = aa.annonet_infer_regions_scaled(net, setup["originals"][n - 1], FACTOR, detection_levels=det, tiling_parameters=tp(tiled), want_scaled=True, want_blobs=True,
                                          want_blended=True)
    assert_same((res[n - 1], tables[n - 1], scaled[n - 1], blobs[n - 1]), (one[0], one[1], one[2], one[3]), "last")


# ---- 4. argument variants ----------------------------------------------------------------------------------------------------------------
def test_factor_one_is_the_unscaled_call(setup):
    net, det, imgs = setup["net"], setup["det"], setup["shrunk"][:3]
    res, table, scaled, blobs, planes = aa.annonet_infer_regions_scaled(net, imgs[1], 1.0, detection_levels=det, tiling_parameters=tp(True), want_scaled=True,
                                                                        want_blobs=True, want_blended=True)
    assert_same((res, table, blobs, planes), single(setup, 1, True, det), "scaled")
    assert scaled.tobytes() == res.tobytes()
    res, tables, scaled, blobs, planes = aa.annonet_infer_regions_scaled_batch(net, imgs, 1.0, detection_levels=det, tiling_parameters=tp(True), want_scaled=True,
                                                                               want_blobs=True, want_blended=True)
    for i in range(3):
        assert_same((res[i], tables[i], blobs[i], planes[i]), single(setup, i, True, det), i)
        assert scaled[i].tobytes() == res[i].tobytes()


@pytest.mark.parametrize("levels", [None, [0.0, 0.0, 0.0]])
def test_without_a_positive_level_nothing_is_removed(setup, levels):
    net = setup["net"]
    res, tables, blobs, planes = aa.annonet_infer_regions_batch(net, setup["shrunk"][:3], detection_levels=levels, tiling_parameters=tp(True), want_blobs=True, want_blended=True)
    sres, stables, sscaled, sblobs = aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:3], FACTOR, detection_levels=levels, tiling_parameters=tp(True),
                                                                           want_scaled=True, want_blobs=True)
    for i in range(3):
        want = single(setup, i, True, levels)
        assert_same((res[i], tables[i], blobs[i], planes[i]), want, i)
        assert_same((sscaled[i], stables[i], sblobs[i]), want, i)
        assert len(tables[i]) > 0 and (tables[i]["detected"] == 1).all()
        np.testing.assert_array_equal(blobs[i], br.blobs_ref(res[i])[0])            # nothing removed: the blobs are those of the result
    one = aa.annonet_infer_regions_scaled(net, setup["originals"][2], FACTOR, detection_levels=levels, tiling_parameters=tp(True), want_scaled=True, want_blobs=True)
    assert_same((one[2], one[1], one[3]), single(setup, 2, True, levels), "scaled")


def test_gains_reach_the_label_maps(setup):
    net, det = setup["net"], setup["det"]
    gains = [0.0, 0.1, -0.05]
    res, tables, blobs = aa.annonet_infer_regions_batch(net, setup["shrunk"][:3], gains=gains, detection_levels=det, tiling_parameters=tp(True), want_blobs=True)
    sres, stables, sscaled = aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:3], FACTOR, gains=gains, detection_levels=det, tiling_parameters=tp(True), want_scaled=True)
    changed = False
    for i in range(3):
        want = single(setup, i, True, det, gains)
        assert_same((res[i], tables[i], blobs[i]), want, i)
        assert_same((sscaled[i], stables[i]), want, i)
        changed = changed or want[0].tobytes() != single(setup, i, True, det)[0].tobytes()
    assert changed, "the gains change no label of these images: the test does not exercise them"


def test_optional_outputs_per_image(setup):
    net, det, n = setup["net"], setup["det"], 4
    wb, wp, ws = [False, True, False, True], [True, False, False, True], [False, False, True, True]
    res, tables, blobs, planes = aa.annonet_infer_regions_batch(net, setup["shrunk"][:n], detection_levels=det, tiling_parameters=tp(True), want_blobs=wb, want_blended=wp)
    sres, stables, sscaled, sblobs, splanes = aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:n], FACTOR, detection_levels=det, tiling_parameters=tp(True),
                                                                                    want_scaled=ws, want_blobs=wb, want_blended=wp)
    for i in range(n):
        want = single(setup, i, True, det)
        assert (blobs[i] is not None) == wb[i] == (sblobs[i] is not None) and (planes[i] is not None) == wp[i] == (splanes[i] is not None) and (sscaled[i] is not None) == ws[i]
        assert_same((res[i], tables[i], blobs[i], planes[i]), want, i)
        assert_same((sscaled[i], stables[i], sblobs[i], splanes[i]), want, i)
        np.testing.assert_array_equal(sres[i], blown_up(want[0]))
    # one list given, the other not at all
    res, tables, blobs = aa.annonet_infer_regions_batch(net, setup["shrunk"][:n], detection_levels=det, tiling_parameters=tp(False), want_blobs=wb)
    for i in range(n):
        assert_same((res[i], tables[i], blobs[i]), single(setup, i, False, det), i)


def test_bad_arguments_are_refused_and_the_handle_stays_usable(setup):
    net, det = setup["net"], setup["det"]
    with pytest.raises(aa.AnnonetHipError) as e:
        aa.annonet_infer_regions_batch(net, setup["shrunk"][:2], detection_levels=[0.0, -1.0, 2.0], tiling_parameters=tp(True))
    assert e.value.code == 1 and "detection levels" in str(e.value)
    with pytest.raises(aa.AnnonetHipError) as e:
        aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:2], -2.0, detection_levels=det)
    assert e.value.code == 1
    with pytest.raises(aa.AnnonetHipError) as e:
        aa.annonet_infer_regions_batch(net, [], detection_levels=det)
    assert e.value.code == 1
    res, tables = aa.annonet_infer_regions_batch(net, setup["shrunk"][:2], detection_levels=det, tiling_parameters=tp(True))
    for i in range(2):
        assert_same((res[i], tables[i]), single(setup, i, True, det), i)


SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import annonet_amd as aa
import blobs_ref as br
det = [0.0, 0.5, 0.25]
rng = np.random.default_rng(3)
lab = rng.integers(0, 3, (3, 41, 67)).astype(np.uint16)          # not square: transposed seeds of the right-hand part fall outside the map
planes = rng.normal(0, 1, (3, 3, 41, 67)).astype(np.float32)
tables, blobs, after = aa.regions_batch(lab, planes, detection_levels=det, apply_filter=True, prefill=0xA5)
differs = False
for i in range(3):
    t, b, a = aa.regions(lab[i], planes[i], detection_levels=det, apply_filter=True, prefill=0xA5)
    assert t.tobytes() == tables[i].tobytes() and b.tobytes() == blobs[i].tobytes() and a.tobytes() == after[i].tobytes(), i
    want, want_blobs, _ = br.region_table(lab[i], planes[i], det, reference_order=True)
    br.assert_table_equal(tables[i], want)
    np.testing.assert_array_equal(after[i], br.filtered(lab[i], want_blobs, want))
    differs = differs or (want["seeds"] != br.region_table(lab[i], planes[i], det)[0]["seeds"]).any()
assert differs, "both lookups agree on these maps: the test does not exercise the switch"
'''


def test_reference_seed_order_switch_reaches_the_batched_seeds():
    env = dict(os.environ)
    env["ANH_DET_SEED_REFERENCE_ORDER"] = "1"      # read once per process: a process of its own
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- 5. two replicas ---------------------------------------------------------------------------------------------------------------------
def test_two_replicas(setup):
    det = setup["det"]
    aa.set_devices([0, 0])
    try:
        net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    finally:
        aa.set_devices([])
    assert net.L.anh_handle_replicas(net.h, 0) == 2
    net.set_params(*setup["params"])
    for n in (3, 1):      # n >= R: replica r serves anh_shard_range(n, 2, r) and the host concatenates the tables; n < R: image by image on replica 0
        for levels in (det, None):
            res, tables, blobs, planes = aa.annonet_infer_regions_batch(net, setup["shrunk"][:n], detection_levels=levels, tiling_parameters=tp(True), want_blobs=True,
                                                                        want_blended=True)
            sres, stables, sscaled, sblobs = aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:n], FACTOR, detection_levels=levels, tiling_parameters=tp(True),
                                                                                   want_scaled=True, want_blobs=True)
            for i in range(n):
                want = single(setup, i, True, levels)
                assert_same((res[i], tables[i], blobs[i], planes[i]), want, (n, i))
                assert_same((sscaled[i], stables[i], sblobs[i]), want, (n, i))
                np.testing.assert_array_equal(sres[i], blown_up(want[0]))
    one = aa.annonet_infer_regions_scaled(net, setup["originals"][1], FACTOR, detection_levels=det, tiling_parameters=tp(True), want_scaled=True, want_blobs=True,
                                          want_blended=True)
    assert_same((one[2], one[1], one[3], one[4]), single(setup, 1, True, det), "scaled")


# ---- 6. call structure -------------------------------------------------------------------------------------------------------------------
def launched(net, fn):
    net.profile_enable(True)
    try:
        net.profile_reset()
        fn()
        return net.profile_launch_order(), {e["name"]: e["launches"] for e in net.profile()}
    finally:
        net.profile_enable(False)


@pytest.mark.parametrize("tiled", [True, False], ids=["tiles2x2", "one_tile"])
def test_a_regions_batch_is_the_batch_forward_then_a_tail_that_does_not_grow_with_n(setup, tiled):
    net, det = setup["net"], setup["det"]
    tails = {}
    for n in (2, 5):
        imgs = setup["shrunk"][:n]
        inner, _ = launched(net, lambda: aa.annonet_infer_batch(net, imgs, tiling_parameters=tp(tiled), want_blended=True))
        order, count = launched(net, lambda: aa.annonet_infer_regions_batch(net, imgs, detection_levels=det, tiling_parameters=tp(tiled)))
        assert inner and order[:len(inner)] == inner                              # begins with the launches of annonet_infer_batch
        tails[n] = order[len(inner):]
        assert "label_blobs" not in count and "blob_regions" not in count         # no image went through the single-image kernels
        sorder, scount = launched(net, lambda: aa.annonet_infer_regions_scaled_batch(net, setup["originals"][:n], FACTOR, detection_levels=det, tiling_parameters=tp(tiled)))
        assert sorder == order + ["resize_labels_nearest"] and scount["resize_image_bilinear"] == 1 and scount["resize_labels_nearest"] == 1
    assert tails[2] == tails[5] == ["label_blobs_batch", "blob_regions_batch"]   # the same launches after the forward for 2 and for 5 images
    # the single scaled form keeps the single-image tail
    inner, _ = launched(net, lambda: aa.annonet_infer(net, setup["shrunk"][0], tiling_parameters=tp(tiled), want_blended=True))
    order, _ = launched(net, lambda: aa.annonet_infer_regions_scaled(net, setup["originals"][0], FACTOR, detection_levels=det, tiling_parameters=tp(tiled)))
    assert order == inner + ["label_blobs", "blob_regions", "resize_labels_nearest"]


# ---- 7. the C++ drop-in header -----------------------------------------------------------------------------------------------------------
def test_cpp_header_regions_batch_forms(tmp_path, setup):
    net, det, n = setup["net"], setup["det"], 3
    H, W = ORIGINAL
    exe = str(tmp_path / "regions_batch_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regions_batch_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "net.bin").write_bytes(net.Serialize())
    imgs = setup["originals"][:n]
    (tmp_path / "images.raw").write_bytes(imgs.tobytes())
    # the unscaled form sees the originals with 72 x 56 tiles (2 x 2 of them), the scaled forms the same cap on the shrunk images (one tile)
    r = subprocess.run([exe, str(tmp_path / "net.bin"), str(tmp_path / "images.raw"), str(n), str(H), str(W), "2", "72", "56", ",".join(repr(v) for v in det),
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    t = aa.tiling.parameters(72, 56, 10, 10)
    assert len(aa.tiling.get_tiles(W, H, t)) == 4
    lines = [line.split() for line in r.stdout.splitlines()]

    def read(form, what, dtype, shape):
        return np.frombuffer((tmp_path / ("out.%s.%s.raw" % (form, what))).read_bytes(), dtype).reshape(shape)
    res, tables, blobs = aa.annonet_infer_regions_batch(net, imgs, detection_levels=det, tiling_parameters=t, want_blobs=True)
    assert lines[0] == ["batch", str(n), str(H), str(W)] + [str(len(x)) for x in tables]
    np.testing.assert_array_equal(read("batch", "labels", np.uint16, (n, H, W)), np.stack(res))
    np.testing.assert_array_equal(read("batch", "blobs", np.uint32, (n, H, W)), np.stack(blobs))
    assert (tmp_path / "out.batch.regions.raw").read_bytes() == b"".join(x.tobytes() for x in tables)
    res, table, scaled, blobs = aa.annonet_infer_regions_scaled(net, imgs[0], FACTOR, detection_levels=det, tiling_parameters=t, want_scaled=True, want_blobs=True)
    assert lines[1] == ["scaled", "1", str(SHAPE[0]), str(SHAPE[1]), str(len(table))]
    np.testing.assert_array_equal(read("scaled", "labels", np.uint16, (H, W)), res)
    np.testing.assert_array_equal(read("scaled", "scaled", np.uint16, SHAPE), scaled)
    np.testing.assert_array_equal(read("scaled", "blobs", np.uint32, SHAPE), blobs)
    assert (tmp_path / "out.scaled.regions.raw").read_bytes() == table.tobytes()
    res, tables, scaled, blobs = aa.annonet_infer_regions_scaled_batch(net, imgs, FACTOR, detection_levels=det, tiling_parameters=t, want_scaled=True, want_blobs=True)
    assert lines[2] == ["sbatch", str(n), str(SHAPE[0]), str(SHAPE[1])] + [str(len(x)) for x in tables]
    np.testing.assert_array_equal(read("sbatch", "labels", np.uint16, (n, H, W)), np.stack(res))
    np.testing.assert_array_equal(read("sbatch", "scaled", np.uint16, (n,) + SHAPE), np.stack(scaled))
    np.testing.assert_array_equal(read("sbatch", "blobs", np.uint32, (n,) + SHAPE), np.stack(blobs))
    assert (tmp_path / "out.sbatch.regions.raw").read_bytes() == b"".join(x.tobytes() for x in tables)
    assert sum(len(x) for x in tables) > 0
