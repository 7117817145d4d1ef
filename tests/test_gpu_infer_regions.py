"""annonet_infer() with its region table (anh_infer_regions and its mirrors) through the net: the label map equals annonet_infer()'s and
the oracle's, the blob map equals tests/blobs_ref.py of the UNFILTERED map (annonet_infer.cpp:217 labels before :229-238 filter) and the
table equals a numpy computation from the returned planes.  fp32 parity mode: every comparison is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import annonet_amd as aa
import blobs_ref as br
from conftest import random_params
from oracle.oracle import OracleNet

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
OV = 35   # TrainingNet::GetRequiredInputDimension() of a 2-level net
SHAPE = (150, 130)
IMAGE_SEED = 4


def tp():
    return aa.tiling.parameters(96, 96, OV, OV)


def image():
    return np.random.default_rng(IMAGE_SEED).integers(0, 256, SHAPE + (3,), dtype=np.uint8)


def levels_between_peaks(labels, planes):
    """det[k] strictly between two distinct blob peaks of class k (0 where the class has fewer than two), from the given map and planes"""
    table, _, _ = br.region_table(labels, planes)
    det = [0.0] * K
    for k in range(1, K):
        peaks = np.unique(table["peak"][(table["label"] == k) & np.isfinite(table["peak"])].astype(np.float64))
        if len(peaks) >= 2:
            m = len(peaks) // 2
            det[k] = float(peaks[m - 1] + peaks[m]) / 2.0
            assert peaks[m - 1] < det[k] < peaks[m]
    return det


@pytest.fixture(scope="module")
def setup():
    o = OracleNet(2, 3, K, 0.25, 4)
    p, r = random_params(o, 21)
    o.params[:], o.running[:] = p, r
    net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    net.set_params(p, r)
    img = image()
    plain, planes = o.infer(img, max_tile=(96, 96), overlap=OV, want_blended=True)
    det = levels_between_peaks(plain, planes)
    # on the oracle's numbers alone: the levels keep at least one blob and remove at least one
    want, _, _ = br.region_table(plain, planes, det)
    assert max(det) > 0 and (want["detected"] == 1).any() and (want["detected"] == 0).any()
    filtered = o.infer(img, detection_levels=det, max_tile=(96, 96), overlap=OV)
    assert (filtered != plain).any() and (filtered != 0).any()
    return {"o": o, "net": net, "params": (p, r), "img": img, "plain": plain, "planes": planes, "det": det, "filtered": filtered}


def test_result_blobs_and_table_with_detection_levels(setup):
    net, img, det = setup["net"], setup["img"], setup["det"]
    result, table, blobs, planes = aa.annonet_infer_regions(net, img, detection_levels=det, tiling_parameters=tp(), want_blobs=True, want_blended=True)
    np.testing.assert_array_equal(result, aa.annonet_infer(net, img, detection_levels=det, tiling_parameters=tp()))
    np.testing.assert_array_equal(result, setup["filtered"])
    plain = aa.annonet_infer(net, img, tiling_parameters=tp())
    np.testing.assert_array_equal(plain, setup["plain"])
    want_blobs, want_count = br.blobs_ref(plain)
    assert blobs.dtype == np.uint32 and len(table) == want_count - 1
    np.testing.assert_array_equal(blobs, want_blobs)            # the blobs of the UNFILTERED map: removed blobs keep their numbers
    assert planes.tobytes() == setup["planes"].tobytes()
    want, _, _ = br.region_table(plain, planes, det)
    br.assert_table_equal(table, want)
    np.testing.assert_array_equal(result, br.filtered(plain, want_blobs, want))
    assert (table["detected"] == 1).any() and (table["detected"] == 0).any()
    # without the optional outputs: the same map and table
    only, only_table = aa.annonet_infer_regions(net, img, detection_levels=det, tiling_parameters=tp())
    np.testing.assert_array_equal(only, result)
    assert only_table.tobytes() == table.tobytes()


@pytest.mark.parametrize("levels", [None, [0.0, 0.0, 0.0]])
def test_without_a_positive_level_nothing_is_removed(setup, levels):
    net, img = setup["net"], setup["img"]
    result, table, blobs, planes = aa.annonet_infer_regions(net, img, detection_levels=levels, tiling_parameters=tp(), want_blobs=True, want_blended=True)
    np.testing.assert_array_equal(result, aa.annonet_infer(net, img, detection_levels=levels, tiling_parameters=tp()))
    np.testing.assert_array_equal(result, setup["plain"])
    assert len(table) > 0 and (table["detected"] == 1).all()
    want, want_blobs, _ = br.region_table(result, planes, levels)
    np.testing.assert_array_equal(blobs, want_blobs)
    br.assert_table_equal(table, want)


def test_gains_reach_the_label_map(setup):
    net, img, det = setup["net"], setup["img"], setup["det"]
    gains = [0.0, 0.1, 0.0]
    result, table, blobs = aa.annonet_infer_regions(net, img, gains=gains, detection_levels=det, tiling_parameters=tp(), want_blobs=True)
    np.testing.assert_array_equal(result, aa.annonet_infer(net, img, gains=gains, detection_levels=det, tiling_parameters=tp()))
    np.testing.assert_array_equal(result, setup["o"].infer(img, gains=gains, detection_levels=det, max_tile=(96, 96), overlap=OV))
    np.testing.assert_array_equal(blobs, br.blobs_ref(aa.annonet_infer(net, img, gains=gains, tiling_parameters=tp()))[0])


SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import annonet_amd as aa
import test_gpu_infer_regions as t
from conftest import random_params
from oracle.oracle import OracleNet
o = OracleNet(2, 3, t.K, 0.25, 4)
p, r = random_params(o, 21)
net = aa.RuntimeNet(aa.net_config(2, 3, t.K, 0.25, 4, aa.ANH_FP32))
net.set_params(p, r)
img = t.image()
det = [float(v) for v in sys.argv[3].split(",")]
result, table, blobs, planes = aa.annonet_infer_regions(net, img, detection_levels=det, tiling_parameters=t.tp(), want_blobs=True, want_blended=True)
np.savez(sys.argv[2], result=result, table=table, blobs=blobs, planes=planes, infer=aa.annonet_infer(net, img, detection_levels=det, tiling_parameters=t.tp()),
         plain=aa.annonet_infer(net, img, tiling_parameters=t.tp()))
'''


def test_reference_seed_order_switch(tmp_path, setup):
    out = str(tmp_path / "reference.npz")
    env = dict(os.environ)
    env["ANH_DET_SEED_REFERENCE_ORDER"] = "1"      # read once per process: a process of its own
    r = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, out, ",".join(repr(v) for v in setup["det"])], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    np.testing.assert_array_equal(got["result"], got["infer"])          # both filters honour the switch, on a non-square image
    np.testing.assert_array_equal(got["plain"], setup["plain"])
    want, want_blobs, _ = br.region_table(got["plain"], got["planes"], setup["det"], reference_order=True)
    np.testing.assert_array_equal(got["blobs"], want_blobs)
    br.assert_table_equal(got["table"], want)
    np.testing.assert_array_equal(got["result"], br.filtered(got["plain"], want_blobs, want))
    assert (got["result"] != setup["filtered"]).any(), "both lookups agree on this image: the test does not exercise the switch"


def test_two_replicas(setup):
    one, img, det = setup["net"], setup["img"], setup["det"]
    aa.set_devices([0, 0])
    try:
        net = aa.RuntimeNet(aa.net_config(2, 3, K, 0.25, 4, aa.ANH_FP32))
    finally:
        aa.set_devices([])
    assert net.L.anh_handle_replicas(net.h, 0) == 2
    net.set_params(*setup["params"])
    for levels in (det, None):       # the call runs on replica 0 whatever the levels: the outputs of the one-replica handle
        want = aa.annonet_infer_regions(one, img, detection_levels=levels, tiling_parameters=tp(), want_blobs=True, want_blended=True)
        got = aa.annonet_infer_regions(net, img, detection_levels=levels, tiling_parameters=tp(), want_blobs=True, want_blended=True)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1].tobytes() == want[1].tobytes()
        np.testing.assert_array_equal(got[2], want[2])
        assert got[3].tobytes() == want[3].tobytes()


def test_cpp_header_annonet_infer_regions(tmp_path, setup):
    net, img, det = setup["net"], setup["img"], setup["det"]
    exe = str(tmp_path / "regions_shim")
    lib = os.path.join(ROOT, "annonet_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "regions_shim.cpp"),
                           "-o", exe, "-L" + lib, "-lannonet_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    (tmp_path / "net.bin").write_bytes(net.Serialize())
    (tmp_path / "image.raw").write_bytes(img.tobytes())
    r = subprocess.run([exe, str(tmp_path / "net.bin"), str(tmp_path / "image.raw"), str(SHAPE[0]), str(SHAPE[1]), ",".join(repr(v) for v in det), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    result, table, blobs, planes = aa.annonet_infer_regions(net, img, detection_levels=det, tiling_parameters=tp(), want_blobs=True, want_blended=True)
    assert r.stdout.split() == [str(SHAPE[0]), str(SHAPE[1]), str(SHAPE[0]), str(SHAPE[1]), str(len(table)), "56"]
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.labels.raw").read_bytes(), np.uint16).reshape(SHAPE), result)
    np.testing.assert_array_equal(np.frombuffer((tmp_path / "out.blobs.raw").read_bytes(), np.uint32).reshape(SHAPE), blobs)
    assert (tmp_path / "out.regions.raw").read_bytes() == table.tobytes()
    assert (tmp_path / "out.planes.raw").read_bytes() == planes.tobytes()
