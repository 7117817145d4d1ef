"""The detection-level filter every annonet_infer form runs (det_seed_kernel, det_flood_kernel and its host loop, det_apply_kernel),
on GIVEN label maps through anh_detection_filter_device: the map it leaves equals tests/detection_filter_ref.py: expected() bit for
bit, and equals what the one-launch filter of anh_regions_device leaves.  The maps are chosen around the flood's 32-pixel tiles and
its 34 x 34 window (seams, four-tile corners, ragged last tiles, 1 x N, one long chain), the seed plans around what a flood can get
wrong (a seed only on a blob's last or first pixel, none, all, labels >= K), the hand-made cases around the seed comparison's number
formats.  The handle's scratch is left full of set flags before most calls."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import annonet_amd as aa
import detection_filter_ref as dr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = dr.T
LEVELS = [0.0, 0.5, 0.5]


def seeded_at(lab, pixels):
    planes = np.zeros((3,) + lab.shape, np.float32)
    for p in pixels:
        planes[(int(lab[p]),) + p] = 1.0
    return planes


@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_patterns_sizes_plans(c):
    lab, planes, levels, want = dr.case(*c)
    got, rounds = aa.detection_filter(lab, planes, levels, prefill_scratch=True)
    np.testing.assert_array_equal(got, want)
    assert rounds >= 1
    _, _, after = aa.regions(lab, planes, detection_levels=levels, apply_filter=True)     # the blob path's filter: the same map
    np.testing.assert_array_equal(after, got)


@pytest.mark.parametrize("name", sorted(dr.HAND_MADE))
def test_hand_made_cases(name):
    lab, planes, levels, want, _ = dr.hand_made(name)
    np.testing.assert_array_equal(dr.expected(lab, planes, levels), want)
    got, _ = aa.detection_filter(lab, planes, levels, prefill_scratch=True)
    np.testing.assert_array_equal(got, want)


def test_spiral_with_one_seed():
    """rounds >= ceil(segments / 4), segments = the 8-connected pieces of the path inside tile (0,0): a workgroup loads its halo once
    per launch, and the next piece is a whole lap through other tiles away (tests/test_detection_filter_ref.py)"""
    lab = dr.pattern("spiral", dr.SIZES[-1])
    segments = dr.tile_segments(lab)
    assert segments >= 8
    for end in dr.spiral_ends(lab):
        got, rounds = aa.detection_filter(lab, seeded_at(lab, [end]), LEVELS, prefill_scratch=True)
        np.testing.assert_array_equal(got, lab)                   # the whole path survives
        print("spiral seeded at %s: %d rounds (bound %d)" % (end, rounds, -(-segments // 4)))
        assert rounds >= -(-segments // 4)
    got, rounds = aa.detection_filter(lab, seeded_at(lab, []), LEVELS, prefill_scratch=True)
    assert not got.any()
    assert rounds == 1                                            # one quiet round ends the loop


def test_no_positive_level_and_bad_arguments():
    lab, planes, _, _ = dr.case("random", (T + 1, T - 1), "random")
    net = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
    for levels in (None, np.zeros(3), [0, 0, 0]):
        got, rounds = aa.detection_filter(lab, planes, levels, net=net, prefill_scratch=True)
        assert got.tobytes() == lab.tobytes() and rounds == 0
    H, W = lab.shape
    d_lab = torch.from_numpy(lab.view(np.int16).copy()).cuda()
    d_planes = torch.from_numpy(planes.copy()).cuda()
    torch.cuda.synchronize()
    for args in ((d_lab.data_ptr(), d_planes.data_ptr(), 3, H, W, [0.0, -1.0, 1.0]),       # a negative level
                 (0, d_planes.data_ptr(), 3, H, W, LEVELS), (d_lab.data_ptr(), 0, 3, H, W, LEVELS),   # null pointers
                 (d_lab.data_ptr(), d_planes.data_ptr(), 0, H, W, []),                     # no classes
                 (d_lab.data_ptr(), d_planes.data_ptr(), 3, 0, W, LEVELS), (d_lab.data_ptr(), d_planes.data_ptr(), 3, H, 0, LEVELS)):
        with pytest.raises(aa.AnnonetHipError):
            aa.detection_filter_device(net, *args)
    assert d_lab.cpu().numpy().view(np.uint16).tobytes() == lab.tobytes()     # a refused call touches nothing
    _, _, levels, want = dr.case("random", (T + 1, T - 1), "random")
    got, rounds = aa.detection_filter(lab, planes, levels, net=net)           # the handle still works
    np.testing.assert_array_equal(got, want)
    assert rounds >= 1


def test_dirty_scratch_on_one_handle():
    net = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
    big = dr.pattern("random", (200, 300))
    planes, levels = dr.plan("random", big, "random")
    want = dr.expected(big, planes, levels)
    assert ((want == 0) & (big != 0)).any() and want.any()
    first, _ = aa.detection_filter(big, planes, levels, net=net)
    np.testing.assert_array_equal(first, want)
    for c in dr.CASES:
        if c[1] == (T - 1, T + 1):
            lab, p, lv, w = dr.case(*c)
            np.testing.assert_array_equal(aa.detection_filter(lab, p, lv, net=net)[0], w, err_msg=dr.case_id(c))
    second, _ = aa.detection_filter(big, planes, levels, net=net)
    np.testing.assert_array_equal(second, want)
    assert first.tobytes() == second.tobytes()


@pytest.mark.parametrize("name,plan", [("random", "random"), ("random", "last_pixel"), ("random_wide_values", "random"), ("random_wide_values", "wide")])
def test_unaligned_maps_through_the_device_form(name, plan):
    """image i of a batch with an odd plane: the map starts on a 2-byte boundary only, the planes on a 4-byte one"""
    shape = (T + 1, T - 1)
    lab, planes, levels, want = dr.case(name, shape, plan)
    H, W = shape
    n, K = H * W, planes.shape[0]
    assert n % 2 == 1
    net = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
    aligned, rounds = aa.detection_filter(lab, planes, levels, net=net)
    fill = np.int16(np.uint16(0xA5A5).view(np.int16))
    d_lab = torch.full((n + 3,), int(fill), dtype=torch.int16, device="cuda")          # one element before the map, two after it
    d_lab[1:n + 1] = torch.from_numpy(lab.view(np.int16).reshape(-1).copy()).cuda()
    d_planes = torch.full((K * n + 2,), 7.0, dtype=torch.float32, device="cuda")
    d_planes[1:K * n + 1] = torch.from_numpy(planes.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    assert (d_lab.data_ptr() + 2) % 4 == 2 and (d_planes.data_ptr() + 4) % 8 == 4
    assert aa.detection_filter_device(net, d_lab.data_ptr() + 2, d_planes.data_ptr() + 4, K, H, W, levels) == rounds
    out = d_lab.cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(out[1:n + 1].reshape(shape), aligned)
    np.testing.assert_array_equal(aligned, want)
    assert out[0] == 0xA5A5 and (out[n + 1:] == 0xA5A5).all()
    flat = d_planes.cpu().numpy()
    assert flat[0] == 7.0 and flat[-1] == 7.0 and flat[1:-1].tobytes() == planes.tobytes()


def test_large_smooth_map_twice():
    shape = (1000, 1500)
    lab = dr.smooth_map(shape, 11)
    rng = np.random.default_rng(12)
    planes = ndimage.gaussian_filter(rng.normal(0, 3, (3,) + shape), (0, 2.0, 2.0)).astype(np.float32)     # test_gpu_blobs.py's
    planes[:, rng.random(shape) < 0.01] = np.nan
    levels = [0.0, 0.8, 0.6]
    want = dr.expected(lab, planes, levels)
    assert ((want == 0) & (lab != 0)).any() and ((want != 0) & (want != 65535)).any()
    a, rounds_a = aa.detection_filter(lab, planes, levels)
    b, rounds_b = aa.detection_filter(lab, planes, levels, prefill_scratch=True)
    print("smooth map of %d x %d: %d and %d rounds" % (shape + (rounds_a, rounds_b)))
    assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(a, want)


def test_reference_seed_order(tmp_path):
    """ANH_DET_SEED_REFERENCE_ORDER=1 (read once per process: a child): the seed marks the blob that holds the TRANSPOSED pixel, and on
    a non-square map the positions that fall outside are dropped"""
    out = str(tmp_path / "reference_order.npz")
    env = dict(os.environ, ANH_DET_SEED_REFERENCE_ORDER="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "run_detection_filter.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    differs = 0
    for name, shape in dr.REFERENCE_ORDER_MAPS:
        lab = dr.pattern(name, shape)
        planes, levels = dr.plan("random", lab, name)
        key = "%s_%dx%d" % ((name,) + shape)
        np.testing.assert_array_equal(got[key], dr.expected(lab, planes, levels, reference_order=True), err_msg=key)
        plain, _ = aa.detection_filter(lab, planes, levels)
        np.testing.assert_array_equal(plain, dr.expected(lab, planes, levels), err_msg=key)
        differs += int((plain != got[key]).any())
    assert differs >= 1, "both seed orders agree on every map: the switch is not exercised"
