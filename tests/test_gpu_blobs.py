"""Connected blobs on the device, the kernels alone (anh_label_blobs_device, anh_regions_device): blob map AND count equal
tests/blobs_ref.py exactly, on maps chosen around the labelling's 32-pixel tiles (T): one tile, partial tiles, several tiles, blobs that
meet only across a seam or a tile corner, one long chain, one blob over everything.  The blob map is prefilled with 0xA5 so that an
element no kernel writes shows.  The region table equals a numpy computation from blobs_ref and the planes, field by field."""
import numpy as np
import pytest
from scipy import ndimage

import annonet_amd as aa
import blobs_ref as br
from blobs_ref import PATTERNS, SIZES, T, pattern, smooth_map

pytestmark = pytest.mark.gpu

K = 3
_cache = {}


def case(name, shape):
    """(label map, planes, reference table without levels, reference blob map, count): computed once per case"""
    key = (name, shape)
    if key not in _cache:
        lab = pattern(name, shape)
        rng = np.random.default_rng(len(name) + shape[0] * 7 + shape[1])
        planes = rng.normal(0, 2, (K,) + shape).astype(np.float32)
        planes[rng.random((K,) + shape) < 0.05] = np.nan
        lab.setflags(write=False)
        planes.setflags(write=False)
        _cache[key] = (lab, planes) + br.region_table(lab, planes)
    return _cache[key]


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_blob_map_and_count_equal_the_reference(name, shape):
    lab, _, _, want, want_count = case(name, shape)
    got, count = aa.label_blobs(lab, prefill=0xA5)
    assert count == want_count
    np.testing.assert_array_equal(got, want)


def test_patterns_are_what_they_claim():
    big = SIZES[-1]
    assert case("spiral", big)[4] == 2 and case("spiral", big)[0].sum() > big[0] * big[1] // 3      # ONE blob, long
    assert case("checkerboard", big)[4] == 3 and case("full", big)[4] == 2 and case("zeros", big)[4] == 1
    lab, _, table, _, count = case("u_shape", big)
    assert count == 2 and (table["first_row"][0], table["first_col"][0]) == (5, big[1] - 3)        # the later arm's tile holds the root
    lab, _, _, blobs, count = case("corner_diagonals", big)
    assert blobs[T - 1, T - 1] == blobs[T, T] != 0 and blobs[T - 1, T] == blobs[T, T - 1] != 0 and blobs[T - 1, T] != blobs[T, T]


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_region_table_equals_numpy(name, shape):
    lab, planes, want, want_blobs, _ = case(name, shape)
    table, blobs, after = aa.regions(lab, planes, prefill=0xA5)
    np.testing.assert_array_equal(blobs, want_blobs)
    br.assert_table_equal(table, want)
    np.testing.assert_array_equal(after, lab)            # no filter asked for: the map is untouched
    assert (table["detected"] == 1).all()


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_region_filter_equals_numpy(name, shape):
    lab, planes, _, want_blobs, _ = case(name, shape)
    levels = [0.0, 3.0, 4.5]
    want, _, _ = br.region_table(lab, planes, levels)
    table, blobs, after = aa.regions(lab, planes, detection_levels=levels, apply_filter=True, prefill=0xA5)
    np.testing.assert_array_equal(blobs, want_blobs)      # the blob map keeps the numbers of the removed blobs
    br.assert_table_equal(table, want)
    np.testing.assert_array_equal(after, br.filtered(lab, want_blobs, want))
    kept, _, untouched = aa.regions(lab, planes, detection_levels=levels, apply_filter=False)
    br.assert_table_equal(kept, want)
    np.testing.assert_array_equal(untouched, lab)


def test_filter_removes_and_keeps_something():
    lab, planes, _, blobs, _ = case("random", SIZES[-1])
    want, _, _ = br.region_table(lab, planes, [0.0, 3.0, 4.5])
    assert (want["seeds"] == 0).any() and (want["seeds"] > 0).any()
    assert np.isneginf(case("random_wide_values", SIZES[-1])[2]["peak"]).any()      # labels 7 and 65535 are >= K


def test_large_smooth_map_twice():
    shape = (1000, 1500)
    lab = smooth_map(shape, 11)
    rng = np.random.default_rng(12)
    planes = ndimage.gaussian_filter(rng.normal(0, 3, (K,) + shape), (0, 2.0, 2.0)).astype(np.float32)
    planes[:, rng.random(shape) < 0.01] = np.nan
    levels = [0.0, 0.8, 0.6]
    want, want_blobs, want_count = br.region_table(lab, planes, levels)
    assert want_count > 50 and (want["seeds"] == 0).any() and (want["seeds"] > 0).any()
    first = aa.label_blobs(lab, prefill=0xA5)
    second = aa.label_blobs(lab, prefill=0x00)
    assert first[1] == second[1] == want_count
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[0], want_blobs)
    t1, b1, a1 = aa.regions(lab, planes, detection_levels=levels, apply_filter=True, prefill=0xA5)
    t2, b2, a2 = aa.regions(lab, planes, detection_levels=levels, apply_filter=True, prefill=0x00)
    assert t1.tobytes() == t2.tobytes()                    # integer atomics: the same bits on every run
    np.testing.assert_array_equal(b1, b2)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(b1, want_blobs)
    br.assert_table_equal(t1, want)
    np.testing.assert_array_equal(a1, br.filtered(lab, want_blobs, want))
