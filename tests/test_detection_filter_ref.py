"""tests/detection_filter_ref.py on the CPU: the two references of the detection filter agree (expected() labels blobs with scipy and
counts seeds per blob; flood() spreads flags as the device does), the seed plans are what they claim, the hand-made cases have the
answers their descriptions state, and the bound on the flood's rounds over the spiral follows from the map."""
import numpy as np
import pytest
from scipy import ndimage

import blobs_ref as br
import detection_filter_ref as dr

T = dr.T


@pytest.mark.parametrize("c", dr.CASES, ids=dr.case_id)
def test_flood_equals_expected(c):
    lab, planes, levels, want = dr.case(*c)
    got, _ = dr.flood(lab, br.seed_flags(lab, planes, levels))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name,shape", dr.REFERENCE_ORDER_MAPS + [("random", (2 * T, 2 * T))], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_flood_equals_expected_in_reference_order(name, shape):
    lab = dr.pattern(name, shape)
    planes, levels = dr.plan("random", lab, name)
    flags = br.seed_flags(lab, planes, levels, reference_order=True)
    got, _ = dr.flood(lab, flags)
    np.testing.assert_array_equal(got, dr.expected(lab, planes, levels, reference_order=True))
    if name == "random":
        assert (got != dr.expected(lab, planes, levels)).any()     # the order matters on these maps
        assert flags.sum() < br.seed_flags(lab, planes, levels).sum() or shape[0] == shape[1]      # non-square: positions fall outside


@pytest.mark.parametrize("name", sorted(dr.HAND_MADE))
def test_hand_made_cases_have_the_stated_answers(name):
    lab, planes, levels, want, seeds = dr.hand_made(name)
    assert lab.shape == dr.FRAME
    flags = br.seed_flags(lab, planes, levels)
    np.testing.assert_array_equal(flags, seeds)
    np.testing.assert_array_equal(dr.expected(lab, planes, levels), want)
    np.testing.assert_array_equal(dr.flood(lab, flags)[0], want)
    assert (want != lab).any() and (want != 0).any()              # every case removes something and keeps something
    rows, cols = np.nonzero(lab)                                   # ... and straddles a tile seam
    assert rows.min() // T != rows.max() // T or cols.min() // T != cols.max() // T


def test_the_number_format_cases_sit_where_they_claim():
    lab, planes, levels, _, _ = dr.hand_made("equality")
    margin = (planes[1, 31, 33] - planes[0, 31, 33], planes[2, 32, 30] - planes[0, 32, 30])
    assert float(margin[0]) == levels[1] - levels[0] and margin[1] == np.nextafter(np.float32(levels[2] - levels[0]), np.float32(2))
    lab, planes, levels, _, _ = dr.hand_made("float_subtraction")
    y, x = np.argwhere(lab == 1)[0]
    assert float(planes[1, y, x] - planes[0, y, x]) == 16777216.0 < levels[1] < float(planes[1, y, x]) - float(planes[0, y, x]) == 16777217.0
    lab, planes, levels, _, _ = dr.hand_made("double_threshold")
    assert levels[1] - levels[0] == 0.19999999999999998 < float(planes[1, 32, 32]) <= float(np.float32(levels[1]) - np.float32(levels[0]))


@pytest.mark.parametrize("shape", dr.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", dr.PATTERNS)
def test_plans_are_what_they_claim(name, shape):
    lab = dr.pattern(name, shape)
    blobs, count = br.blobs_ref(lab)
    first = np.full(count, lab.size, np.int64)
    np.minimum.at(first, blobs.reshape(-1).astype(np.int64), np.arange(lab.size))
    label_of = lab.reshape(-1)[first[1:]]                         # by blob number - 1
    for plan, K in [("last_pixel", 3), ("first_pixel", 3)] + ([("wide", 8)] if name == "random_wide_values" else []):
        planes, levels = dr.plan(plan, lab, name)
        assert planes.shape == (K,) + shape and planes.dtype == np.float32 and len(levels) == K
        table, _, _ = br.region_table(lab, planes, levels)
        seeded = (np.arange(1, count) % 2 == (1 if plan == "first_pixel" else 0)) & (label_of < K)
        np.testing.assert_array_equal(table["seeds"], seeded.astype(np.int64))      # ONE seed per chosen blob, none elsewhere
        pixel = table["first_row"] * shape[1] + table["first_col"] if plan == "first_pixel" else None
        rows, cols = np.nonzero(br.seed_flags(lab, planes, levels))
        if plan == "first_pixel":
            np.testing.assert_array_equal(np.sort(rows * shape[1] + cols), np.sort(pixel[seeded]))
        else:
            last = np.zeros(count, np.int64)
            np.maximum.at(last, blobs.reshape(-1).astype(np.int64), np.arange(lab.size))
            np.testing.assert_array_equal(np.sort(rows * shape[1] + cols), np.sort(last[1:][seeded]))
        if (label_of < K).sum() >= 2:
            assert seeded.any() and (~seeded & (label_of < K)).any(), plan      # keeps a blob and removes one
        if plan == "wide" and shape[0] * shape[1] > 100:
            assert (table["seeds"][label_of == 7] > 0).any() and not table["seeds"][label_of == 65535].any()
    assert not dr.case(name, shape, "none")[3].any()
    want = dr.case(name, shape, "negative_threshold")[3]
    np.testing.assert_array_equal(want, np.where((lab == 1) | (lab == 2), lab, 0))


def test_random_plan_is_the_blob_tests_own_and_mixed():
    lab, planes, levels, want = dr.case("random", dr.SIZES[-1], "random")
    rng = np.random.default_rng(len("random") + lab.shape[0] * 7 + lab.shape[1])     # test_gpu_blobs.py: case()
    np.testing.assert_array_equal(planes, np.where(np.isnan(planes), np.nan, rng.normal(0, 2, planes.shape).astype(np.float32)))
    assert np.isnan(planes).mean() > 0.03 and levels == (0.0, 3.0, 4.5)
    assert ((want == 0) & (lab != 0)).any() and (want != 0).any()


def test_no_positive_level_leaves_the_map():
    lab, planes, _, _ = dr.case("random", (T - 1, T + 1), "random")
    for levels in (None, [0.0, 0.0, 0.0]):
        np.testing.assert_array_equal(dr.expected(lab, planes, levels), lab)


def test_spiral_needs_a_launch_per_segment_of_its_first_tile():
    """On the spiral with its only seed at one end, flood tile (0,0) can flag its lap j+1 segment only in a launch after the one that
    flagged its lap j segment: inside the tile the two are not connected (they are different 8-connected pieces of the 32 x 32 window),
    the path joins them only by a whole lap through other tiles, and a workgroup loads its halo once per launch.  So launches >=
    segments and, at 4 launches per host round, rounds >= ceil(segments / 4)."""
    lab = dr.pattern("spiral", dr.SIZES[-1])
    assert lab.shape == (97, 130) and int((lab != 0).sum()) == 6418 and br.blobs_ref(lab)[1] == 2
    outer, inner = dr.spiral_ends(lab)
    assert (outer, inner) == ((0, 0), (48, 81))
    segments = dr.tile_segments(lab)
    assert segments == 16 and -(-segments // 4) == 4
    # the pieces are met in order along the path, one full lap apart: walk it from the outer end and note each entry into tile (0,0)
    pieces, _ = ndimage.label(lab[:T, :T] != 0, structure=np.ones((3, 3)))
    order, seen, (y, x), visited = [], set(), outer, np.zeros(lab.shape, bool)
    while True:
        visited[y, x] = True
        if y < T and x < T and pieces[y, x] not in seen:
            seen.add(pieces[y, x])
            order.append(int(pieces[y, x]))
        nxt = [(yy, xx) for yy in range(max(y - 1, 0), min(y + 2, lab.shape[0])) for xx in range(max(x - 1, 0), min(x + 2, lab.shape[1]))
               if lab[yy, xx] and not visited[yy, xx] and (yy == y or xx == x)]
        if not nxt:
            break
        (y, x), = nxt
    assert (y, x) == inner and visited.sum() == 6418 and len(order) == segments
    for seed in (outer, inner):
        seeds = np.zeros(lab.shape, bool)
        seeds[seed] = True
        got, sweeps = dr.flood(lab, seeds)
        np.testing.assert_array_equal(got, lab)
        assert sweeps > 6000                                       # one pixel per sweep, bar the corners a diagonal step cuts
    np.testing.assert_array_equal(dr.flood(lab, np.zeros(lab.shape, bool))[0], 0)
