"""The host logic of batched inference over equal-sized images (anh_infer_batch_plan) and the argument checks of anh_infer_batch that
need no GPU.  The plan concatenates the images' tile lists image by image and cuts every run of equal windows into as few batches as
the cap allows, of sizes that differ by at most one."""
import ctypes as C

import pytest

import annonet_amd as aa

LEVELS = 2
OV = 20
ANH_ERR_INVALID = 1


def grid(col_widths, row_heights):
    """a hand-made row-major tile list (full = unique rectangles): the plan only looks at the full rectangles' sizes"""
    out, top = [], 0
    for h in row_heights:
        left = 0
        for w in col_widths:
            rect = (left, top, left + w - 1, top + h - 1)
            out.append((rect, rect))
            left += w
        top += h
    return out


def tiles_of(name):
    if name == "1x1":
        return aa.tiling.get_tiles(61, 45, aa.tiling.parameters(1024, 1024, OV, OV))
    if name == "2x3":     # the tiler's own 2 rows x 3 columns: all windows equal
        return aa.tiling.get_tiles(150, 100, aa.tiling.parameters(64, 64, OV, OV))
    return grid([64, 64, 40], [64, 30])   # ragged 3 columns x 2 rows: the last column and the last row are smaller (runs of 2, 1, 2, 1)


def window(tile):
    (l, t, r, b), _ = tile
    fw, fh = r - l + 1, b - t + 1
    return aa.RuntimeNet.GetRecommendedInputDimension(LEVELS, fh), aa.RuntimeNet.GetRecommendedInputDimension(LEVELS, fw)


def infer_device_batches(tiles, cap):
    """Engine::infer_device's rule on one image's list: runs of equal windows, ceil(run / cap) batches of ceil(run / batches) tiles.
    It leaves a run's remainder to the last batch, where the plan spreads it over the first ones (25 tiles at a cap of 8: 7+7+7+4 here,
    7+6+6+6 in the plan); the two agree on the lists of this file because every run in them has at most 6 tiles."""
    out, i = [], 0
    while i < len(tiles):
        run = 1
        while i + run < len(tiles) and window(tiles[i + run]) == window(tiles[i]):
            run += 1
        n_batches = -(-run // cap)
        per = -(-run // n_batches)
        for done in range(0, run, per):
            out.append([(0, i + j) for j in range(done, min(run, done + per))])
        i += run
    return out


def test_the_tilings_are_what_the_names_say():   # a guard on this file's fixtures only: it exercises nothing of the feature
    assert len(tiles_of("1x1")) == 1
    assert len(tiles_of("2x3")) == 6 and len({window(t) for t in tiles_of("2x3")}) == 1
    assert len(tiles_of("ragged3x2")) == 6 and len({window(t) for t in tiles_of("ragged3x2")}) == 4


@pytest.mark.parametrize("cap", [1, 8, 16])
@pytest.mark.parametrize("n", [1, 2, 5, 17, 40])
@pytest.mark.parametrize("name", ["1x1", "2x3", "ragged3x2"])
def test_batch_plan(name, n, cap):
    tiles = tiles_of(name)
    plan = aa.infer_batch_plan(tiles, n, LEVELS, cap)
    flat = [s for b in plan for s in b]
    assert flat == [(i, t) for i in range(n) for t in range(len(tiles))]      # every pair once, image-major, list order
    wins = [window(tiles[t]) for _, t in flat]
    at, runs = 0, []                                                          # runs of equal windows over the concatenation
    for b in plan:
        assert 1 <= len(b) <= cap
        assert len({window(tiles[t]) for _, t in b}) == 1
    while at < len(wins):
        end = at
        while end < len(wins) and wins[end] == wins[at]:
            end += 1
        runs.append((at, end))
        at = end
    pos, k = 0, 0
    for lo, hi in runs:                                                       # no batch crosses a run; per run: the fewest batches, sizes within one
        sizes = []
        while pos < hi:
            assert pos + len(plan[k]) <= hi
            sizes.append(len(plan[k]))
            pos += len(plan[k])
            k += 1
        assert len(sizes) == -(-(hi - lo) // cap)
        assert max(sizes) - min(sizes) <= 1
    assert k == len(plan)
    if n == 1:      # (holds for runs whose sizes infer_device's rule keeps within one: see infer_device_batches)
        assert plan == infer_device_batches(tiles, cap)


def test_a_batch_may_span_image_boundaries():
    plan = aa.infer_batch_plan(tiles_of("2x3"), 3, LEVELS, 8)      # 18 equal windows: 6 + 6 + 6 would do, and so would any split
    assert [len(b) for b in plan] == [6, 6, 6]
    plan = aa.infer_batch_plan(tiles_of("2x3"), 5, LEVELS, 16)     # 30 windows: 15 + 15, the first batch ends inside image 2
    assert [len(b) for b in plan] == [15, 15]
    assert plan[0][-1] == (2, 2) and plan[1][0] == (2, 3)


def test_bad_plan_arguments_are_errors():
    tiles = tiles_of("1x1")
    for n, cap in ((0, 8), (1, 0)):
        with pytest.raises(aa.AnnonetHipError):
            aa.infer_batch_plan(tiles, n, LEVELS, cap)


def test_infer_batch_rejects_an_empty_batch_and_a_null_list_without_a_gpu():
    L = aa.lib()
    image = (C.c_uint8 * 48)()
    result = (C.c_uint16 * 16)()
    images = (C.c_void_p * 1)(C.addressof(image))
    results = (C.c_void_p * 1)(C.addressof(result))
    def message():
        return L.anh_last_error().decode()
    assert L.anh_infer_batch(None, images, 0, 4, 4, None, None, None, results, None) == ANH_ERR_INVALID and "at least one image" in message()
    assert L.anh_infer_batch(None, images, -3, 4, 4, None, None, None, results, None) == ANH_ERR_INVALID and "at least one image" in message()
    assert L.anh_infer_batch(None, None, 1, 4, 4, None, None, None, results, None) == ANH_ERR_INVALID and "null image or result list" in message()
    assert L.anh_infer_batch(None, images, 1, 4, 4, None, None, None, None, None) == ANH_ERR_INVALID and "null image or result list" in message()
    assert L.anh_infer_batch_device(None, None, 0, 4, 4, None, None, None, None) == ANH_ERR_INVALID and "at least one image" in message()
