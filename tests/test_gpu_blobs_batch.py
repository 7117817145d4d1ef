"""Connected blobs over a stack of label maps, the blob kernels alone (anh_label_blobs_batch_device, anh_regions_batch_device): every
image of a stack [n,H,W] gets the count, the blob map, the table rows and the filtered map that tests/blobs_ref.py gives that image
alone, and, bit for bit, what the single-image calls return for it.  The shapes sit where a batched form can go wrong: planes of 1023,
1024, 1025, 4095 and 4096 pixels (the 1024-pixel blocks of flatten / rank and the 4096-pixel blocks of the statistics launch must not
straddle two images), one row, one column, several 32 x 32 tiles with ragged edges.  Blob maps are prefilled with 0xA5 so that an
element no kernel writes shows.  A single map is a stack of one on the same path: the last test runs single maps between stacks on one
handle, so that every call finds the shared scratch laid out for another n and another size."""
import numpy as np
import pytest

import annonet_amd as aa
import blobs_ref as br

pytestmark = pytest.mark.gpu

T = 32          # kBlobTile (annonet_amd/csrc/kernels.h)
K = 3
SHAPES = [(31, 33), (25, 41), (32, 32), (64, 64), (63, 65), (1, 70), (70, 1), (97, 130)]
COUNTS = [1, 2, 3, 5]
LEVELS = [0.0, 3.0, 4.5]
# The two patterns a stack is built from, by kind.  A stack of n: zeros first, in the middle and last as far as n has room for them
# (n = 3: zeros, a, zeros; n = 5: zeros, a, zeros, b, zeros; n = 2: zeros, a; n = 1: a), so every stack of two or more mixes images with
# different blob counts and every block boundary between two images has an empty plane on one side and a busy one on the other.
KINDS = {"random": ("random", "random_wide_values"), "chains": ("spiral", "corner_diagonals"), "solid": ("checkerboard", "u_shape")}


def spiral(h, w):
    """a one-pixel path that winds inwards from (0, 0) and leaves one pixel of background between its turns: ONE blob, one long chain"""
    a = np.zeros((h, w), np.uint16)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1
    failed = 0
    while failed < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead_free = not (0 <= fy < h and 0 <= fx < w) or a[fy, fx] == 0
        if 0 <= ny < h and 0 <= nx < w and a[ny, nx] == 0 and ahead_free:
            y, x = ny, nx
            a[y, x] = 1
            failed = 0
        else:
            dy, dx = dx, -dy
            failed += 1
    return a


def pattern(name, shape, seed=0):
    """the patterns of test_gpu_blobs.py"""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + 7919 * seed)
    if name == "random":
        return rng.integers(0, 3, shape).astype(np.uint16)
    if name == "random_wide_values":
        return rng.choice(np.array([0, 1, 2, 7, 65535], np.uint16), size=shape, p=[0.3, 0.25, 0.25, 0.1, 0.1])
    if name == "checkerboard":          # every colour is ONE blob through its diagonals
        yy, xx = np.mgrid[0:h, 0:w]
        return (1 + (yy + xx) % 2).astype(np.uint16)
    if name == "corner_diagonals":      # pairs that touch only across the corner where four tiles meet, and a diagonal through every tile corner
        a = np.zeros(shape, np.uint16)
        for (y, x, v) in ((T - 1, T - 1, 1), (T, T, 1), (T - 1, T, 2), (T, T - 1, 2)):
            if y < h and x < w:
                a[y, x] = v
        for i in range(min(h, w)):
            if a[i, i] == 0 and i not in (T - 1, T):
                a[i, i] = 3
        return a
    if name == "spiral":
        return spiral(h, w)
    if name == "full":
        return np.full(shape, 2, np.uint16)
    if name == "u_shape":               # arms in different tile columns that meet only in the last row
        a = np.zeros(shape, np.uint16)
        left, right = min(3, w - 1), max(w - 3, 0)
        a[min(5, h - 1):, right] = 1
        a[min(9, h - 1):, left] = 1
        a[h - 1, left:right + 1] = 1
        return a
    if name == "zeros":
        return np.zeros(shape, np.uint16)
    raise KeyError(name)


def planes_for(n, shape, seed):
    rng = np.random.default_rng(seed)
    planes = rng.normal(0, 2, (n, K) + shape).astype(np.float32)
    planes[rng.random((n, K) + shape) < 0.05] = np.nan
    return planes


_cache = {}


def stack(kind, n, shape):
    """(label maps [n,H,W], planes [n,K,H,W], per image: reference table without levels, blob map, count): computed once, read-only"""
    key = (kind, n, shape)
    if key not in _cache:
        a, b = KINDS[kind]
        names = {1: [a], 2: ["zeros", a], 3: ["zeros", a, "zeros"], 5: ["zeros", a, "zeros", b, "zeros"]}[n]
        lab = np.stack([pattern(name, shape, seed=i) for i, name in enumerate(names)])
        planes = planes_for(n, shape, len(kind) + 31 * n + shape[0] * 7 + shape[1])
        lab.setflags(write=False)
        planes.setflags(write=False)
        _cache[key] = (lab, planes, [br.region_table(lab[i], planes[i]) for i in range(n)])
    return _cache[key]


def ids(s):
    return "%dx%d" % s


def check_against_reference(lab, planes, levels=None):
    """one batched call with and one without the filter: counts, blob maps, rows and filtered maps against blobs_ref, image by image"""
    n = lab.shape[0]
    tables, blobs, after = aa.regions_batch(lab, planes, detection_levels=levels, apply_filter=True, prefill=0xA5)
    kept, blobs2, untouched = aa.regions_batch(lab, planes, detection_levels=levels, apply_filter=False, prefill=0xA5)
    np.testing.assert_array_equal(untouched, lab)
    np.testing.assert_array_equal(blobs2, blobs)
    positive = levels is not None and max(levels) > 0
    for i in range(n):
        want, want_blobs, want_count = br.region_table(lab[i], planes[i], levels)
        assert len(tables[i]) == want_count - 1, i
        np.testing.assert_array_equal(blobs[i], want_blobs, err_msg="image %d" % i)      # numbers restart at 1 in every image
        br.assert_table_equal(tables[i], want)
        assert kept[i].tobytes() == tables[i].tobytes()
        np.testing.assert_array_equal(after[i], br.filtered(lab[i], want_blobs, want) if positive else lab[i], err_msg="image %d" % i)
        if not positive:
            assert (tables[i]["detected"] == 1).all()
    return tables, blobs, after


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_blob_maps_and_counts_equal_the_reference(kind, n, shape):
    lab, _, want = stack(kind, n, shape)
    got, counts = aa.label_blobs_batch(lab, prefill=0xA5)
    assert counts == [w[2] for w in want]
    for i in range(n):
        np.testing.assert_array_equal(got[i], want[i][1], err_msg="image %d" % i)
        single, count = aa.label_blobs(lab[i], prefill=0xA5)
        assert count == counts[i] and single.tobytes() == got[i].tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_region_tables_and_filter_equal_the_reference_and_the_single_calls(kind, n, shape):
    lab, planes, _ = stack(kind, n, shape)
    check_against_reference(lab, planes)
    tables, blobs, after = check_against_reference(lab, planes, LEVELS)
    for i in range(n):      # bit for bit what the single-image call gives the map
        t, b, a = aa.regions(lab[i], planes[i], detection_levels=LEVELS, apply_filter=True, prefill=0xA5)
        assert t.tobytes() == tables[i].tobytes(), i
        assert b.tobytes() == blobs[i].tobytes() and a.tobytes() == after[i].tobytes(), i


def test_stacks_are_what_they_claim():
    for n in COUNTS:
        lab, planes, want = stack("random", n, SHAPES[-1])
        counts = [w[2] for w in want]
        if n >= 3:
            assert counts[0] == counts[-1] == 1 and (n < 5 or counts[2] == 1)      # zeros first and last, and in the middle of five
        if n >= 2:
            assert len(set(counts)) >= 2                                 # images of different blob counts in one stack
    lab, planes, _ = stack("random", 5, SHAPES[-1])
    seeds = np.concatenate([br.region_table(lab[i], planes[i], LEVELS)[0]["seeds"] for i in range(5)])
    assert (seeds == 0).any() and (seeds > 0).any()                      # the filter keeps a blob and removes one somewhere in the stack


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("n", [2, 3])
def test_images_never_merge(n, shape):
    h, w = shape
    # (a) every image ends in a full row of label 1 and the next begins with one (the two rows of an image joined down its first column):
    # one blob each, each numbered 1
    rows = np.zeros((n,) + shape, np.uint16)
    rows[:, 0, :] = 1
    rows[:, h - 1, :] = 1
    rows[:, :, 0] = 1
    # (b) one blob over every image
    full = np.stack([pattern("full", shape)] * n)
    # (c) the last column of a row and the first column of the next carry the same label, and nothing else does
    # (linear neighbours that are no neighbours in the plane), the last pixel of an image and the first of the next included
    wrap = np.zeros((n,) + shape, np.uint16)
    wrap[:, 0::2, w - 1] = 1
    wrap[:, 1::2, 0] = 1
    wrap[:, 0, 0] = 1
    wrap[:, h - 1, w - 1] = 1
    for name, lab, blobs_per_image in (("rows", rows, 1), ("full", full, 1), ("wrap", wrap, None)):
        planes = planes_for(n, shape, 5)
        tables, blobs, _ = check_against_reference(lab, planes, LEVELS)
        for i in range(n):
            if blobs_per_image is not None:
                assert len(tables[i]) == blobs_per_image, (name, i)
                assert tables[i]["blob"].tolist() == [1] and set(np.unique(blobs[i])) <= {0, 1}, (name, i)
        if name == "wrap" and w > 2 and h > 1:      # what the map is for: (0, w - 1) and (1, 0) are linear neighbours and different blobs
            assert all(b[0, w - 1] != 0 and b[1, 0] != 0 and b[0, w - 1] != b[1, 0] for b in blobs)


def test_one_stack_twice_gives_the_same_bits():
    lab, planes, _ = stack("random", 5, SHAPES[-1])
    t1, b1, a1 = aa.regions_batch(lab, planes, detection_levels=LEVELS, apply_filter=True, prefill=0xA5)
    t2, b2, a2 = aa.regions_batch(lab, planes, detection_levels=LEVELS, apply_filter=True, prefill=0x00)
    assert [t.tobytes() for t in t1] == [t.tobytes() for t in t2]          # integer atomics: the same bits on every run
    assert b1.tobytes() == b2.tobytes() and a1.tobytes() == a2.tobytes()
    first = aa.label_blobs_batch(lab, prefill=0xA5)
    second = aa.label_blobs_batch(lab, prefill=0x00)
    assert first[1] == second[1] and first[0].tobytes() == second[0].tobytes()


# ---- one handle, calls whose reservations lay the shared scratch out differently ----
def layout_cases():
    """[(label maps [n,H,W], planes [n,K,H,W], stacked)] in call order: a stack of 3, then single maps of 2 x 3 ragged tiles, of one tile
    (no seam launch) and of one pixel, then the stack again.  Read-only, computed once."""
    if "layout" not in _cache:
        big = (40, 70)
        first = np.stack([br.pattern("random", big), br.pattern("random_wide_values", big), br.smooth_map(big, 3)])
        singles = [br.pattern("random", (33, 65))[None], br.pattern("random_wide_values", (32, 32))[None], np.ones((1, 1, 1), np.uint16)]
        out = []
        for i, (lab, stacked) in enumerate([(first, True)] + [(s, False) for s in singles]):
            planes = planes_for(lab.shape[0], lab.shape[1:], 100 + i)
            if lab.shape[1:] == (1, 1):
                planes = np.array([0.0, 5.0, 0.0], np.float32).reshape(1, K, 1, 1)      # a margin above its level: the pixel's blob is kept
            lab.setflags(write=False)
            planes.setflags(write=False)
            out.append((lab, planes, stacked))
        _cache["layout"] = out + out[:1]
    return _cache["layout"]


def test_layout_cases_are_what_they_claim():
    cases = layout_cases()
    assert [c[0].shape for c in cases] == [(3, 40, 70), (1, 33, 65), (1, 32, 32), (1, 1, 1), (3, 40, 70)]
    kept = removed = 0
    for lab, planes, _ in cases:
        for i in range(lab.shape[0]):
            table, _, count = br.region_table(lab[i], planes[i], LEVELS)
            assert count >= 2                                     # no map is all background
            kept += int((table["seeds"] > 0).sum())
            removed += int((table["seeds"] == 0).sum())
            if lab[i].size > 1:
                assert (table["seeds"] > 0).any() and (table["seeds"] == 0).any()      # the filter keeps a blob and removes one in every map
    assert kept and removed


@pytest.mark.parametrize("levels", [LEVELS, None], ids=["levels", "no_levels"])
def test_single_maps_between_stacks_on_one_handle(levels):
    """A single-image call is a stack of one on the scratch the previous call laid out for another n and another size: an offset or a
    count left by that layout must not be read."""
    net = aa.RuntimeNet(aa.net_config(1, 3, 3, 0.25, 4, aa.ANH_FP32))
    positive = levels is not None
    for step, (lab, planes, stacked) in enumerate(layout_cases()):
        if stacked:
            tables, blobs, after = aa.regions_batch(lab, planes, detection_levels=levels, apply_filter=True, prefill=0xA5, net=net)
        else:
            t, b, a = aa.regions(lab[0], planes[0], detection_levels=levels, apply_filter=True, prefill=0xA5, net=net)
            tables, blobs, after = [t], b[None], a[None]
        for i in range(lab.shape[0]):
            want, want_blobs, want_count = br.region_table(lab[i], planes[i], levels)
            assert len(tables[i]) == want_count - 1, (step, i)
            np.testing.assert_array_equal(blobs[i], want_blobs, err_msg="step %d image %d" % (step, i))
            br.assert_table_equal(tables[i], want)
            np.testing.assert_array_equal(after[i], br.filtered(lab[i], want_blobs, want) if positive else lab[i], err_msg="step %d image %d" % (step, i))
