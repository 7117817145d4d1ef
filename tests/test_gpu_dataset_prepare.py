"""Dataset preparation and crop-centre sampling on the device (anh_dataset_prepare, anh_dataset_pick, the _picked crop and training
calls): the two label filters against tests/dataset_ref.py and the library's own host anh_ignore_large_nonzero_regions, bit for bit;
the point index against np.flatnonzero; the rectangles against anh_random_rect_containing_point; picked crops and training steps
against the existing device-crop path given the reference's rectangles."""
import numpy as np
import pytest

import annonet_amd as aa
import dataset_ref as ref

pytestmark = pytest.mark.gpu

INF = float("inf")
IGNORE = aa.LABEL_IGNORE
RF = 5                                   # receptive-field side of the size-filter cases
BY_AREA, BY_WIDTH, BY_HEIGHT = 4.0, 6.0, 6.0   # -> 100 pixels, 30 columns, 30 rows


def block_map(rng, h, w, classes):
    """the 7 x 7-block label maps of test_gpu_crops.make_dataset, 5 % ignore pixels"""
    coarse = rng.integers(0, classes, ((h + 6) // 7 + 1, (w + 6) // 7 + 1))
    lab = np.kron(coarse, np.ones((7, 7), dtype=np.int64))[:h, :w].astype(np.uint16)
    lab[rng.random((h, w)) < 0.05] = IGNORE
    return lab


def plant(lab, top, left, height, width, value):
    """a solid rectangle of `value` inside a one-pixel moat of background, where it fits; -> whether it was planted"""
    h, w = lab.shape
    if top + height > h or left + width > w:
        return False
    lab[max(top - 1, 0):top + height + 1, max(left - 1, 0):left + width + 1] = 0
    lab[top:top + height, left:left + width] = value
    return True


def size_filter_map(rng, h, w):
    """blobs that cross the 32-pixel tile seams and corners of the labelling, and, where the map has room: label 5 too large by area only
    (11 x 11 over the tile corner at (32, 32)), 6 by width only, 7 by height only, 8 with exactly by_area * rf^2 pixels, a large region
    of the ignore label"""
    lab = block_map(rng, h, w, 4)
    planted = {}
    planted[5] = plant(lab, 27, 27, 11, 11, 5)
    planted[6] = plant(lab, 50 if h > 50 else 0, 20, 1, 40, 6)
    planted[7] = plant(lab, 10, 100 if w > 100 else 0, 40, 1, 7)
    planted[8] = plant(lab, 60, 60, 10, 10, 8)
    planted[IGNORE] = plant(lab, 80, 150, 40, 40, IGNORE)
    return lab, planted


def dataset_of(lab, channels=3, rng=None):
    ds = aa.Dataset(channels)
    h, w = lab.shape
    img = np.zeros((h, w) if channels == 1 else (h, w, channels), np.uint8) if rng is None else \
        rng.integers(0, 256, (h, w) if channels == 1 else (h, w, channels), dtype=np.uint8)
    assert ds.add(img, lab) == 0
    return ds, img


def check_info(info, lab):
    classes, counts = ref.present_classes(lab)
    assert info["classes"] == classes and info["counts"] == counts


@pytest.mark.parametrize("h,w", [(33, 97), (70, 45), (1, 200), (200, 1), (130, 260)])
def test_size_filter_matches_the_host_routine(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    lab, planted = size_filter_map(rng, h, w)
    want, want_ignored = aa.ignore_large_nonzero_regions(lab, RF, BY_AREA, BY_WIDTH, BY_HEIGHT)
    if (h, w) == (130, 260):
        assert all(planted.values())          # the large map holds every special blob, and the host routine decides them as intended
        assert not (want == 5).any() and not (want == 6).any() and not (want == 7).any() and (want == 8).sum() == 100
    assert want_ignored > 0 or min(h, w) == 1
    ds, _ = dataset_of(lab)
    info = ds.prepare(0, (), BY_AREA, BY_WIDTH, BY_HEIGHT, RF)
    got = ds.labels(0, lab.shape)
    np.testing.assert_array_equal(got, want)
    assert info["ignored_by_size"] == want_ignored and info["ignored_by_class"] == 0      # the ignore-label region is not counted
    check_info(info, want)
    again = ds.prepare(0, (), BY_AREA, BY_WIDTH, BY_HEIGHT, RF)                            # on the labels as they now stand: nothing left to do
    assert again["ignored_by_size"] == 0 and again["classes"] == info["classes"] and again["counts"] == info["counts"]
    np.testing.assert_array_equal(ds.labels(0, lab.shape), want)


@pytest.mark.parametrize("limits", [(BY_AREA, INF, INF), (INF, BY_WIDTH, INF), (INF, INF, BY_HEIGHT), (0.0, INF, INF), (1.0 / 3.0, 7.0 / 3.0, 2.2)])
def test_size_filter_single_limits_and_fractions(limits):
    rng = np.random.default_rng(77)
    lab, _ = size_filter_map(rng, 130, 260)
    want, want_ignored = aa.ignore_large_nonzero_regions(lab, 7, *limits)
    ds, _ = dataset_of(lab)
    info = ds.prepare(0, (), *limits, 7)
    np.testing.assert_array_equal(ds.labels(0, lab.shape), want)
    assert info["ignored_by_size"] == want_ignored
    check_info(info, want)


def test_infinite_limits_leave_the_map_alone_and_reserve_no_blob_scratch():
    rng = np.random.default_rng(3)
    h, w = 130, 260
    lab, _ = size_filter_map(rng, h, w)
    ds, _ = dataset_of(lab)
    assert ds.scratch_bytes() == 0
    info = ds.prepare(0, (), INF, INF, INF, 35)
    np.testing.assert_array_equal(ds.labels(0, lab.shape), lab)
    assert info["ignored_by_size"] == 0 and info["ignored_by_class"] == 0
    check_info(info, lab)
    blocks = -(-h * w // 1024)
    index_scratch = ds.scratch_bytes()
    assert 64 * blocks * 4 <= index_scratch <= 64 * blocks * 4 + 1024        # 0.25 bytes per pixel and the call's counters: no blob scratch
    ds.prepare(0, (), BY_AREA, INF, INF, RF)                                   # a finite limit: parents and blob map (8 bytes per pixel), sums, table
    assert ds.scratch_bytes() >= index_scratch + 8 * h * w


def test_class_ignoring():
    rng = np.random.default_rng(8)
    lab = block_map(rng, 61, 83, 5)
    assert (lab == 3).any() and not (lab == 9).any()
    want, changed = ref.relabel(lab, [3, 9])       # 9 is absent from the image
    ds, _ = dataset_of(lab)
    info = ds.prepare(0, (3, 9))
    assert info["ignored_by_class"] == changed == int((lab == 3).sum()) and info["ignored_by_size"] == 0
    np.testing.assert_array_equal(ds.labels(0, lab.shape), want)
    assert 3 not in info["classes"]
    check_info(info, want)
    # both filters: the class goes first, so its pixels are "ignored by class" however large its blobs are
    ds2, _ = dataset_of(lab)
    info2 = ds2.prepare(0, (3, 9), BY_AREA, BY_WIDTH, BY_HEIGHT, RF)
    want2, by_size = aa.ignore_large_nonzero_regions(want, RF, BY_AREA, BY_WIDTH, BY_HEIGHT)
    assert info2["ignored_by_class"] == changed and info2["ignored_by_size"] == by_size
    np.testing.assert_array_equal(ds2.labels(0, lab.shape), want2)
    check_info(info2, want2)


def rect_side(dim, factor):
    """round(dim * further_downscaling_factor) as std::round does it: halves away from zero (35 * 1.5 -> 53)"""
    return int(np.floor(dim * factor + 0.5))


def picks_for(ds, lab, wanted, dim=35, factor=1.0, rect_draws=None):
    """wanted: [(slot, k)] -> the device's picks"""
    specs = [(0, 0, 0, 0, 0, 1.0, factor, 0, 0, (0, 0, 0))] * len(wanted)
    draws = [(slot, k) + (rect_draws[i] if rect_draws else (0, 0)) for i, (slot, k) in enumerate(wanted)]
    return ds.pick(specs, draws, dim)


def test_index_picks_every_labelled_pixel():
    rng = np.random.default_rng(21)
    lab = block_map(rng, 37, 53, 6)                                  # the width is no multiple of 64; two blocks of 1024 pixels
    ds, _ = dataset_of(lab)
    info = ds.prepare(0)
    check_info(info, lab)
    wanted = [(slot, k) for slot, n in enumerate(info["counts"]) for k in range(n)]
    assert len(wanted) == int((lab != IGNORE).sum()) > 1800
    got = picks_for(ds, lab, wanted)
    flat = lab.ravel()
    positions = {c: np.flatnonzero(flat == c) for c in info["classes"]}
    for (slot, k), (label, x, y, _, _) in zip(wanted, got):
        c = info["classes"][slot]
        p = int(positions[c][k])
        assert (label, x, y) == (c, p % 53, p // 53), (slot, k)


def test_index_over_more_than_1024_blocks():
    rng = np.random.default_rng(22)
    h, w = 1100, 1000                                                # 1075 blocks: the scan of a class takes two strides
    lab = block_map(rng, h, w, 4)
    lab[500, 100:130] = 40                                          # a class confined to one block
    lab[h - 1, w - 1] = 41                                           # a class whose only pixel is the last pixel of the image
    ds, _ = dataset_of(lab)
    info = ds.prepare(0)
    check_info(info, lab)
    assert info["classes"][-2:] == [40, 41] and info["counts"][-2:] == [30, 1]
    wanted = []
    for slot, n in enumerate(info["counts"]):
        wanted += [(slot, 0), (slot, n - 1)] + [(slot, int(k)) for k in rng.integers(0, n, 200)]
    got = picks_for(ds, lab, wanted)
    flat = lab.ravel()
    positions = {c: np.flatnonzero(flat == c) for c in info["classes"]}
    for (slot, k), (label, x, y, _, _) in zip(wanted, got):
        c = info["classes"][slot]
        p = int(positions[c][k])
        assert (label, x, y) == (c, p % w, p // w), (slot, k)
    assert got[wanted.index((len(info["classes"]) - 1, 0))][1:3] == (w - 1, h - 1)
    # draws beyond the counts wrap as anh_resolve_pick says
    label, k = aa.resolve_pick(info["info"], 2 ** 32 - 1, 2 ** 64 - 1)
    (got_label, x, y, _, _), = ds.pick([(0, 0, 0, 0, 0, 1.0)], [(2 ** 32 - 1, 2 ** 64 - 1, 0, 0)], 35)
    assert (got_label, (x, y)) == (label, ref.kth_pixel(lab, label, k))


def test_a_label_of_64_is_invalid_and_the_dataset_still_works():
    rng = np.random.default_rng(23)
    lab = block_map(rng, 40, 50, 3)
    bad = lab.copy()
    bad[17, 23] = 64
    ds = aa.Dataset(3)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    assert ds.add(img, bad) == 0 and ds.add(img, lab) == 1
    with pytest.raises(aa.AnnonetHipError) as e:
        ds.prepare(0)
    assert e.value.code == 1
    with pytest.raises(aa.AnnonetHipError):                          # the image stays unprepared
        ds.pick([(0, 0, 0, 0, 0, 1.0)], [(0, 0, 0, 0)], 35)
    info = ds.prepare(1)
    check_info(info, lab)
    (label, x, y, _, _), = ds.pick([(1, 0, 0, 0, 0, 1.0)], [(1, 5, 0, 0)], 35)
    assert (x, y) == ref.kth_pixel(lab, info["classes"][1], 5)
    got_img, _, _ = ds.crop_batch([(1, 3, 2, 0, 0, 1.0)], 16, 3)
    np.testing.assert_array_equal(got_img[0], img[2:18, 3:19])


@pytest.mark.parametrize("dim", [35, 48])
@pytest.mark.parametrize("factor", [1.0, 1.5, 2.37])
def test_rectangles_match_random_rect_containing_point(dim, factor):
    rng = np.random.default_rng(dim * 10 + int(factor * 100))
    lab = block_map(rng, 90, 70, 3)
    ds, _ = dataset_of(lab)
    info = ds.prepare(0)
    side = rect_side(dim, factor)
    wanted = [(int(rng.integers(0, len(info["classes"]))), int(rng.integers(0, 2 ** 62))) for _ in range(60)]
    rect_draws = [(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))) for _ in wanted]
    rect_draws[:4] = [(0, 0), (2 ** 32 - 1, 2 ** 32 - 1), (side - 1, side), (side, side - 1)]
    got = picks_for(ds, lab, wanted, dim, factor, rect_draws)
    for (slot, point_draw), (dx, dy), (label, x, y, left, top) in zip(wanted, rect_draws, got):
        want_label, k = ref.resolve(info["classes"], info["counts"], slot, point_draw)
        assert (label, (x, y)) == (want_label, ref.kth_pixel(lab, want_label, k))
        r = aa.random_rect_containing_point(dx, dy, x, y, side, side)
        assert (left, top) == (r[0], r[1]) == ref.rect_corner(dx, dy, x, y, side)
        assert left <= x < left + side and top <= y < top + side


def reference_rectangles(full, infos, specs, draws, dim):
    """the specs with the rectangle the reference arithmetic gives for each draw"""
    out = []
    for s, (class_draw, point_draw, dx, dy) in zip(specs, draws):
        lab, info = full[s[0]], infos[s[0]]
        label, k = ref.resolve(info["classes"], info["counts"], class_draw, point_draw)
        x, y = ref.kth_pixel(lab, label, k)
        side = rect_side(dim, s[6] if len(s) > 6 and s[6] else 1.0)
        r = aa.random_rect_containing_point(dx, dy, x, y, side, side)
        out.append((s[0], r[0], r[1]) + tuple(s[3:]))
    return out


def random_draws(rng, n):
    return [(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)))
            for _ in range(n)]


def prepared_dataset(rng, channels, sizes, classes, **prepare):
    ds = aa.Dataset(channels)
    full, infos, images = [], [], []
    for i, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w) if channels == 1 else (h, w, channels), dtype=np.uint8)
        lab = block_map(rng, h, w, classes)
        assert ds.add(img, lab) == i
        infos.append(ds.prepare(i, **prepare))
        full.append(ds.labels(i, lab.shape))
        images.append(img)
    return ds, full, infos, images


@pytest.mark.parametrize("channels,classes,dim", [(3, 3, 35), (1, 5, 48)])
def test_crop_batch_picked_equals_crop_batch_on_the_reference_rectangles(channels, classes, dim):
    """the flips, brightness, further downscaling, noise and colour-offset cases of test_gpu_crops.py, with the rectangle picked on the device"""
    rng = np.random.default_rng(300 + channels)
    ds, full, infos, _ = prepared_dataset(rng, channels, [(60, 83), (130, 171), (20, 150)], classes, classes_to_ignore=(classes - 1,), by_area=40.0, receptive_field_side=RF)
    assert all(classes - 1 not in i["classes"] for i in infos)
    specs = []
    for k in range(30):
        gain = 1.0 if rng.random() < 0.4 else float(np.exp(rng.normal() * 0.2))
        f = [1.0, 1.5, 2.0, 2.37][k % 4]
        level = [0, 3, 40, 255][(k // 2) % 4]
        off = (0, 0, 0) if channels == 1 or k % 3 == 0 else tuple(int(v) for v in rng.integers(-40, 41, 3))
        specs.append((int(rng.integers(0, 3)), 10 ** 6, -10 ** 6, int(rng.random() < 0.5), int(rng.random() < 0.5), gain, f, level, int(rng.integers(0, 2 ** 62)), off))
    specs += [(0, 0, 0, 1, 1, 0.0), (2, 0, 0, 0, 1, 300.0)]            # short specs; zero / saturating gains
    draws = random_draws(rng, len(specs))
    img, lab, wgt, picks = ds.crop_batch_picked(specs, draws, dim, classes, 0.5, 0.5)    # the specs' own left / top (far outside) are ignored
    want_specs = reference_rectangles(full, infos, specs, draws, dim)
    wi, wl, ww = ds.crop_batch(want_specs, dim, classes, 0.5, 0.5)
    np.testing.assert_array_equal(img, wi)
    np.testing.assert_array_equal(lab, wl)
    np.testing.assert_array_equal(wgt, ww)
    assert [(p[3], p[4]) for p in picks] == [(s[1], s[2]) for s in want_specs]
    assert (lab != IGNORE).any() and len({p[0] for p in picks}) > 1
    img2, lab2, wgt2, _ = ds.crop_batch_picked(specs[:5], draws[:5], dim, classes, 0.3, 0.9)
    w2 = ds.crop_batch(want_specs[:5], dim, classes, 0.3, 0.9)
    np.testing.assert_array_equal(img2, w2[0])
    np.testing.assert_array_equal(wgt2, w2[2])


def test_training_on_picked_crops_equals_training_on_crops_with_those_rectangles():
    rng = np.random.default_rng(9)
    d = aa.RuntimeNet.GetRecommendedInputDimension(1, 40)
    ds, full, infos, _ = prepared_dataset(rng, 3, [(90, 120), (75, 64)], 3)

    def trainer():
        t = aa.TrainingNet(1, 3, aa.ANH_BF16, seed=3)
        t.SetNetWidth(0.5, 4); t.SetClassCount(3); t.Initialize(); t.SetLearningRate(0.05)
        return t

    a, b = trainer(), trainer()
    for step in range(3):
        specs = [(int(rng.integers(0, 2)), 0, 0, int(rng.random() < 0.5), int(rng.random() < 0.5), 1.0 if rng.random() < 0.4 else float(np.exp(rng.normal() * 0.2)))
                 for _ in range(6)]
        draws = random_draws(rng, 6)
        a.StartTrainingOnPickedCrops(ds, specs, draws, d)
        b.StartTrainingOnCrops(ds, reference_rectangles(full, infos, specs, draws, d), d)
        a.synchronize(); b.synchronize()
        assert a.get_last_loss() == b.get_last_loss()
    pa, ra = a.get_params()
    pb, rb = b.get_params()
    np.testing.assert_array_equal(pa, pb)
    np.testing.assert_array_equal(ra, rb)


def test_errors_and_bookkeeping():
    rng = np.random.default_rng(4)
    ds = aa.Dataset(3)
    imgs = [rng.integers(0, 256, (40 + 10 * i, 50, 3), dtype=np.uint8) for i in range(3)]
    labs = [block_map(rng, im.shape[0], 50, 3) for im in imgs]
    labs[2][:] = IGNORE                                               # nothing to draw from
    for i, (im, lb) in enumerate(zip(imgs, labs)):
        assert ds.add(im, lb) == i
    plain = sum(im.shape[0] * 50 * 5 for im in imgs)
    assert ds.resident_bytes() == plain
    spec, draw = [(0, 0, 0, 0, 0, 1.0)], [(1, 2, 3, 4)]
    t = aa.TrainingNet(1, 3, aa.ANH_BF16, seed=3)
    t.SetNetWidth(0.5, 4); t.SetClassCount(3); t.Initialize()
    d = aa.RuntimeNet.GetRecommendedInputDimension(1, 40)
    for call in (lambda: ds.pick(spec, draw, 35), lambda: ds.crop_batch_picked(spec, draw, 35, 3), lambda: t.StartTrainingOnPickedCrops(ds, spec, draw, d)):
        with pytest.raises(aa.AnnonetHipError, match="not been prepared") as e:      # an unprepared image
            call()
        assert e.value.code == 1
    info = ds.prepare(0)
    blocks = -(-40 * 50 // 1024)
    index_bytes = 4 * len(info["classes"]) * blocks                   # the documented size: 4 bytes per present class and 1024 pixels
    assert len(info["classes"]) == 3 and ds.resident_bytes() == plain + index_bytes
    ds.prepare(0)                                                     # again: the index is replaced, not added twice
    assert ds.resident_bytes() == plain + index_bytes
    empty = ds.prepare(2)
    assert empty["classes"] == [] and empty["counts"] == [] and ds.resident_bytes() == plain + index_bytes
    with pytest.raises(aa.AnnonetHipError) as e:                      # present == 0
        ds.pick([(2, 0, 0, 0, 0, 1.0)], draw, 35)
    assert e.value.code == 1
    with pytest.raises(aa.AnnonetHipError):
        ds.prepare(5)
    with pytest.raises(aa.AnnonetHipError):
        ds.prepare(0, by_area=-1.0)
    with pytest.raises(aa.AnnonetHipError):
        ds.prepare(0, classes_to_ignore=list(range(65)))
    assert len(ds.pick(spec, draw, 35)) == 1                          # the dataset still works
    ds.remove(0)
    assert ds.resident_bytes() == plain - 40 * 50 * 5
    assert ds.add(imgs[1], labs[1]) == 0                              # the slot is reused ...
    with pytest.raises(aa.AnnonetHipError, match="not been prepared"):  # ... without the index of the image that lay there
        ds.pick(spec, draw, 35)
    info = ds.prepare(0)
    check_info(info, labs[1])
    (label, x, y, _, _), = ds.pick(spec, [(1, 7, 0, 0)], 35)
    assert (x, y) == ref.kth_pixel(labs[1], info["classes"][1], 7)
