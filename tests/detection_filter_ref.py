"""Reference for the detection-level filter's flood path (anh_detection_filter_device: det_seed_kernel, det_flood_kernel and its host
loop, det_apply_kernel), the maps and seed plans its tests run on, and the hand-made cases.

expected() is the answer by labelling: blobs_ref.region_table counts each blob's seeds, blobs_ref.filtered removes the blobs without one.
flood() is a literal numpy restatement of what the device does instead — seed flags spread to 8-neighbours of equal non-zero label
until nothing changes — and shares no code with the scipy labelling; tests/test_detection_filter_ref.py holds the two to each other."""
import functools

import numpy as np
from scipy import ndimage

import blobs_ref as br
from blobs_ref import PATTERNS, SIZES, T, pattern, smooth_map  # noqa: F401  (the GPU test takes them from here)

FRAME = (T + 1, 2 * T + 1)      # 33 x 65: the hand-made cases sit across the seams of its 2 x 3 flood tiles
PLANS = ["random", "last_pixel", "first_pixel", "none", "negative_threshold"]
# non-square: a transposed seed position can fall outside the map
REFERENCE_ORDER_MAPS = [(name, shape) for name in ("random", "corner_diagonals") for shape in (FRAME, FRAME[::-1])]


def expected(lab, planes, levels, reference_order=False):
    """the map the filter leaves: every blob without a seed becomes 0; unchanged when no level is positive"""
    lab = np.asarray(lab)
    if levels is None or not (np.asarray(levels, np.float64) > 0).any():
        return lab.copy()
    table, blobs, _ = br.region_table(lab, planes, levels, reference_order)
    return br.filtered(lab, blobs, table)


def flood(lab, seeds):
    """(filtered map, sweeps): flags |= any 8-neighbour of equal non-zero label that is flagged, until a sweep changes nothing; then
    labels[(labels != 0) & ~flags] = 0.  Outside the map the label is 0 and the flag is 0, as in the kernel's halo."""
    lab = np.asarray(lab)
    h, w = lab.shape
    padded = np.zeros((h + 2, w + 2), lab.dtype)
    padded[1:-1, 1:-1] = lab
    flags = np.zeros((h + 2, w + 2), bool)
    flags[1:-1, 1:-1] = seeds
    shifts = [(dy, dx) for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)]
    same = [(padded[dy:dy + h, dx:dx + w] == lab) & (lab != 0) for dy, dx in shifts]
    sweeps = 0
    while True:
        sweeps += 1
        reach = np.zeros((h, w), bool)
        for (dy, dx), eq in zip(shifts, same):
            reach |= eq & flags[dy:dy + h, dx:dx + w]
        reach &= ~flags[1:-1, 1:-1]
        if not reach.any():
            break
        flags[1:-1, 1:-1] |= reach
    out = lab.copy()
    out[(lab != 0) & ~flags[1:-1, 1:-1]] = 0
    return out, sweeps


def tile_segments(lab, ty=0, tx=0):
    """the number of 8-connected pieces of equal non-zero label inside flood tile (ty, tx), the tile taken alone"""
    window = np.asarray(lab)[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
    return sum(ndimage.label(window == v, structure=np.ones((3, 3)))[1] for v in np.unique(window) if v != 0)


def spiral_ends(lab):
    """(outer end, inner end) of blobs_ref.spiral's path: the two pixels with a single 8-neighbour on the path"""
    on = np.pad(np.asarray(lab) != 0, 1)
    h, w = lab.shape
    neighbours = sum(on[dy:dy + h, dx:dx + w].astype(int) for dy in range(3) for dx in range(3)) - 1
    ends = [tuple(int(v) for v in p) for p in np.argwhere((lab != 0) & (neighbours == 1))]
    assert len(ends) == 2 and ends[0] == (0, 0), ends
    return ends[0], ends[1]


# ---- seed plans: (planes float32 [K,H,W], levels) for a map -------------------------------------------------------------------------
def _blob_pixel_plan(lab, K, parity, last):
    blobs, count = br.blobs_ref(lab)
    planes = np.zeros((K,) + lab.shape, np.float32)
    flat = blobs.reshape(-1).astype(np.int64)
    where = np.full(count, -1 if last else flat.size, np.int64)
    (np.maximum if last else np.minimum).at(where, flat, np.arange(flat.size))
    for b in range(1, count):
        label = int(lab.reshape(-1)[where[b]])
        if b % 2 == parity and label < K:
            planes[label].reshape(-1)[where[b]] = 1.0
    return planes, [0.0] + [0.5] * (K - 1)


def plan(name, lab, pattern_name="", K=3):
    lab = np.asarray(lab)
    if name == "random":            # the planes and levels of test_gpu_blobs.py's cases
        rng = np.random.default_rng(len(pattern_name) + lab.shape[0] * 7 + lab.shape[1])
        planes = rng.normal(0, 2, (K,) + lab.shape).astype(np.float32)
        planes[rng.random((K,) + lab.shape) < 0.05] = np.nan
        return planes, [0.0, 3.0, 4.5]
    if name == "last_pixel":        # one seed on the LAST pixel of every even-numbered blob of label < K: the odd ones go
        return _blob_pixel_plan(lab, K, 0, True)
    if name == "first_pixel":       # one seed on the FIRST pixel of every odd-numbered blob of label < K: the even ones go
        return _blob_pixel_plan(lab, K, 1, False)
    if name == "wide":              # last_pixel with 8 classes: label 7 seeds, 65535 never does
        return _blob_pixel_plan(lab, 8, 0, True)
    if name == "none":              # no seed anywhere: every non-zero pixel becomes 0
        return np.zeros((K,) + lab.shape, np.float32), [0.0, 0.5, 0.5]
    if name == "negative_threshold":    # levels[label] - levels[0] < 0 = every margin: every pixel of label 1 or 2 seeds; 7 and 65535 go
        return np.zeros((K,) + lab.shape, np.float32), [2.0, 0.5, 0.0]
    raise KeyError(name)


def plans_of(pattern_name):
    return PLANS + (["wide"] if pattern_name == "random_wide_values" else [])


CASES = [(p, s, q) for p in PATTERNS for s in SIZES for q in plans_of(p)]


def case_id(c):
    return "%s-%dx%d-%s" % (c[0], c[1][0], c[1][1], c[2])


@functools.lru_cache(maxsize=None)
def case(pattern_name, shape, plan_name):
    """(label map, planes, levels, expected map), computed once and read-only"""
    lab = pattern(pattern_name, shape)
    planes, levels = plan(plan_name, lab, pattern_name)
    want = expected(lab, planes, levels)
    for a in (lab, planes, want):
        a.setflags(write=False)
    return lab, planes, tuple(levels), want


# ---- hand-made cases: tiny maps padded into the 33 x 65 frame so that they straddle tiles --------------------------------------------
def _frame(K=3):
    return np.zeros(FRAME, np.uint16), np.zeros((K,) + FRAME, np.float32)


def _equality():
    """a margin exactly equal to levels[label] - levels[0] is not a seed; the next float32 above is.  Blob A (label 1, row 31) holds the
    equal margin, blob B (label 2, row 32, touching A) the next one: A goes, B stays."""
    lab, planes = _frame()
    lab[31, 30:34], lab[32, 30:34] = 1, 2
    planes[0] = -0.25
    planes[1, 31, 33] = 0.5                                             # 0.5 + 0.25 = 0.75 = 1.25 - 0.5 exactly
    planes[2, 32, 30] = np.nextafter(np.float32(0.5), np.float32(1))    # (0.5 + 2^-24) + 0.25 is a float32: the next one above 0.75
    assert planes[2, 32, 30] - planes[0, 32, 30] == np.nextafter(np.float32(0.75), np.float32(1))
    want = lab.copy()
    want[31] = 0
    seeds = np.zeros(FRAME, bool)
    seeds[32, 30] = True
    return lab, planes, [0.5, 1.25, 1.25], want, seeds


def _float_subtraction():
    """planes[1] = 2^24, planes[0] = -1, level 16777216.5: the float32 difference is 16777216 (no seed), the double one 16777217 (a
    seed).  The label-1 blob goes; a label-2 blob with margin 1 > 0.5 beside it stays."""
    lab, planes = _frame()
    lab[30:33, 31:33] = 1
    lab[30:33, 34] = 2
    planes[0], planes[1] = -1.0, 2.0 ** 24
    want = lab.copy()
    want[want == 1] = 0
    return lab, planes, [0.0, 16777216.5, 0.5], want, lab == 2


def _double_threshold():
    """levels [0.1, 0.3] give the threshold 0.3 - 0.1 = 0.19999999999999998 in double; a margin of float32(0.2) = 0.2000000029... is a
    seed (formed in float32 the threshold would be 0.20000002, above it).  A second blob with margin 0.19 goes."""
    lab, planes = _frame(2)
    lab[31:33, 31:33] = 1
    lab[31:33, 40:42] = 1
    planes[1, 32, 32] = np.float32(0.2)
    planes[1, 31, 40] = np.float32(0.19)
    want = lab.copy()
    want[:, 40:42] = 0
    seeds = np.zeros(FRAME, bool)
    seeds[32, 32] = True
    return lab, planes, [0.1, 0.3], want, seeds


def _corner_seed():
    """a seed on (31,31) whose blob continues only at (32,32), across the corner where four tiles meet; the mirror pair (31,32)/(32,31)
    of label 2 has no seed and goes"""
    lab, planes = _frame()
    lab[31, 31] = lab[32, 32] = 1
    lab[31, 32] = lab[32, 31] = 2
    planes[1, 31, 31] = 1.0
    want = lab.copy()
    want[want == 2] = 0
    seeds = np.zeros(FRAME, bool)
    seeds[31, 31] = True
    return lab, planes, [0.0, 0.5, 0.5], want, seeds


def _ragged_edge():
    """a seeded blob along the last row and up the last column of the 33 x 65 map — (32,64) is the only pixel of its tile — and an
    unseeded pixel next to it"""
    lab, planes = _frame()
    lab[32, 58:65] = 1
    lab[27:33, 64] = 1
    lab[30, 62] = 2
    planes[1, 32, 58] = 1.0
    want = lab.copy()
    want[30, 62] = 0
    seeds = np.zeros(FRAME, bool)
    seeds[32, 58] = True
    return lab, planes, [0.0, 0.5, 0.5], want, seeds


def _trapped_neighbour():
    """an unseeded blob of label 2 wholly enclosed by a seeded ring of label 1, over the four-tile corner: the ring stays, the inside goes"""
    lab, planes = _frame()
    lab[28:33, 30:35] = 1
    lab[29:32, 31:34] = 2
    planes[1, 28, 30] = 1.0
    want = lab.copy()
    want[want == 2] = 0
    seeds = np.zeros(FRAME, bool)
    seeds[28, 30] = True
    return lab, planes, [0.0, 0.5, 0.5], want, seeds


def _adjacent_ignore():
    """a seeded blob of label 1 next to pixels of label 65535 (whose planes would seed any class): they go"""
    lab, planes = _frame()
    lab[30:33, 29:33] = 1
    lab[30:33, 33:36] = 65535
    lab[29, 29:36] = 65535
    planes[1:] = 1.0
    want = lab.copy()
    want[want == 65535] = 0
    return lab, planes, [0.0, 0.5, 0.5], want, lab == 1


HAND_MADE = {"equality": _equality, "float_subtraction": _float_subtraction, "double_threshold": _double_threshold, "corner_seed": _corner_seed,
             "ragged_edge": _ragged_edge, "trapped_neighbour": _trapped_neighbour, "adjacent_ignore": _adjacent_ignore}


@functools.lru_cache(maxsize=None)
def hand_made(name):
    """(label map, planes, levels, the stated answer, the stated seed flags), read-only"""
    lab, planes, levels, want, seeds = HAND_MADE[name]()
    for a in (lab, planes, want, seeds):
        a.setflags(write=False)
    return lab, planes, tuple(levels), want, seeds
