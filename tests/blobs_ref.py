"""Reference for the device's connected-blob labelling and region table (anh_label_blobs_device, anh_regions_device).

A blob = an 8-connected set of pixels of EQUAL non-zero value; blobs are numbered 1, 2, ... in raster order of their first pixel and the
count is "labels including the background one", as annonet_amd/host/annonet_host.h: label_connected_blobs returns it.  blobs_ref labels
with scipy.ndimage.label per distinct value (3 x 3 structure, as png_util.blobs_8) and renumbers; flood_fill is a literal transcription
of label_connected_blobs for small maps; region_table is the numpy computation of the table's fields."""
import numpy as np
from scipy import ndimage

REGION_FIELDS = ("blob", "label", "detected", "left", "top", "right", "bottom", "first_row", "first_col", "area", "seeds", "peak")


def blobs_ref(label_map):
    """(u32 blob map, count): numbering by each blob's first pixel in raster order"""
    img = np.asarray(label_map)
    ids = np.zeros(img.shape, np.int64)
    nxt = 1
    for v in np.unique(img):
        if v == 0:
            continue
        lab, n = ndimage.label(img == v, structure=np.ones((3, 3)))
        ids[lab > 0] = lab[lab > 0] + nxt - 1
        nxt += n
    flat = ids.reshape(-1)
    first = np.full(nxt, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")          # distinct first pixels: the order is total
    number = np.zeros(nxt, np.int64)
    number[1 + order] = np.arange(1, nxt)
    return number[ids].astype(np.uint32), nxt


def flood_fill(label_map):
    """label_connected_blobs (annonet_host.h) transcribed line by line; for small maps"""
    img = np.asarray(label_map)
    nr, nc = img.shape
    blobs = np.zeros((nr, nc), np.uint32)
    nxt = 1
    for r in range(nr):
        for c in range(nc):
            if img[r, c] == 0 or blobs[r, c] != 0:
                continue
            v = img[r, c]
            blobs[r, c] = nxt
            stack = [(r, c)]
            while stack:
                y, x = stack.pop()
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if yy < 0 or yy >= nr or xx < 0 or xx >= nc or blobs[yy, xx] != 0 or img[yy, xx] != v:
                            continue
                        blobs[yy, xx] = nxt
                        stack.append((yy, xx))
            nxt += 1
    return blobs, nxt


def seed_flags(label_map, planes, levels, reference_order=False):
    """det_seed_kernel: pixel p is a seed where float32(planes[label] - planes[0]) > levels[label] - levels[0] (compared in float64);
    labels 0, 65535 and >= K never seed.  reference_order: the flag lands on the transposed pixel (dropped outside the map)."""
    lab = np.asarray(label_map)
    K = planes.shape[0]
    H, W = lab.shape
    levels = np.zeros(K) if levels is None else np.asarray(levels, np.float64)
    ok = (lab != 0) & (lab != 65535) & (lab < K)
    idx = np.where(ok, lab, 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        margin = (np.take_along_axis(planes, idx[None], 0)[0] - planes[0]).astype(np.float32)
        f = ok & (margin.astype(np.float64) > levels[idx] - levels[0])
    if not reference_order:
        return f
    out = np.zeros_like(f)
    r, c = np.nonzero(f)
    keep = (c < H) & (r < W)
    out[c[keep], r[keep]] = True
    return out


def region_table(label_map, planes, levels=None, reference_order=False):
    """(table as a dict of arrays by field name, blob map, count) from blobs_ref and the planes.  peak = the largest non-NaN
    float32(planes[label] - planes[0]) over the blob, -inf where there is none or the label is >= K."""
    lab = np.asarray(label_map)
    K = planes.shape[0]
    H, W = lab.shape
    blobs, count = blobs_ref(lab)
    n = count - 1
    flat = blobs.reshape(-1).astype(np.int64)
    fg = flat > 0
    rows, cols = np.divmod(np.arange(flat.size), W)
    positive = levels is not None and (np.asarray(levels) > 0).any()
    t = {"blob": np.arange(1, n + 1, dtype=np.uint32)}
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    first = first[1:]
    t["first_row"], t["first_col"] = (first // W).astype(np.int32), (first % W).astype(np.int32)
    t["label"] = lab.reshape(-1)[first].astype(np.uint16)
    t["area"] = np.bincount(flat, minlength=n + 1)[1:].astype(np.int64)
    for name, src, fn, init in (("left", cols, np.minimum, W), ("right", cols, np.maximum, -1), ("top", rows, np.minimum, H), ("bottom", rows, np.maximum, -1)):
        acc = np.full(n + 1, init, np.int64)
        fn.at(acc, flat[fg], src[fg])
        t[name] = acc[1:].astype(np.int32)
    flags = seed_flags(lab, planes, levels if positive else None, reference_order).reshape(-1)
    t["seeds"] = np.bincount(flat[flags & fg], minlength=n + 1)[1:].astype(np.int64)
    t["detected"] = ((t["seeds"] > 0) if positive else np.ones(n, bool)).astype(np.uint16)
    ok = fg & (lab.reshape(-1) < K)
    idx = np.where(ok, lab.reshape(-1), 0).astype(np.int64)
    pl = planes.reshape(K, -1)
    with np.errstate(invalid="ignore"):
        margin = (pl[idx, np.arange(flat.size)] - pl[0]).astype(np.float32)
    ok &= ~np.isnan(margin)
    peak = np.full(n + 1, -np.inf, np.float32)
    np.maximum.at(peak, flat[ok], margin[ok])
    t["peak"] = peak[1:]
    return t, blobs, count


def filtered(label_map, blobs, table):
    """the label map with every blob without a seed relabelled 0 (annonet_infer.cpp:229-238)"""
    keep = np.concatenate([[True], table["seeds"] > 0])
    out = np.asarray(label_map).copy()
    out[~keep[blobs.astype(np.int64)]] = 0
    return out


def assert_table_equal(got, want):
    """every field of every row; the margins were subtracted in float32 on both sides and are compared in float64"""
    assert len(got) == len(want["blob"]), (len(got), len(want["blob"]))
    for name in REGION_FIELDS:
        g, w = np.asarray(got[name]), want[name]
        if name == "peak":
            g, w = g.astype(np.float64), w.astype(np.float64)
        np.testing.assert_array_equal(g, w, err_msg=name)


# ---- the maps of the device tests (test_gpu_blobs.py, test_gpu_detection_filter.py), chosen around the kernels' 32-pixel tiles ----
T = 32          # kBlobTile (annonet_amd/csrc/kernels.h); det_flood_kernel tiles by 32 as well
SIZES = [(1, 1), (1, 2 * T + 6), (2 * T + 6, 1), (T - 1, T + 1), (T + 1, T - 1), (2 * T, 2 * T), (3 * T + 1, 4 * T + 2)]


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


def pattern(name, shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    if name == "random":
        return rng.integers(0, 3, shape).astype(np.uint16)
    if name == "random_wide_values":
        return rng.choice(np.array([0, 1, 2, 7, 65535], np.uint16), size=shape, p=[0.3, 0.25, 0.25, 0.1, 0.1])
    if name == "checkerboard":          # every colour is ONE blob through its diagonals
        yy, xx = np.mgrid[0:h, 0:w]
        return (1 + (yy + xx) % 2).astype(np.uint16)
    if name == "corner_diagonals":      # (T-1,T-1)->(T,T) and (T-1,T)->(T,T-1): pairs that touch only across the corner where four tiles meet
        a = np.zeros(shape, np.uint16)
        for (y, x, v) in ((T - 1, T - 1, 1), (T, T, 1), (T - 1, T, 2), (T, T - 1, 2)):
            if y < h and x < w:
                a[y, x] = v
        for i in range(min(h, w)):       # and a long diagonal of a third label through every tile corner on its way
            if a[i, i] == 0 and i not in (T - 1, T):
                a[i, i] = 3
        return a
    if name == "spiral":
        return spiral(h, w)
    if name == "full":
        return np.full(shape, 2, np.uint16)
    if name == "u_shape":               # arms in different tile columns that meet only in the last row: the root moves to the earlier arm's first pixel
        a = np.zeros(shape, np.uint16)
        left, right = min(3, w - 1), max(w - 3, 0)
        a[min(5, h - 1):, right] = 1     # the right arm starts higher up ...
        a[min(9, h - 1):, left] = 1      # ... than the left one
        a[h - 1, left:right + 1] = 1
        return a
    if name == "zeros":
        return np.zeros(shape, np.uint16)
    raise KeyError(name)


PATTERNS = ["random", "random_wide_values", "checkerboard", "corner_diagonals", "spiral", "full", "u_shape", "zeros"]


def smooth_map(shape, seed):
    rng = np.random.default_rng(seed)
    field = ndimage.gaussian_filter(rng.normal(size=shape), 6.0)
    other = ndimage.gaussian_filter(rng.normal(size=shape), 9.0)
    lab = np.zeros(shape, np.uint16)
    s = field.std()
    lab[field > 0.4 * s] = 1
    lab[field < -0.5 * s] = 2
    lab[(other > 1.2 * other.std()) & (lab == 0)] = 65535
    return lab
