"""numpy restatements of the two resizes of downscaled inference, as annonet_amd/host/annonet_host.h states them
(dlib::resize_image's corner-aligned grid [UPSTREAM-UNVERIFIED]): resize_image_bilinear (read_sample, annonet.cpp:153) here,
resize_label_image (annonet.cpp:132-141) in png_util.resize_nearest.  The array form follows oracle/oracle.py's crop restatement.
Test infrastructure."""
import numpy as np

from png_util import resize_nearest  # noqa: F401  (the nearest-neighbour half)


def round_half_away(v):
    """std::round on a non-negative double"""
    return int(np.floor(v + 0.5))


def scaled_size(n, scale):
    """the side resize_image_bilinear gives: std::round(size_scale * n)"""
    return round_half_away(np.float64(scale) * np.float64(n))


def bilinear_to(img, out_h, out_w):
    """the sampling of resize_image_bilinear onto an out_h x out_w grid: coordinates in double, fractions and interpolation in float,
    (1-fy)*((1-fx)*tl + fx*tr) + fy*((1-fx)*bl + fx*br) in that order, rounded half up"""
    a = np.asarray(img, dtype=np.uint8)
    in_h, in_w = a.shape[:2]
    c = a.astype(np.float32).reshape(in_h, in_w, -1)
    ys = np.arange(out_h) * ((in_h - 1) / float(max(out_h - 1, 1)))
    xs = np.arange(out_w) * ((in_w - 1) / float(max(out_w - 1, 1)))
    t = np.floor(ys).astype(np.int64)
    b = np.minimum(t + 1, in_h - 1)
    le = np.floor(xs).astype(np.int64)
    ri = np.minimum(le + 1, in_w - 1)
    fy = (ys - t).astype(np.float32)[:, None, None]
    fx = (xs - le).astype(np.float32)[None, :, None]
    one = np.float32(1.0)
    top = (one - fx) * c[np.ix_(t, le)] + fx * c[np.ix_(t, ri)]
    bot = (one - fx) * c[np.ix_(b, le)] + fx * c[np.ix_(b, ri)]
    val = (one - fy) * top + fy * bot + np.float32(0.5)
    assert val.dtype == np.float32
    return val.astype(np.int32).astype(np.uint8).reshape((out_h, out_w) + a.shape[2:])


def bilinear(img, scale):
    """resize_image_bilinear(scale, img); scale 1 returns the image itself"""
    a = np.asarray(img, dtype=np.uint8)
    if scale == 1.0:
        return a
    return bilinear_to(a, scaled_size(a.shape[0], scale), scaled_size(a.shape[1], scale))


def shrink(img, factor):
    """read_sample's resize: dlib::resize_image(1.0 / factor, image)"""
    return bilinear(img, 1.0 / factor)


# (source height, source width), scale — the cases the host restatement and the device kernels are both checked on
CASES = [((97, 131), 1 / 2), ((150, 170), 1 / 1.5), ((260, 190), 1 / 3.7), ((64, 64), 1.0), ((40, 30), 2.0),
         ((1, 57), 1 / 2), ((61, 1), 1 / 2), ((3, 90), 1 / 2.9)]   # 1 row; 1 column; 3 rows -> a single output row (max(out - 1, 1))
