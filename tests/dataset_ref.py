"""numpy restatement of what anh_dataset_prepare / anh_dataset_pick compute (annonet_train_main.cpp:414-424 class ignoring, :121-131 the
choice of a crop's centre), written for clarity: the reference the device code is held to.  The size filter's reference is the
library's own host routine (aa.ignore_large_nonzero_regions)."""
import numpy as np

IGNORE = 65535


def relabel(labels, classes_to_ignore):
    """-> (label map with the given classes set to IGNORE, pixels changed)"""
    lab = np.array(labels, dtype=np.uint16)
    hit = np.isin(lab, [c for c in classes_to_ignore if c != IGNORE])
    lab[hit] = IGNORE
    return lab, int(hit.sum())


def present_classes(labels):
    """-> (class values present, ascending; their pixel counts), the ignore label left out"""
    values, counts = np.unique(np.asarray(labels)[np.asarray(labels) != IGNORE], return_counts=True)
    return [int(v) for v in values], [int(c) for c in counts]


def resolve(classes, counts, class_draw, point_draw):
    """the class is drawn uniformly over the present ones, taken in ascending value, then a point of it: -> (label, k)"""
    if not classes:
        raise ValueError("nothing to draw from")
    slot = class_draw % len(classes)
    return classes[slot], point_draw % counts[slot]


def kth_pixel(labels, label, k):
    """(x, y) of the k-th pixel of `label` in raster order"""
    lab = np.asarray(labels)
    p = int(np.flatnonzero(lab.ravel() == label)[k])
    return p % lab.shape[1], p // lab.shape[1]


def rect_corner(draw_x, draw_y, x, y, side):
    """(left, top) of random_rect_containing_point (annonet_train.h:85-105) for a square: the centre is drawn from `side` positions"""
    cx = x - (side - 1) // 2 + draw_x % side
    cy = y - (side - 1) // 2 + draw_y % side
    return cx - side // 2, cy - side // 2
