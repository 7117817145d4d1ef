"""tests/dataset_ref.py against hand-worked 4 x 5 cases."""
import numpy as np
import pytest

import dataset_ref as ref

I = ref.IGNORE
LAB = np.array([[0, 0, 1, 1, I],
                [2, 0, 1, I, I],
                [2, 2, 0, 3, 0],
                [I, 2, 0, 0, 1]], dtype=np.uint16)


def test_relabel_by_hand():
    got, changed = ref.relabel(LAB, [1, 7])          # 7 does not occur
    assert changed == 4
    want = LAB.copy()
    want[0, 2] = want[0, 3] = want[1, 2] = want[3, 4] = I
    np.testing.assert_array_equal(got, want)
    assert LAB[0, 2] == 1                             # the input is left alone
    got, changed = ref.relabel(LAB, [I])              # the ignore label itself: nothing changes
    assert changed == 0
    np.testing.assert_array_equal(got, LAB)


def test_present_classes_by_hand():
    assert ref.present_classes(LAB) == ([0, 1, 2, 3], [7, 4, 4, 1])
    assert ref.present_classes(np.full((2, 2), I, np.uint16)) == ([], [])


def test_kth_pixel_is_raster_order():
    assert [ref.kth_pixel(LAB, 1, k) for k in range(4)] == [(2, 0), (3, 0), (2, 1), (4, 3)]
    assert [ref.kth_pixel(LAB, 2, k) for k in range(4)] == [(0, 1), (0, 2), (1, 2), (1, 3)]
    assert ref.kth_pixel(LAB, 3, 0) == (3, 2)
    with pytest.raises(IndexError):
        ref.kth_pixel(LAB, 3, 1)


def test_resolve_by_hand():
    classes, counts = ref.present_classes(LAB)
    assert ref.resolve(classes, counts, 0, 0) == (0, 0)
    assert ref.resolve(classes, counts, 5, 9) == (1, 1)            # 5 % 4 = 1 -> class 1 with 4 pixels; 9 % 4 = 1
    assert ref.resolve(classes, counts, 2 ** 32 - 1, 2 ** 64 - 1) == (3, 0)
    assert ref.resolve(classes, counts, 6, 2 ** 64 - 1) == (2, (2 ** 64 - 1) % 4)
    with pytest.raises(ValueError):
        ref.resolve([], [], 1, 1)


def test_rect_corner_by_hand():
    # side 4 around x = 10: centres 9..12 (x - 1 .. x + 2), left = centre - 2
    assert [ref.rect_corner(d, 0, 10, 20, 4)[0] for d in range(5)] == [7, 8, 9, 10, 7]
    # side 5 around y = 20: centres 18..22, top = centre - 2
    assert [ref.rect_corner(0, d, 10, 20, 5)[1] for d in range(6)] == [16, 17, 18, 19, 20, 16]
    for side in (1, 4, 5):
        for d in range(side):
            left, top = ref.rect_corner(d, d, 3, 2, side)
            assert left <= 3 < left + side and top <= 2 < top + side   # the rectangle contains the point
