"""Writes tests/golden/band_plan.npz: the column-strip width that the built
library plans for GaussianBlur and RandomAdjustSharpness launches
(ffcv_gaussian_blur_strip_cols, ffcv_sharpness_strip_cols) over a grid that
crosses every branch of the strip search, and the workgroups per image that
follow from it.  Needs the built library; no GPU.

    python tests/golden/make_band_plan.py

The numbers are a record of the library at the commit that wrote them
(tests/test_band_plan.py holds later commits to them): run it again only when
the launch shapes are meant to change.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

HEIGHTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 46, 64, 65, 97)
WIDTHS = (1, 2, 3, 4, 5, 47, 48, 64, 65, 67, 70, 120, 125, 131, 224, 300, 412, 600, 1024, 4096, 65535)
KSIZES = (1, 3, 5, 9, 23, 31)
# (height, width, ksize): sides that are 0, negative or above 65535, an even or out-of-range ksize
REJECTED = ((0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, -3, 3), (65536, 5, 3), (5, 65536, 3), (0, 0, 1),
            (32, 32, 0), (32, 32, 2), (32, 32, 4), (32, 32, 30), (32, 32, 33), (32, 32, -1), (32, 32, -3))


def workgroups(h, w, px_bytes, lds_bytes, band_rows, strip_cols):
    """Workgroups per image: one while px_bytes * h * w fits lds_bytes, else
    ceil(w / strip_cols) strips of every band of band_rows rows."""
    rows = h if px_bytes * h * w <= lds_bytes else min(h, band_rows)
    return -(-h // rows) * -(-w // strip_cols)


def blur_grid():
    return [(h, w, k) for h in HEIGHTS for w in WIDTHS for k in KSIZES if (k - 1) // 2 < min(h, w)]


def sharp_grid():
    return [(h, w) for h in HEIGHTS for w in WIDTHS]


def main():
    from ffcv_amd import libffcv as L
    blur = [(h, w, k, L.gaussian_blur_strip_cols(h, w, k)) for h, w, k in blur_grid()]
    blur = [r + (workgroups(r[0], r[1], 15, L.gaussian_blur_lds_bytes(), L.gaussian_blur_band_rows(), r[3]),)
            for r in blur]
    sharp = [(h, w, L.sharpness_strip_cols(h, w)) for h, w in sharp_grid()]
    sharp = [r + (workgroups(r[0], r[1], 6, L.sharpness_lds_bytes(), L.sharpness_band_rows(), r[2]),) for r in sharp]
    rejected = [r + (L.gaussian_blur_strip_cols(*r), L.sharpness_strip_cols(r[0], r[1])) for r in REJECTED]
    np.savez_compressed(os.path.join(HERE, 'band_plan.npz'),
                        blur=np.array(blur, np.int32),          # height, width, ksize, strip_cols, workgroups
                        sharpness=np.array(sharp, np.int32),    # height, width, strip_cols, workgroups
                        rejected=np.array(rejected, np.int32))  # height, width, ksize, blur's and sharpness's answer
    print(len(blur), 'blur rows,', len(sharp), 'sharpness rows,', len(rejected), 'rejected')


if __name__ == '__main__':
    main()
