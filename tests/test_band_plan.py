"""The launch shapes of GaussianBlur and RandomAdjustSharpness, pinned exactly
(no GPU): ffcv_gaussian_blur_strip_cols and ffcv_sharpness_strip_cols against
the table tests/golden/band_plan.npz (written by tests/golden/make_band_plan.py
from the library at the commit that added it), over a grid of shapes that
crosses every branch of the planner: the whole image, one strip per band, the
strip search from its first guess down, the last strip and band cut short, the
widest supported side, and the inputs it rejects."""
import os

import numpy as np

from tests.golden import make_band_plan as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'band_plan.npz')


def test_table_covers_the_grid():
    z = np.load(GOLDEN)
    assert [tuple(r) for r in z['blur'][:, :3]] == M.blur_grid()
    assert [tuple(r) for r in z['sharpness'][:, :2]] == M.sharp_grid()
    assert [tuple(r) for r in z['rejected'][:, :3]] == list(M.REJECTED)
    assert len(M.sharp_grid()) == 13 * 21 and len(M.blur_grid()) > 4 * 13 * 21
    # every regime is there: one workgroup, bands of one strip, and strips
    for name, col in (('blur', 3), ('sharpness', 2)):
        t = z[name]
        h, w, strip, wgs = t[:, 0], t[:, 1], t[:, col], t[:, col + 1]
        assert (wgs == 1).any() and ((strip == w) & (wgs > 1)).any() and ((strip < w) & (strip > 1)).any()
        assert ((strip >= 1) & (strip <= w)).all() and (wgs >= 1).all()


def test_strip_cols_match_the_table(hip_lib):
    from ffcv_amd import libffcv as L
    z = np.load(GOLDEN)
    lds, band = L.gaussian_blur_lds_bytes(), L.gaussian_blur_band_rows()
    for h, w, k, strip, wgs in z['blur'].tolist():
        assert L.gaussian_blur_strip_cols(h, w, k) == strip, (h, w, k)
        assert M.workgroups(h, w, 15, lds, band, strip) == wgs, (h, w, k)
    lds, band = L.sharpness_lds_bytes(), L.sharpness_band_rows()
    for h, w, strip, wgs in z['sharpness'].tolist():
        assert L.sharpness_strip_cols(h, w) == strip, (h, w)
        assert M.workgroups(h, w, 6, lds, band, strip) == wgs, (h, w)


def test_rejected_inputs_plan_nothing(hip_lib):
    from ffcv_amd import libffcv as L
    for h, w, k, blur, sharp in np.load(GOLDEN)['rejected'].tolist():
        assert blur == 0 and L.gaussian_blur_strip_cols(h, w, k) == 0, (h, w, k)
        assert L.sharpness_strip_cols(h, w) == sharp, (h, w)
        assert (sharp == 0) == (not (0 < h <= 65535 and 0 < w <= 65535)), (h, w)
