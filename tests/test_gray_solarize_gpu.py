"""RandomGrayscale / RandomSolarization on the MI355X: the two new steps of
ffcv_color_jitter_batch, bit for bit against numpy (tests/blur_ref.py), in
every program of one to three distinct steps that contains one, in both
regimes (whole image in LDS; tiles, two passes with contrast)."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from tests import blur_ref as R
from tests.color_jitter_ref import CONTRAST, SATURATION, near_integer_triples
from tests.test_color_jitter_gpu import _device_program, _shapes
from tests.test_gray_solarize import THRESHOLDS, draw_values

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PROGRAMS = R.programs_with_new_kind()
# one- and two-step programs, and the three-step ones in two halves
PARTS = {'n12': [p for p in PROGRAMS if len(p) < 3],
         'n3a': [p for p in PROGRAMS if len(p) == 3][0::2],
         'n3b': [p for p in PROGRAMS if len(p) == 3][1::2]}


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.mark.parametrize('part', sorted(PARTS))
@pytest.mark.parametrize('shape', _shapes()[0])
def test_every_program_with_a_new_kind_matches_numpy(shape, part):
    """7 images with mixed apply flags (image 2 with every flag 0: untouched),
    at a byte alignment that moves with the program.  43 x 127 is the largest
    image of the one-workgroup regime, 2 x 2731 the first beyond it, 231 x 227
    spans 13 tiles; beyond the regime a program with contrast is two passes,
    with the new kinds before and after it."""
    assert L.color_jitter_lds_bytes() == _shapes()[1]
    assert sum(len(v) for v in PARTS.values()) == 70 and any(CONTRAST in p for p in PARTS[part])
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + len(part))
    B = 7
    imgs = rng.integers(0, 256, (B,) + shape + (3,), dtype=np.uint8)
    imgs[1] //= 16
    imgs[3] |= 0xF0
    for n, kinds in enumerate(PARTS[part]):
        apply = rng.integers(0, 2, (len(kinds), B)).astype(np.uint8)
        apply[:, 0] = 1
        apply[:, 2] = 0
        value = draw_values(rng, kinds, B)
        got = _device_program(imgs, kinds, apply, value, lead=n % 16)
        want = R.apply_program_batch(imgs, kinds, apply, value)
        bad = [k for k in range(B) if not np.array_equal(got[k], want[k])]
        assert not bad, (shape, kinds, bad)
        assert np.array_equal(got[2], imgs[2])


def test_thresholds_and_near_integer_triples():
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (len(THRESHOLDS), 80, 80, 3), dtype=np.uint8)     # tiled regime
    imgs[:, 0, :16, 0] = np.arange(120, 136)
    thr = np.array([THRESHOLDS], np.float64)
    for im in (imgs, imgs[:, :16, :16]):
        im = np.ascontiguousarray(im)
        got = _device_program(im, (R.SOLARIZE,), np.ones((1, len(THRESHOLDS)), np.uint8), thr, lead=3)
        for k, t in enumerate(THRESHOLDS):
            assert np.array_equal(got[k], np.where(im[k] >= t, 255 - im[k], im[k])), t
    near = near_integer_triples()
    assert len(near) == 1704
    near = near.reshape(1, 24, 71, 3)
    one = np.ones((1, 1), np.uint8)
    gray = _device_program(near, (R.GRAYSCALE,), one, [[0.7]], lead=5)
    assert np.array_equal(gray, _device_program(near, (SATURATION,), one, [[0.0]], lead=2))
    assert np.array_equal(gray[0], R.step_np(near[0], R.GRAYSCALE, 0))
    host = near.copy()
    L.color_jitter_batch_host(host, [R.GRAYSCALE], one, [[0.0]])
    assert np.array_equal(host, gray)
