"""numpy statement of TrivialAugmentWide, shared by
test_auto_augment*.py: the three draws under the seeding contract (op id 20),
the strength of every operation at every bin with the integer forms for any
number of bins, and one sample through the SIBLING operation's statement
(tests/affine_ref.py, color_jitter_ref.py, blur_ref.py, tone_ref.py,
sharpness_ref.py) at the drawn strength."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests import affine_ref as AR
from tests import blur_ref as BR
from tests import color_jitter_ref as CR
from tests import sharpness_ref as SR
from tests import tone_ref as TR

OP_POLICY = 20
NUM_OPS = 14
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(NUM_OPS)
SIGNED = (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)


def draw(seed, epoch, sid, nbins=31):
    """(op, bin, neg) of sample sid: always all three draws."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_POLICY))
    u0, u1, u2 = rs.rand(), rs.rand(), rs.rand()
    return min(NUM_OPS - 1, int(u0 * NUM_OPS)), min(nbins - 1, int(u1 * nbins)), bool(u2 < 0.5)


# ---- the integer forms, for any number of bins (m = bin / (nbins - 1)) ----
def translate_pixels(b, nbins):
    """floor(32 m)."""
    return (32 * b) // (nbins - 1)


def posterize_bits(b, nbins):
    """8 - round-half-up(6 m) = 8 - floor((12 bin + (nbins - 1)) / (2 (nbins - 1))): 8 down to 2."""
    return 8 - (12 * b + (nbins - 1)) // (2 * (nbins - 1))


def solarize_threshold(b, nbins):
    """255 - floor(255 m): 255 down to 0."""
    return 255 - (255 * b) // (nbins - 1)


def values(nbins=31):
    """float64 (14, nbins), every value built by numpy."""
    b = np.arange(nbins)
    m = b / np.float64(nbins - 1)
    z = np.zeros(nbins)
    shear = np.degrees(np.arctan(np.float64(0.99) * m))
    px = np.array([translate_pixels(int(x), nbins) for x in b], np.float64)
    ratio = np.float64(0.99) * m
    bits = np.array([posterize_bits(int(x), nbins) for x in b], np.float64)
    thr = np.array([solarize_threshold(int(x), nbins) for x in b], np.float64)
    return np.stack([z, shear, shear, px, px, np.float64(135.0) * m, ratio, ratio, ratio, ratio, bits, thr, z, z])


def signed_value(table, op, b, neg):
    v = np.float64(table[op, b])
    return -v if neg and op in SIGNED else v


def affine_args(op, sv):
    """(angle, tx, ty, scale, shear x, shear y) of a geometric operation."""
    a = dict(angle=0.0, tx=0.0, ty=0.0, s=1.0, shx=0.0, shy=0.0)
    a[{SHEAR_X: 'shx', SHEAR_Y: 'shy', TRANSLATE_X: 'tx', TRANSLATE_Y: 'ty', ROTATE: 'angle'}[op]] = sv
    return a


def expected(img, op, b, neg, table, mode=AR.NEAREST, fill=(0, 0, 0), guard=True):
    """One uint8 (H, W, 3) image through operation `op` at bin `b`: the
    sibling operation's numpy statement at the drawn value (a new array)."""
    img = np.array(img, np.uint8)
    sv = signed_value(table, op, b, neg)
    H, W = img.shape[:2]
    if op == IDENTITY:
        return img
    if op <= ROTATE:
        m = AR.matrix_f64(H=H, W=W, **affine_args(op, sv))
        assert not guard or AR.guard_holds(m), (op, b, neg)
        return AR.warp(img, AR.quantise(m), mode, fill)
    if op in (BRIGHTNESS, COLOR, CONTRAST):
        kind = {BRIGHTNESS: CR.BRIGHTNESS, COLOR: CR.SATURATION, CONTRAST: CR.CONTRAST}[op]
        return CR.jitter_np(img, kind, np.float64(1.0) + sv)
    if op == SHARPNESS:
        return SR.sharpen(img, np.float32(np.float64(1.0) + sv))
    if op == POSTERIZE:
        return TR.step_np(img, TR.POSTERIZE, int(sv))
    if op == SOLARIZE:
        return BR.solarize(img, int(sv))
    return TR.step_np(img, TR.AUTOCONTRAST if op == AUTOCONTRAST else TR.EQUALIZE)
