"""numpy statement of RandAugment, shared by
test_randaugment*.py: the two draws per slot under the seeding contract (op id
23), the strength of every operation at every bin with the integer forms for
any number of bins and any image shape, and one sample through its slots, each
the sibling operation's statement (tests/auto_augment_ref.expected) on the
uint8 result of the slot before."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests import affine_ref as AR
from tests import auto_augment_ref as R

OP_RANDAUGMENT = 23
NUM_OPS = R.NUM_OPS


def draw(seed, epoch, sid, num_ops):
    """[(op, neg)] of sample sid, one pair per slot: always both draws."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_RANDAUGMENT))
    out = []
    for _ in range(num_ops):
        u0, u1 = rs.rand(), rs.rand()
        out.append((min(NUM_OPS - 1, int(u0 * NUM_OPS)), bool(u1 < 0.5)))
    return out


# ---- the integer forms, for any number of bins (m = bin / (nbins - 1)) ----
def translate_pixels(b, nbins, side):
    """floor(150 / 331 * side * m)."""
    return (150 * side * b) // (331 * (nbins - 1))


def posterize_bits(b, nbins):
    """8 - round-half-up(4 m) = 8 - floor((8 bin + (nbins - 1)) / (2 (nbins - 1))): 8 down to 4."""
    return 8 - (8 * b + (nbins - 1)) // (2 * (nbins - 1))


def solarize_threshold(b, nbins):
    """255 - floor(255 m): 255 down to 0."""
    return 255 - (255 * b) // (nbins - 1)


def values(nbins, H, W):
    """float64 (14, nbins) for H x W images, every value built by numpy."""
    b = np.arange(nbins)
    m = b / np.float64(nbins - 1)
    z = np.zeros(nbins)
    shear = np.degrees(np.arctan(np.float64(0.3) * m))
    px = np.array([translate_pixels(int(x), nbins, W) for x in b], np.float64)
    py = np.array([translate_pixels(int(x), nbins, H) for x in b], np.float64)
    ratio = np.float64(0.9) * m
    bits = np.array([posterize_bits(int(x), nbins) for x in b], np.float64)
    thr = np.array([solarize_threshold(int(x), nbins) for x in b], np.float64)
    return np.stack([z, shear, shear, px, py, np.float64(30.0) * m, ratio, ratio, ratio, ratio, bits, thr, z, z])


def expected(img, ops, negs, magnitude, table, mode=AR.NEAREST, fill=(0, 0, 0), guard=True):
    """One uint8 (H, W, 3) image through its slots: slot s runs operation
    ops[s] at bin `magnitude`, negated where negs[s], on the result of slot
    s - 1."""
    img = np.array(img, np.uint8)
    for op, neg in zip(ops, negs):
        img = R.expected(img, op, magnitude, neg, table, mode, fill, guard)
    return img
