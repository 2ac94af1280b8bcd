"""numpy statement of AugMix, shared by test_augmix*.py: the
chain draws (op id 24) and the weight draws (op id 25, RandomState's own
standard_gamma) under the seeding contract, the value table's integer forms,
and one sample: every chain as tests/randaugment_ref.expected from the
original, then the float32 mix."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests import affine_ref as AR
from tests import auto_augment_ref as R

OP_CHAINS, OP_WEIGHTS = 24, 25
OPS_ALL = tuple(range(1, 14))
OPS_BASIC = (R.SHEAR_X, R.SHEAR_Y, R.TRANSLATE_X, R.TRANSLATE_Y, R.ROTATE, R.POSTERIZE, R.SOLARIZE, R.AUTOCONTRAST,
             R.EQUALIZE)


def draw_chains(seed, epoch, sid, severity, width, chain_depth, all_ops):
    """[[(op, bin, neg)] * depth] of sample sid, one list per chain: always ten draws per chain."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_CHAINS))
    ops = OPS_ALL if all_ops else OPS_BASIC
    chains = []
    for _ in range(width):
        ud = rs.rand()
        depth = chain_depth if chain_depth > 0 else min(3, 1 + int(ud * 3))
        steps = []
        for _ in range(3):
            u0, u1, u2 = rs.rand(), rs.rand(), rs.rand()
            steps.append((ops[min(len(ops) - 1, int(u0 * len(ops)))], min(severity - 1, int(u1 * severity)),
                          bool(u2 < 0.5)))
        chains.append(steps[:depth])
    return chains


def draw_weights(seed, epoch, sid, width, alpha):
    """float32 (width + 1,): a, b, g_0 .. in this order from one RandomState."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_WEIGHTS))
    a, b = rs.standard_gamma(alpha), rs.standard_gamma(alpha)
    g = [rs.standard_gamma(alpha) for _ in range(width)] + [0.0] * (4 - width)
    gs = ((g[0] + g[1]) + g[2]) + g[3]
    return np.array([a / (a + b)] + [(b / (a + b)) * (g[i] / gs) for i in range(width)], np.float64).astype(np.float32)


def values(H, W):
    """float64 (14, 10) for H x W images, the integer forms written out."""
    b = np.arange(10)
    m = b / np.float64(9)
    z = np.zeros(10)
    shear = np.degrees(np.arctan(np.float64(0.3) * m))
    px = np.array([(W * int(x)) // 27 for x in b], np.float64)
    py = np.array([(H * int(x)) // 27 for x in b], np.float64)
    ratio = np.float64(0.9) * m
    bits = np.array([4, 4, 3, 3, 2, 2, 1, 1, 1, 1], np.float64)
    thr = np.array([255 - (255 * int(x)) // 9 for x in b], np.float64)
    return np.stack([z, shear, shear, px, py, np.float64(30.0) * m, ratio, ratio, ratio, ratio, bits, thr, z, z])


def mix(orig, results, weights):
    """min(255, rint(w_0 x + w_1 y_0 + ..)) in float32, one rounding per product and per sum."""
    w = np.asarray(weights, np.float32)
    acc = w[0] * orig.astype(np.float32)
    for i, y in enumerate(results):
        acc = acc + w[i + 1] * y.astype(np.float32)
    assert acc.dtype == np.float32
    return np.minimum(np.float32(255), np.rint(acc)).astype(np.uint8)


def expected(img, chains, weights, table, mode=AR.NEAREST, fill=(0, 0, 0)):
    """One uint8 (H, W, 3) image: every chain [(op, bin, neg)] from the original, then the mix."""
    results = []
    for steps in chains:
        y = np.array(img, np.uint8)
        for op, b, neg in steps:
            y = R.expected(y, op, b, neg, table, mode, fill)
        results.append(y)
    return mix(np.asarray(img, np.uint8), results, weights)
