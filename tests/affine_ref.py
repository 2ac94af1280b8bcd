"""The RandomAffine / RandomRotation contract as plain numpy:
the seven draws under the seeding contract, the float64 matrix with every
operation a statement of its own, the Q16 quantisation, the guard for
comparisons of drawn coefficients, and both pixel modes on int64 arrays."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed

OP_AFFINE = 14
BILINEAR, NEAREST = 0, 1
M_MAX, B_MAX = 1 << 23, 1 << 40
K = np.float64(0.017453292519943295)
IDENTITY = (65536, 0, 0, 0, 65536, 0)

# the three configurations of the guard statement (loader seed 7, epoch 0, ids 0 .. 255)
CONFIGS = (dict(degrees=30, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=(-10, 10, -10, 10)),
           dict(degrees=180),
           dict(degrees=0, translate=(0.25, 0.25), scale=(0.5, 2.0), shear=(-20, 20, 0, 0)))
GUARD_SHAPES = ((32, 32), (97, 131), (224, 224))


def ranges(H, W, degrees, translate=(0.0, 0.0), scale=(1.0, 1.0), shear=(0.0, 0.0, 0.0, 0.0)):
    """Six (low, high) pairs in draw order: angle, tx, ty, scale, shear x, shear y."""
    deg = (-float(degrees), float(degrees)) if np.isscalar(degrees) else tuple(float(x) for x in degrees)
    if np.isscalar(shear):
        shear = (-float(shear), float(shear), 0.0, 0.0)
    elif len(shear) == 2:
        shear = tuple(shear) + (0.0, 0.0)
    a, b = (np.float64(x) for x in translate)
    tw, th = a * np.float64(W), b * np.float64(H)
    return tuple(np.float64(x) for x in deg + (-tw, tw, -th, th) + tuple(scale) + tuple(shear))


def draws(seed, epoch, sid, p, rg):
    """(apply, angle, tx, ty, s, shx, shy): always all seven, in this order."""
    rs = np.random.RandomState(contract_seed(seed, epoch, sid, OP_AFFINE))

    def uniform(lo, hi):
        return np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.float64(rs.random_sample())
    apply = bool(rs.random_sample() < p)
    angle = uniform(rg[0], rg[1])
    tx = np.rint(uniform(rg[2], rg[3]))
    ty = np.rint(uniform(rg[4], rg[5]))
    s = uniform(rg[6], rg[7])
    shx = uniform(rg[8], rg[9])
    shy = uniform(rg[10], rg[11])
    return apply, angle, tx, ty, s, shx, shy


def matrix_f64(angle, tx, ty, s, shx, shy, H, W):
    """(m00, m01, b0, m10, m11, b1) in float64."""
    angle, tx, ty, s, shx, shy = (np.float64(x) for x in (angle, tx, ty, s, shx, shy))
    rot = angle * K
    sx = shx * K
    sy = shy * K
    rs = rot - sy
    a = np.cos(rs) / np.cos(sy)
    bt = np.cos(rs) * np.tan(sx)
    b = -(bt / np.cos(sy)) - np.sin(rot)
    c = np.sin(rs) / np.cos(sy)
    dt = np.sin(rs) * np.tan(sx)
    d = -(dt / np.cos(sy)) + np.cos(rot)
    m00 = d / s
    m01 = -b / s
    m10 = -c / s
    m11 = a / s
    cx = np.float64(W - 1) / np.float64(2)
    cy = np.float64(H - 1) / np.float64(2)
    ux = -cx - tx
    uy = -cy - ty
    b0 = (m00 * ux + m01 * uy) + cx
    b1 = (m10 * ux + m11 * uy) + cy
    return np.array([m00, m01, b0, m10, m11, b1], np.float64)


def quantise(m):
    return np.rint(np.asarray(m, np.float64) * np.float64(65536.0)).astype(np.int64)


def coefficients(angle, tx=0, ty=0, s=1, shx=0, shy=0, H=1, W=1):
    return quantise(matrix_f64(angle, tx, ty, s, shx, shy, H, W))


def guard_holds(m):
    """No coefficient within 2^-20 of a rounding boundary after the scaling."""
    v = np.asarray(m, np.float64) * np.float64(65536.0)
    return bool((np.abs((v - np.floor(v)) - 0.5) > 2.0 ** -20).all())


def draw_coefficients(seed, epoch, sid, p, rg, H, W):
    """(apply, float64 matrix, int64 coefficients) of one sample."""
    apply, *vals = draws(seed, epoch, sid, p, rg)
    m = matrix_f64(*vals, H, W)
    return apply, m, quantise(m)


def coef_ok(q):
    q = [int(x) for x in q]
    return all(abs(q[i]) <= M_MAX for i in (0, 1, 3, 4)) and all(abs(q[i]) <= B_MAX for i in (2, 5))


def _taps(img, iy, ix, fill):
    """img[iy, ix] as int64 (H, W, 3), fill where the tap lies outside."""
    H, W = img.shape[:2]
    inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    v = img[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].astype(np.int64)
    return np.where(inside[:, :, None], v, np.asarray(fill, np.int64).reshape(1, 1, 3))


def warp(img, q, mode, fill=(0, 0, 0)):
    """One uint8 (H, W, 3) image under the six int64 coefficients."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    fill = np.broadcast_to(np.asarray(fill).astype(np.uint8).reshape(-1), (3,)).astype(np.int64)
    if not coef_ok(q):
        out = np.empty_like(img)
        out[:] = fill.astype(np.uint8)
        return out
    q = [np.int64(int(x)) for x in q]
    r, c = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    X = q[0] * c + q[1] * r + q[2]
    Y = q[3] * c + q[4] * r + q[5]
    if mode == NEAREST:
        return _taps(img, (Y + 32768) >> 16, (X + 32768) >> 16, fill).astype(np.uint8)
    ix, iy = X >> 16, Y >> 16
    fx, fy = ((X & 0xFFFF) >> 8)[:, :, None], ((Y & 0xFFFF) >> 8)[:, :, None]
    top = (256 - fx) * _taps(img, iy, ix, fill) + fx * _taps(img, iy, ix + 1, fill)
    bot = (256 - fx) * _taps(img, iy + 1, ix, fill) + fx * _taps(img, iy + 1, ix + 1, fill)
    out = ((256 - fy) * top + fy * bot + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def warp_batch(imgs, coef, mode, apply, fill=(0, 0, 0)):
    return np.stack([warp(im, q, mode, fill) if a else np.array(im) for im, q, a in zip(imgs, coef, apply)])


def expected(img, seed, epoch, sid, mode, H=None, W=None, fill=(0, 0, 0), p=1.0, **config):
    """One image through RandomAffine(**config) with the contract's draws,
    under the guard; returns (image, applied)."""
    H, W = img.shape[:2]
    apply, m, q = draw_coefficients(seed, epoch, sid, p, ranges(H, W, **config), H, W)
    assert guard_holds(m), (seed, epoch, sid)
    return (warp(img, q, mode, fill) if apply else np.array(img, np.uint8)), apply
