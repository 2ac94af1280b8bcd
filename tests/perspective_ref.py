"""The RandomPerspective contract as plain numpy: the nine
draws under the seeding contract, the convexity rule in exact integers, the
float64 coefficients with every operation a statement of its own, and a
pixel's float64 coordinates, floored to Q16 and sampled by tests/affine_ref.py."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests import affine_ref as A

OP_PERSPECTIVE = 26
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)
F = np.float64


def corners(H, W):
    return [0, 0, W - 1, 0, W - 1, H - 1, 0, H - 1]


def draws(seed, epoch, sid, p, d, H, W):
    """(apply, [x0, y0, .. x3, y3]): always all nine draws, in this order."""
    rs = np.random.RandomState(contract_seed(seed, epoch, sid, OP_PERSPECTIVE))
    apply = bool(rs.random_sample() < p)
    bw, bh = int(np.floor(F(d) * F(W // 2))), int(np.floor(F(d) * F(H // 2)))

    def randint(lo, hi):
        return lo + min(int(np.floor(F(rs.random_sample()) * F(hi - lo + 1))), hi - lo)
    rx, ry = (W - 1 - bw, W - 1), (H - 1 - bh, H - 1)
    return apply, [randint(*r) for r in ((0, bw), (0, bh), rx, (0, bh), rx, ry, (0, bw), ry)]


def convex(q):
    P = [(int(q[2 * i]), int(q[2 * i + 1])) for i in range(4)]
    return all((P[(i + 1) % 4][0] - P[i][0]) * (P[(i + 2) % 4][1] - P[(i + 1) % 4][1]) -
               (P[(i + 1) % 4][1] - P[i][1]) * (P[(i + 2) % 4][0] - P[(i + 1) % 4][0]) > 0 for i in range(4))


def coefficients(quad, H, W):
    """The nine float64 coefficients of the quadrilateral (x0, y0, .. x3, y3)."""
    x0, y0, x1, y1, x2, y2, x3, y3 = (int(v) for v in quad)
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    dn = F(dx2 * dy1 - dx1 * dy2)
    with np.errstate(all='ignore'):
        g, h = F(sy * dx2 - sx * dy2) / dn, F(dy1 * sx - dx1 * sy) / dn
        a, b, c = F(x1 - x0) + g * F(x1), F(x3 - x0) + h * F(x3), F(x0)
        d, e, f = F(y1 - y0) + g * F(y1), F(y3 - y0) + h * F(y3), F(y0)
        adj = [e - f * h, c * h - b, b * f - c * e, f * g - d, a - c * g, c * d - a * f,
               d * h - e * g, b * g - a * h, a * e - b * d]
        det = (a * adj[0] + b * adj[3]) + c * adj[6]
        if not (det > 0 and np.isfinite(det)):
            return None
        scale = [F(W - 1)] * 3 + [F(H - 1)] * 3
        return np.array([(v * s) / det for v, s in zip(adj, scale)] + [v / det for v in adj[6:]], np.float64)


def draw_coefficients(seed, epoch, sid, p, d, H, W):
    """(apply, coefficients) of one sample."""
    apply, quad = draws(seed, epoch, sid, p, d, H, W)
    q = coefficients(quad, H, W) if convex(quad) else None
    return (apply, q) if q is not None else (False, IDENTITY.copy())


def warp(img, q, mode, fill=(0, 0, 0)):
    """One uint8 (H, W, 3) image under the nine float64 coefficients."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape[:2]
    fill = np.broadcast_to(np.asarray(fill).astype(np.uint8).reshape(-1), (3,))
    q = np.asarray(q, np.float64)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    with np.errstate(all='ignore'):
        nx = (q[0] * c + q[1] * r) + q[2]
        ny = (q[3] * c + q[4] * r) + q[5]
        den = (q[6] * c + q[7] * r) + q[8]
        w = F(1.0) / den
        X, Y = nx * w, ny * w
        ok = (den > 0) & (np.abs(X) < 65536) & (np.abs(Y) < 65536)      # NaN and inf fail
        Xq = np.floor(np.where(ok, X, 0) * F(65536.0)).astype(np.int64)
        Yq = np.floor(np.where(ok, Y, 0) * F(65536.0)).astype(np.int64)
    if mode == A.NEAREST:
        out = A._taps(img, (Yq + 32768) >> 16, (Xq + 32768) >> 16, fill)
    else:
        ix, iy = Xq >> 16, Yq >> 16
        fx, fy = ((Xq & 0xFFFF) >> 8)[:, :, None], ((Yq & 0xFFFF) >> 8)[:, :, None]
        top = (256 - fx) * A._taps(img, iy, ix, fill) + fx * A._taps(img, iy, ix + 1, fill)
        bot = (256 - fx) * A._taps(img, iy + 1, ix, fill) + fx * A._taps(img, iy + 1, ix + 1, fill)
        out = ((256 - fy) * top + fy * bot + 32768) >> 16
    return np.where(ok[:, :, None], out, fill.astype(np.int64)).astype(np.uint8)


def warp_batch(imgs, coef, mode, apply, fill=(0, 0, 0)):
    return np.stack([warp(im, q, mode, fill) if a else np.array(im) for im, q, a in zip(imgs, coef, apply)])
