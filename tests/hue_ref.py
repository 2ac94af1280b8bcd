"""numpy statement of the hue contract and of the draws of
RandomHue (op id 12) and RandomColorJitter (op id 13): what the host twins, the
kernels and the transforms are checked against.  Every float32 operation is a
numpy statement of its own, so every intermediate is rounded on its own."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed
from tests.color_jitter_ref import BRIGHTNESS, CONTRAST, SATURATION, jitter_np

OP_HUE, OP_JOINT = 12, 13
F = np.float32
# sector i -> which of V, Q, P, T each channel takes
_SECTOR = {'R': 'VQPPTV', 'G': 'TVVQPP', 'B': 'PPTVVQ'}


def shift6(d):
    return F(np.float64(6.0) * np.float64(d))


def hue_np(img, d, contracted=False):
    """A new uint8 array: img (..., 3) with every pixel's hue turned by d.
    ``contracted``: 1 - s * f and 1 - s * (1 - f) with the product kept exact
    (float64) and ONE rounding, as a fused multiply-add computes them: the
    deliberately wrong order of tests/test_hue.py."""
    img = np.asarray(img, np.uint8)
    D = shift6(d)
    r = img[..., 0].astype(np.int64)
    g = img[..., 1].astype(np.int64)
    b = img[..., 2].astype(np.int64)
    mx = np.maximum(r, np.maximum(g, b))
    mn = np.minimum(r, np.minimum(g, b))
    c = mx - mn
    gray = c == 0
    C = np.where(gray, 1, c).astype(F)
    V = np.where(gray, 1, mx).astype(F)
    red = mx == r
    green = (mx == g) & (mx != r)
    num = np.where(red, g - b, np.where(green, b - r, r - g)).astype(F)
    base = np.where(red, 0, np.where(green, 2, 4)).astype(F)
    q = num / C
    x = base + q
    x = x + D
    x = np.where(x < F(0), x + F(6), x)
    x = np.where(x >= F(6), x - F(6), x)
    fl = np.floor(x)
    i = fl.astype(np.int64)
    assert i.min() >= 0 and i.max() <= 5, (i.min(), i.max())
    f = x - fl
    s = C / V
    oms = F(1) - s
    P = V * oms
    omf = F(1) - f
    if contracted:
        s64, f64, omf64 = s.astype(np.float64), f.astype(np.float64), omf.astype(np.float64)
        omsf = (1.0 - s64 * f64).astype(F)        # float32 x float32 is exact in float64
        omsomf = (1.0 - s64 * omf64).astype(F)
    else:
        sf = s * f
        omsf = F(1) - sf
        somf = s * omf
        omsomf = F(1) - somf
    Q = V * omsf
    T = V * omsomf
    for a in (x, f, s, P, Q, T):
        assert a.dtype == F
    vals = {'V': V, 'Q': Q, 'P': P, 'T': T}
    out = np.empty_like(img)
    for ch, name in enumerate('RGB'):
        v = np.select([i == k for k in range(6)], [vals[_SECTOR[name][k]] for k in range(6)])
        assert v.min() >= 0 and v.max() <= 255
        out[..., ch] = np.where(gray, img[..., ch], np.rint(v).astype(np.uint8))
    return out


def all_triples():
    """All 2^24 RGB triples as one 4096 x 4096 image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def hue_draw(seed, epoch, sid, p, magnitude):
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_HUE))
    apply = bool(rs.rand() < p)
    return apply, np.float64(rs.uniform(-magnitude, magnitude))


def joint_draw(seed, epoch, sid, p, mags):
    """(apply, [b, c, s, h] values): five draws from one stream."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), OP_JOINT))
    apply = bool(rs.rand() < p)
    vals = [np.float64(rs.uniform(max(0, 1 - m), 1 + m)) for m in mags[:3]]
    vals.append(np.float64(rs.uniform(-mags[3], mags[3])))
    return apply, vals


def joint_np(img, mags, apply, vals):
    """The sequential numpy chain b -> c -> s -> h on one image (a new array)."""
    out = np.array(img, np.uint8, copy=True)
    if not apply:
        return out
    for kind, m, v in zip((BRIGHTNESS, CONTRAST, SATURATION), mags[:3], vals[:3]):
        if m != 0:
            out = jitter_np(out, kind, v)
    if mags[3] != 0:
        out = hue_np(out, vals[3])
    return out


def joint_batch(imgs, ids, seed, epoch, p, mags):
    return np.stack([joint_np(im, mags, *joint_draw(seed, epoch, sid, p, mags)) for im, sid in zip(imgs, ids)])
