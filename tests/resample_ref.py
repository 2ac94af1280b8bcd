"""numpy statement of RandomResizedCrop's 'bilinear' and 'bicubic' modes
(DESIGN.md s30), shared by test_resample*.py: Pillow's ImagingResample for
8-bit images on the crop window, that is
``Image.fromarray(img[i:i+h, j:j+w]).resize((out_w, out_h), BILINEAR | BICUBIC)``,
restated; taps clamp at the window's edge; every product and sum is rounded
on its own, in the order written."""
import numpy as np

SUPPORT = {'bilinear': 1.0, 'bicubic': 2.0}
# (window h, w) -> (out_h, out_w): the grid the statement was compared with Pillow on
SHAPES = (((1, 1), (1, 1)), ((1, 1), (5, 3)), ((2, 3), (7, 7)), ((7, 5), (3, 2)), ((64, 64), (32, 32)),
          ((33, 47), (32, 32)), ((224, 224), (224, 224)), ((224, 200), (32, 32)), ((5, 224), (64, 64)),
          ((17, 9), (64, 64)), ((256, 256), (7, 7)), ((3, 3), (224, 224)), ((200, 150), (224, 224)))


def filt(mode, x):
    x, a = abs(x), -0.5
    if mode == 'bilinear':
        return 1.0 - x if x < 1.0 else 0.0
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    return (((x - 5.0) * x + 8.0) * x - 4.0) * a if x < 2.0 else 0.0


def coeffs(n_in, n_out, mode):
    """[(xmin, int32 k[0..n))] for the n_out samples of a pass from n_in."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[mode] * fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [filt(mode, (x + xmin - center + 0.5) * (1.0 / fs)) for x in range(n)]
        ww = sum(w, 0.0)            # left to right
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * 2.0 ** 22) if v < 0 else int(0.5 + v * 2.0 ** 22) for v in w]
        out.append((xmin, np.array(k, np.int64)))
    return out


def _pass(src, n_out, mode, seen):
    """Axis 0 of src (n_in, ...) uint8 -> (n_out, ...) uint8."""
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    s64 = src.astype(np.int64)
    for xx, (xmin, k) in enumerate(coeffs(src.shape[0], n_out, mode)):
        acc = (1 << 21) + np.tensordot(k, s64[xmin:xmin + len(k)], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31
        v = acc >> 22
        seen['low'] |= bool((v < 0).any())
        seen['high'] |= bool((v > 255).any())
        seen['k'] = max(seen['k'], int(np.abs(k).max()))
        out[xx] = np.clip(v, 0, 255)
    return out


def seen():
    """What resample() records: whether a sum left 0 .. 255 on either side, and the largest |k|."""
    return {'low': False, 'high': False, 'k': 0}


def resample(img, window, out_h, out_w, mode, stats=None):
    """One uint8 (H, W, 3) image: the contract."""
    i, j, h, w = (int(x) for x in window)
    win = np.asarray(img, np.uint8)[i:i + h, j:j + w]
    stats = seen() if stats is None else stats
    mid = _pass(win.transpose(1, 0, 2), out_w, mode, stats).transpose(1, 0, 2)   # (h, out_w, 3)
    return _pass(mid, out_h, mode, stats)


def pillow_resample(win, out_h, out_w, mode):
    from PIL import Image
    f = Image.BILINEAR if mode == 'bilinear' else Image.BICUBIC
    return np.asarray(Image.fromarray(np.ascontiguousarray(win), 'RGB').resize((out_w, out_h), f))


def images(rng, h, w):
    """Two (h, w, 3) images: uniform bytes, and 0 / 255, which makes bicubic overshoot."""
    return np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
                     (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)])


def loader(fn, decoder, size, interpolation, device=None, **kw):
    """[decoder, RandomResizedCrop] on the CPU (device None) or followed by ToDevice."""
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields.decoders import IntDecoder
    from ffcv_amd.transforms import RandomResizedCrop, ToDevice, ToTensor
    ops = [decoder(), RandomResizedCrop((0.25, 1), (0.75, 4 / 3), size, interpolation=interpolation), ToTensor()]
    if device is None:
        return Loader(fn, batch_size=8, device='cpu', seed=12, drop_last=False, pipelines={'image': ops})
    return Loader(fn, batch_size=8, seed=12, drop_last=False, pipelines={
        'image': ops + [ToDevice(device)], 'label': [IntDecoder(), ToTensor(), ToDevice(device)]}, **kw)
