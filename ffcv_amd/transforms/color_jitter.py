"""RandomBrightness, RandomContrast, RandomSaturation
(ffcv/transforms/color_jitter.py:16-139).

Each operation draws ``rand() < p`` and then ``uniform(max(0, 1 - magnitude),
1 + magnitude)`` from the sample's own MT19937 under the seeding contract
(op id 5 brightness, 6 contrast, 7 saturation) and, where the first
draw says so, blends the uint8 HWC image in float64 like the reference:
``uint8(clip(ratio * v + (1 - ratio) * other, 0, 255))`` with ``other`` 0
(brightness), the mean of the image's uint8 gray values (contrast) or the
pixel's own gray value (saturation).

RandomGrayscale and RandomSolarization (op ids 9 and 10; the
reference has neither) are two more operations of the same family: the same
two draws, with ``uniform(0, 0)`` and ``uniform(threshold, threshold)``;
grayscale sets every channel to the pixel's gray value (saturation at ratio
0), solarization maps ``v >= threshold ? 255 - v : v``.

On device tensors a run of adjacent colour-jitter operations is ONE
ffcv_color_jitter_batch launch behind its draws (the graph lowering makes the
first operation of the run carry the program); on host arrays each operation
runs the numpy statement below, in place.
"""
import math
from typing import Callable

import numpy as np
import torch as ch

from ..pipeline import runtime
from .rng import contract_seed
from .u8_image import _U8ImageOp

_IDENT = np.arange(256, dtype=np.float64)


def gray_u8(image):
    """color_jitter.py:85: (0.2989 r + 0.587 g + 0.114 b).astype(uint8)."""
    r, g, b = image[..., 0], image[..., 1], image[..., 2]
    return (0.2989 * r + 0.587 * g + 0.114 * b).astype(np.uint8)


def _table(ratio, other):
    """blend() of every uint8 value against the scalar ``other``."""
    return (ratio * _IDENT + (1 - ratio) * other).clip(0, 255).astype(np.uint8)


def brightness_np(image, ratio):
    """In place on one uint8 (H, W, 3) image."""
    image[...] = _table(ratio, 0)[image]
    return image


def contrast_np(image, ratio):
    gray = gray_u8(image)
    mean = np.float64(int(gray.sum(dtype=np.int64))) / np.float64(gray.size)
    image[...] = _table(ratio, mean)[image]
    return image


def saturation_np(image, ratio):
    gray = gray_u8(image)
    image[...] = (ratio * image + (1 - ratio) * gray[..., None]).clip(0, 255).astype(np.uint8)
    return image


def grayscale_np(image, _ratio=0.0):
    image[...] = gray_u8(image)[..., None]
    return image


def solarize_np(image, threshold):
    image[...] = np.where(image >= threshold, 255 - image, image)
    return image


def jitter_range(magnitude):
    return max(0, 1 - magnitude), 1 + magnitude


def jitter_draw(seed, epoch, sample, op_id, p, magnitude):
    """(apply, ratio) of one sample under the seeding contract."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sample), op_id))
    apply = bool(rs.rand() < p)
    lo, hi = jitter_range(magnitude)
    return apply, np.float64(rs.uniform(lo, hi))


class _ColorJitter(_U8ImageOp):
    op_id = 0      # seeding-contract op id
    kind = 0       # FFCV_CJ_*
    host_fn = None

    def __init__(self, magnitude: float, p=0.5):
        super().__init__()
        name = type(self).__name__
        try:
            m = float(magnitude)
        except (TypeError, ValueError):
            raise ValueError(f'{name}: magnitude must be a number, got {magnitude!r}')
        if not math.isfinite(m) or m < 0:
            raise ValueError(f'{name}: magnitude must be finite and >= 0, got {magnitude!r}')
        self.magnitude = magnitude
        self.p = self.check_p(name, p)

    def draw_device(self, ctx, apply, ratio):
        """The batch's decisions into device apply uint8[B] / ratio float64[B]."""
        from .. import libffcv as L
        L.color_jitter_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, self.op_id, self.p, self.magnitude,
                                  apply, ratio, None, ctx.stream)

    def draw_host(self, seed, epoch, sample):
        return jitter_draw(seed, epoch, sample, self.op_id, self.p, self.magnitude)

    def generate_code(self) -> Callable:
        if self._absorbed:
            return self.identity()
        program = list(self._program)

        def color_jitter(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                from .. import libffcv as L
                B, n = int(images.shape[0]), len(program)
                apply = ch.empty((n, B), dtype=ch.uint8, device=images.device)
                ratio = ch.empty((n, B), dtype=ch.float64, device=images.device)
                for i, op in enumerate(program):
                    op.draw_device(ctx, apply[i], ratio[i])
                ws = None
                if int(images.shape[1]) * int(images.shape[2]) * 3 > L.color_jitter_lds_bytes() and \
                        any(op.kind == L.CJ_CONTRAST for op in program):
                    ws = ch.empty((B,), dtype=ch.int64, device=images.device)
                L.color_jitter_batch(images, [op.kind for op in program], apply, ratio, ws, ctx.stream)
                return images
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            arr = images.numpy() if isinstance(images, ch.Tensor) else images
            for i, sid in enumerate(indices):
                for op in program:
                    apply, ratio = op.draw_host(seed, epoch, sid)
                    if apply:
                        type(op).host_fn(arr[i], ratio)
            return images
        color_jitter.is_parallel = True
        color_jitter.with_indices = True
        return color_jitter


class RandomBrightness(_ColorJitter):
    """Randomly adjust image brightness. Operates on raw arrays (not tensors).

    Parameters
    ----------
    magnitude : float
        randomly choose brightness enhancement factor on [max(0, 1-magnitude), 1+magnitude]
    p : float
        probability to apply brightness
    """
    op_id, kind, host_fn = 5, 1, staticmethod(brightness_np)

    def __init__(self, magnitude: float, p=0.5):
        super().__init__(magnitude, p)


class RandomContrast(_ColorJitter):
    """Randomly adjust image contrast. Operates on raw arrays (not tensors).

    Parameters
    ----------
    magnitude : float
        randomly choose contrast enhancement factor on [max(0, 1-magnitude), 1+magnitude]
    p : float
        probability to apply contrast
    """
    op_id, kind, host_fn = 6, 2, staticmethod(contrast_np)

    def __init__(self, magnitude, p=0.5):
        super().__init__(magnitude, p)


class RandomSaturation(_ColorJitter):
    """Randomly adjust image color balance. Operates on raw arrays (not tensors).

    Parameters
    ----------
    magnitude : float
        randomly choose color balance enhancement factor on [max(0, 1-magnitude), 1+magnitude]
    p : float
        probability to apply saturation
    """
    op_id, kind, host_fn = 7, 3, staticmethod(saturation_np)

    def __init__(self, magnitude, p=0.5):
        super().__init__(magnitude, p)


class _UniformDraw(_ColorJitter):
    """A colour step whose second draw is ``uniform(lo, hi)`` with a range of
    its own (ffcv_uniform_draw_batch)."""
    lo = hi = 0.0

    def __init__(self, p):
        _U8ImageOp.__init__(self)
        self.p = self.check_p(type(self).__name__, p)

    def draw_device(self, ctx, apply, ratio):
        from .. import libffcv as L
        L.uniform_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, self.op_id, self.p, self.lo, self.hi, apply,
                             ratio, None, ctx.stream)

    def draw_host(self, seed, epoch, sample):
        rs = np.random.RandomState(contract_seed(seed, epoch, int(sample), self.op_id))
        apply = bool(rs.rand() < self.p)
        return apply, np.float64(rs.uniform(self.lo, self.hi))


class RandomGrayscale(_UniformDraw):
    """Randomly convert the image to gray (all three channels carry the
    pixel's gray value). Operates on raw arrays (not tensors).

    Parameters
    ----------
    p : float
        probability to convert
    """
    op_id, kind, host_fn = 9, 4, staticmethod(grayscale_np)

    def __init__(self, p=0.1):
        super().__init__(p)


class RandomSolarization(_UniformDraw):
    """Randomly invert every byte at or above a threshold. Operates on raw
    arrays (not tensors).

    Parameters
    ----------
    threshold : int
        bytes ``v >= threshold`` become ``255 - v``; in [0, 256]
    p : float
        probability to solarize
    """
    op_id, kind, host_fn = 10, 5, staticmethod(solarize_np)

    def __init__(self, threshold=128, p=0.5):
        import numbers
        if isinstance(threshold, bool) or not isinstance(threshold, numbers.Integral) or not 0 <= threshold <= 256:
            raise ValueError(f'RandomSolarization: threshold must be an int in [0, 256], got {threshold!r}')
        super().__init__(p)
        self.threshold = int(threshold)
        self.lo = self.hi = float(self.threshold)
