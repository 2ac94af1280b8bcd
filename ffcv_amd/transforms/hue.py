"""RandomHue and the jointly gated RandomColorJitter (the
reference's colour jitter has no hue and no joint gate: the semantics are this
project's own, pinned as arithmetic that numpy reproduces bit for bit).

``RandomHue(magnitude, p)`` draws ``rand() < p`` and then ``d =
uniform(-magnitude, magnitude)`` from the sample's own MT19937 under the
seeding contract (op id 12) and, where the first draw says so, turns the hue
of the uint8 HWC image by ``d`` of a full turn: a per-pixel RGB -> (hue,
saturation, value) -> RGB round trip in float32, every operation rounded on
its own (``hue_np`` below is the statement).

``RandomColorJitter(brightness, contrast, saturation, hue, p)`` is the colour
jitter of the self-supervised recipes (``RandomApply([ColorJitter(...)], p)``):
ONE decision for all four components.  It draws five values from one stream
(op id 13), always all five: ``rand() < p``, then the brightness, contrast and
saturation ratios (``uniform(max(0, 1 - m), 1 + m)``), then the hue shift
(``uniform(-hue, hue)``).  Where the decision is true the components with a
non-zero magnitude run in the fixed order brightness, contrast, saturation,
hue, each on the previous one's uint8 result, with the arithmetic of
RandomBrightness / RandomContrast / RandomSaturation / RandomHue.  (A
per-sample random order of the components is not offered.)

On device tensors RandomHue is its draw launch plus ffcv_hue_batch, and
RandomColorJitter the joint draw launch, ffcv_color_jitter_batch with the
program of its active brightness / contrast / saturation components, and
ffcv_hue_batch; a stage no component needs is left out.  On host arrays each
sample runs the numpy statements, in place.
"""
import math
from typing import Callable

import numpy as np
import torch as ch

from ..pipeline import runtime
from .color_jitter import brightness_np, contrast_np, saturation_np, jitter_range
from .rng import contract_seed
from .u8_image import _U8ImageOp

OP_HUE, OP_JOINT = 12, 13
_F32 = np.float32


def hue_np(image, d):
    """In place on one uint8 (H, W, 3) image: the hue turned by ``d`` of a full
    turn (|d| <= 0.5).  float32 throughout, every operation a numpy statement
    of its own."""
    D = _F32(np.float64(6.0) * np.float64(d))
    px = image.reshape(-1, 3)
    r, g, b = (px[:, j].astype(np.int32) for j in range(3))
    mx = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    c = mx - mn
    colour = c != 0
    C = np.where(colour, c, 1).astype(_F32)   # gray pixels: computed on stand-ins, kept as they are
    V = np.where(colour, mx, 1).astype(_F32)
    is_r = mx == r
    is_g = (mx == g) & ~is_r
    num = np.where(is_r, g - b, np.where(is_g, b - r, r - g)).astype(_F32)
    base = np.where(is_r, _F32(0), np.where(is_g, _F32(2), _F32(4))).astype(_F32)
    x = base + num / C
    x = x + D
    x = np.where(x < 0, x + _F32(6), x)
    x = np.where(x >= 6, x - _F32(6), x)
    fl = np.floor(x)
    f = x - fl
    i = fl.astype(np.int32)
    s = C / V
    one = _F32(1)
    P = V * (one - s)
    Q = V * (one - s * f)
    T = V * (one - s * (one - f))
    out = np.stack([np.choose(i, [V, Q, P, P, T, V], mode='clip'),
                    np.choose(i, [T, V, V, Q, P, P], mode='clip'),
                    np.choose(i, [P, P, T, V, V, Q], mode='clip')], axis=1)
    assert out.dtype == np.float32
    image[...] = np.where(colour[:, None], np.rint(out).astype(np.uint8), px).reshape(image.shape)
    return image


def hue_draw(seed, epoch, sample, p, magnitude):
    """(apply, d) of one sample under the seeding contract (op id 12)."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sample), OP_HUE))
    apply = bool(rs.rand() < p)
    return apply, np.float64(rs.uniform(-magnitude, magnitude))


def joint_draw(seed, epoch, sample, p, magnitudes):
    """(apply, [brightness ratio, contrast ratio, saturation ratio, hue shift])
    of one sample: five draws from one stream (op id 13)."""
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sample), OP_JOINT))
    apply = bool(rs.rand() < p)
    values = [np.float64(rs.uniform(*jitter_range(m))) for m in magnitudes[:3]]
    values.append(np.float64(rs.uniform(-magnitudes[3], magnitudes[3])))
    return apply, values


def _number(cls, name, value):
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f'{cls}: {name} must be a number, got {value!r}')


def _check_hue(cls, name, value):
    m = _number(cls, name, value)
    if not (math.isfinite(m) and 0 <= m <= 0.5):
        raise ValueError(f'{cls}: {name} must be finite and lie in [0, 0.5], got {value!r}')
    return m


class RandomHue(_U8ImageOp):
    """Randomly turn the image's hue. Operates on raw arrays (not tensors).

    Parameters
    ----------
    magnitude : float
        randomly choose the hue shift, as a fraction of a full turn, on
        [-magnitude, magnitude]; in [0, 0.5]
    p : float
        probability to apply hue
    """
    op_id = OP_HUE

    def __init__(self, magnitude: float, p=0.5):
        super().__init__()
        _check_hue('RandomHue', 'magnitude', magnitude)
        self.magnitude = magnitude
        self.p = self.check_p('RandomHue', p)

    def generate_code(self) -> Callable:
        p, magnitude = float(self.p), float(self.magnitude)
        key = ('random_hue', id(self))

        def random_hue(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                from .. import libffcv as L
                B = int(images.shape[0])
                apply = ctx.device_buffer(key + ('apply',), B, ch.uint8)
                shift = ctx.device_buffer(key + ('shift',), B, ch.float64)
                L.hue_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, magnitude, apply, shift, None,
                                 ctx.stream)
                L.hue_batch(images, apply, shift, ctx.stream)
                return images
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            arr = images.numpy() if isinstance(images, ch.Tensor) else images
            for i, sid in enumerate(indices):
                apply, d = hue_draw(seed, epoch, sid, p, magnitude)
                if apply:
                    hue_np(arr[i], d)
            return images
        random_hue.is_parallel = True
        random_hue.with_indices = True
        return random_hue


class RandomColorJitter(_U8ImageOp):
    """Randomly jitter brightness, contrast, saturation and hue under ONE
    decision, in that order. Operates on raw arrays (not tensors).

    Parameters
    ----------
    brightness, contrast, saturation : float
        randomly choose each enhancement factor on [max(0, 1-m), 1+m]; a
        component with magnitude 0 is drawn but not run
    hue : float
        randomly choose the hue shift on [-hue, hue]; in [0, 0.5]
    p : float
        probability to apply the whole jitter
    """
    op_id = OP_JOINT

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, p=0.8):
        super().__init__()
        for name, v in (('brightness', brightness), ('contrast', contrast), ('saturation', saturation)):
            m = _number('RandomColorJitter', name, v)
            if not math.isfinite(m) or m < 0:
                raise ValueError(f'RandomColorJitter: {name} must be finite and >= 0, got {v!r}')
        _check_hue('RandomColorJitter', 'hue', hue)
        self.brightness, self.contrast, self.saturation, self.hue = brightness, contrast, saturation, hue
        self.p = self.check_p('RandomColorJitter', p)

    @property
    def magnitudes(self):
        return [float(self.brightness), float(self.contrast), float(self.saturation), float(self.hue)]

    def generate_code(self) -> Callable:
        p, mags = float(self.p), self.magnitudes
        active = [j for j in range(4) if mags[j] != 0.0]
        kinds = [j + 1 for j in active if j < 3]  # FFCV_CJ_BRIGHTNESS / CONTRAST / SATURATION
        has_hue = 3 in active
        host_fns = (brightness_np, contrast_np, saturation_np, hue_np)
        key = ('random_color_jitter', id(self))

        def random_color_jitter(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                if not active:
                    return images
                from .. import libffcv as L
                B, rows = int(images.shape[0]), len(active)
                apply = ctx.device_buffer(key + ('apply',), rows * B, ch.uint8)[:rows * B].view(rows, B)
                ratio = ctx.device_buffer(key + ('ratio',), rows * B, ch.float64)[:rows * B].view(rows, B)
                L.color_jitter_joint_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, mags, apply, ratio,
                                                None, ctx.stream)
                if kinds:
                    ws = None
                    if int(images.shape[1]) * int(images.shape[2]) * 3 > L.color_jitter_lds_bytes() and \
                            L.CJ_CONTRAST in kinds:
                        ws = ctx.device_buffer(key + ('ws',), B, ch.int64)
                    L.color_jitter_batch(images, kinds, apply, ratio, ws, ctx.stream)
                if has_hue:
                    L.hue_batch(images, apply[rows - 1], ratio[rows - 1], ctx.stream)
                return images
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            arr = images.numpy() if isinstance(images, ch.Tensor) else images
            for i, sid in enumerate(indices):
                apply, values = joint_draw(seed, epoch, sid, p, mags)
                if apply:
                    for j in active:
                        host_fns[j](arr[i], values[j])
            return images
        random_color_jitter.is_parallel = True
        random_color_jitter.with_indices = True
        return random_color_jitter
