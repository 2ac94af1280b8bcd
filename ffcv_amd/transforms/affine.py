"""RandomAffine and RandomRotation (the reference has no
geometric warp: the semantics are this project's own, pinned as arithmetic
that numpy reproduces).

Each sample draws seven values from its own MT19937 under the seeding contract
(op id 14), always all seven: ``rand() < p``, the angle, the whole-pixel
translations ``rint(uniform(-a W, a W))`` and ``rint(uniform(-b H, b H))``, the
scale, and the two shears.  The inverse matrix about the image centre is
computed in float64 and quantised to six Q16 integers; from there on every
pixel is integer arithmetic (nearest, or bilinear with 8-bit weights), with a
constant ``fill`` border.  A positive angle turns the picture clockwise on
screen.

On device tensors it is the draw launch plus ONE launch (ffcv_affine_batch: a
workgroup per image or per tile of outputs, the source footprint staged in
LDS); images that are not applied are copied by the same launch.  On host
arrays it is the host twins over the Loader's threads.
"""
import math
import numbers
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..libffcv import fill_u8
from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .u8_image import _U8ImageOp

_MODES = {'bilinear': 0, 'nearest': 1}       # FFCV_AFFINE_*


def _floats(name, what, value, n):
    try:
        out = tuple(float(x) for x in value)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: {what}, got {value!r}')
    if len(out) not in n or not all(math.isfinite(x) for x in out):
        raise ValueError(f'{name}: {what}, got {value!r}')
    return out


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


class RandomAffine(_U8ImageOp):
    """Randomly rotate, translate, scale and shear the image about its centre.
    Operates on raw arrays (not tensors).

    Parameters
    ----------
    degrees : float or Tuple[float, float]
        d, meaning the range (-d, d), or the (low, high) range of the angle in
        degrees; finite, at most 360 in magnitude.
    translate : Tuple[float, float]
        (a, b) in [0, 1]: the horizontal shift is drawn from (-a W, a W), the
        vertical one from (-b H, b H), each rounded to whole pixels.
    scale : Tuple[float, float]
        The (low, high) range of the scale, 1/16 <= low <= high <= 16.
    shear : float, or a tuple of 2 or 4 floats
        x, meaning (-x, x) along x; (low, high) along x; or (x low, x high,
        y low, y high); degrees, at most 60 in magnitude.
    interpolation : str
        'bilinear' or 'nearest'.
    fill : int or Tuple[int, int, int]
        The colour outside the source image.
    p : float
        probability to warp
    """
    op_id = 14
    _name = 'RandomAffine'

    def __init__(self, degrees, translate=(0.0, 0.0), scale=(1.0, 1.0), shear=(0.0, 0.0, 0.0, 0.0),
                 interpolation='bilinear', fill=(0, 0, 0), p=1.0):
        super().__init__()
        name = self._name
        what = 'degrees must be a finite number d >= 0 or a (low, high) pair within [-360, 360]'
        if _is_number(degrees):
            d = float(degrees)
            if not (math.isfinite(d) and 0 <= d <= 360):
                raise ValueError(f'{name}: {what}, got {degrees!r}')
            self.degrees = (-d, d)
        else:
            self.degrees = _floats(name, what, degrees, (2,))
            if not -360 <= self.degrees[0] <= self.degrees[1] <= 360:
                raise ValueError(f'{name}: {what}, got {degrees!r}')
        what = 'translate must be a pair (a, b) of fractions in [0, 1]'
        self.translate = _floats(name, what, translate, (2,))
        if not all(0 <= x <= 1 for x in self.translate):
            raise ValueError(f'{name}: {what}, got {translate!r}')
        what = 'scale must be a (low, high) pair with 1/16 <= low <= high <= 16'
        self.scale = _floats(name, what, scale, (2,))
        if not 1 / 16 <= self.scale[0] <= self.scale[1] <= 16:
            raise ValueError(f'{name}: {what}, got {scale!r}')
        what = 'shear must be a finite number x >= 0, a (low, high) pair or four numbers, within [-60, 60]'
        if _is_number(shear):
            x = float(shear)
            if not (math.isfinite(x) and 0 <= x <= 60):
                raise ValueError(f'{name}: {what}, got {shear!r}')
            self.shear = (-x, x, 0.0, 0.0)
        else:
            sh = _floats(name, what, shear, (2, 4))
            self.shear = sh + (0.0, 0.0) if len(sh) == 2 else sh
            if not (-60 <= self.shear[0] <= self.shear[1] <= 60 and -60 <= self.shear[2] <= self.shear[3] <= 60):
                raise ValueError(f'{name}: {what}, got {shear!r}')
        if not isinstance(interpolation, str) or interpolation not in _MODES:
            raise ValueError(f"{name}: interpolation must be 'bilinear' or 'nearest', got {interpolation!r}")
        self.interpolation = interpolation
        try:
            f = np.asarray(fill)
            ok = f.dtype.kind in 'iuf' and f.size in (1, 3) and np.isfinite(f).all()
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'{name}: fill must be a number or an RGB triple, got {fill!r}')
        self.fill = f
        self.p = self.check_p(name, p)

    def fill_u8(self):
        return fill_u8(self.fill)

    def ranges(self, height, width):
        """The six (low, high) pairs of the draws for height x width images."""
        a, b = self.translate
        tw, th = a * width, b * height
        return self.degrees + (-tw, tw, -th, th) + self.scale + self.shear

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        p, mode, fill = self.p, _MODES[self.interpolation], self.fill_u8()
        key = ('affine', id(self))

        def device(ctx, images, out):
            H, W = int(images.shape[1]), int(images.shape[2])
            apply = ctx.device_buffer(key + ('apply',), ctx.batch_size, ch.uint8)
            coef = ctx.device_buffer(key + ('coef',), ctx.batch_size * 6, ch.int64)
            L.affine_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, self.ranges(H, W), H, W, apply, coef,
                                None, ctx.stream)
            L.affine_batch(images, out, mode, fill, apply, coef, 0, ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            H, W = src.shape[1:3]
            apply, coef = L.affine_draw_batch_host(ids, seed, epoch, p, self.ranges(H, W), H, W)
            L.affine_batch_host(src, out_np, mode, fill, apply, coef, nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if max(shape[0], shape[1]) > 32767:
            raise TypeError(f'{self._name}: images of {shape[0]}x{shape[1]} exceed the supported 32767 per side')
        return self.declare_out_of_place(previous_state)


class RandomRotation(RandomAffine):
    """Randomly rotate the image about its centre: RandomAffine with no
    translation, scale 1 and no shear, from the same stream (op id 14), so the
    same degrees and seed give the same pictures.

    Parameters
    ----------
    degrees : float or Tuple[float, float]
        d, meaning the range (-d, d), or the (low, high) range in degrees.
    interpolation : str
        'bilinear' or 'nearest'.
    fill : int or Tuple[int, int, int]
        The colour outside the source image.
    p : float
        probability to rotate
    """
    _name = 'RandomRotation'

    def __init__(self, degrees, interpolation='bilinear', fill=(0, 0, 0), p=1.0):
        super().__init__(degrees, interpolation=interpolation, fill=fill, p=p)
