"""RandomPerspective (the reference has no geometric warp: the
semantics are this project's own, pinned as arithmetic that numpy reproduces
bit for bit).

Each sample draws nine values from its own MT19937 under the seeding contract
(op id 26), always all nine: ``rand() < p`` and, in torchvision's
``get_params`` order, the eight integers of the four points where the image's
corners land.  The homography from the output to the source is computed in
closed form in float64 (products, sums and quotients only); every pixel
evaluates it in float64 with one division, floors the source coordinates to
Q16 and takes RandomAffine's integer sample (nearest, or bilinear with 8-bit
weights) with a constant ``fill`` border; a pixel on or behind the horizon is
``fill``.  A quadrilateral that is not strictly convex is not applied.

On device tensors it is the draw launch plus ONE launch
(ffcv_perspective_batch: a workgroup per image or per tile of outputs, the
source footprint staged in LDS); images that are not applied are copied by the
same launch.  On host arrays it is the host twins over the Loader's threads.
"""
import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..libffcv import fill_u8
from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .affine import _MODES, _is_number
from .u8_image import _U8ImageOp


class RandomPerspective(_U8ImageOp):
    """Randomly warp the image by a projective map.  Operates on raw arrays
    (not tensors).

    Parameters
    ----------
    distortion_scale : float
        In [0, 1]: each corner moves by up to this share of half the image's
        side towards the inside.
    p : float
        probability to warp
    interpolation : str
        'bilinear' or 'nearest'.
    fill : int or Tuple[int, int, int]
        The colour outside the source image.
    """
    op_id = 26
    _name = 'RandomPerspective'

    def __init__(self, distortion_scale=0.5, p=0.5, interpolation='bilinear', fill=(0, 0, 0)):
        super().__init__()
        name = self._name
        if not (_is_number(distortion_scale) and math.isfinite(distortion_scale) and 0 <= distortion_scale <= 1):
            raise ValueError(f'{name}: distortion_scale must be a finite number in [0, 1], got {distortion_scale!r}')
        self.distortion_scale = float(distortion_scale)
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

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        p, d, mode, fill = self.p, self.distortion_scale, _MODES[self.interpolation], self.fill_u8()
        key = ('perspective', id(self))

        def device(ctx, images, out):
            H, W = int(images.shape[1]), int(images.shape[2])
            apply = ctx.device_buffer(key + ('apply',), ctx.batch_size, ch.uint8)
            coef = ctx.device_buffer(key + ('coef',), ctx.batch_size * 9, ch.float64)
            L.perspective_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, d, H, W, apply, coef, None,
                                     ctx.stream)
            L.perspective_batch(images, out, mode, fill, apply, coef, 0, ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            H, W = src.shape[1:3]
            apply, coef = L.perspective_draw_batch_host(ids, seed, epoch, p, d, H, W)
            L.perspective_batch_host(src, out_np, mode, fill, apply, coef, nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if min(shape[0], shape[1]) < 2 or max(shape[0], shape[1]) > 32767:
            raise TypeError(f'{self._name}: images of {shape[0]}x{shape[1]} have a side outside the supported '
                            '2 .. 32767')
        return self.declare_out_of_place(previous_state)
