"""ElasticTransform (the reference has no geometric warp: the
semantics are this project's own, pinned as integer arithmetic that numpy
reproduces byte for byte).

Every pixel has a displacement of its own.  A sample's key is the full 64-bit
hash of the seeding contract (op id 27; no MT19937 stream and no draw launch);
each pixel and axis takes 16 bits of ``splitmix64(key ^ index)`` as Q15 noise
in [-1, 1).  The noise is blurred by torchvision's Gaussian (``int(8 sigma +
1)`` taps, made odd; 16-bit integer weights summing to 65536; ``reflect``
border), scaled by ``alpha / 2`` pixels, and added to the pixel's own
coordinates in Q16; the pixel is RandomAffine's integer sample (nearest, or
bilinear with 8-bit weights) there, with a constant ``fill`` border.

On device tensors it is ONE launch (ffcv_elastic_batch: a workgroup per tile
of outputs rebuilds the tile's field in LDS and stages the source box its own
displacements reach).  On host arrays it is the host twin over the Loader's
threads.  It is always applied: torchvision's has no ``p``.
"""
import math
from typing import Callable, Optional, Tuple

import numpy as np

from ..libffcv import fill_u8
from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .affine import _MODES, _is_number
from .u8_image import _U8ImageOp

MAX_R, MAX_ALPHA = 64, 4096


class ElasticTransform(_U8ImageOp):
    """Warp the image by a smoothed random displacement field.  Operates on
    raw arrays (not tensors).

    Parameters
    ----------
    alpha : float
        In [0, 4096]: the displacements reach alpha / 2 pixels.
    sigma : float
        At least 1: the smoothness of the field.  The blur's radius
        ``int(8 sigma + 1) // 2`` is at most 64 and below the image's sides.
    interpolation : str
        'bilinear' or 'nearest'.
    fill : int or Tuple[int, int, int]
        The colour outside the source image.
    """
    op_id = 27
    _name = 'ElasticTransform'

    def __init__(self, alpha=50.0, sigma=5.0, interpolation='bilinear', fill=(0, 0, 0)):
        super().__init__()
        name = self._name
        if not (_is_number(alpha) and math.isfinite(alpha) and 0 <= alpha <= MAX_ALPHA):
            raise ValueError(f'{name}: alpha must be a number in [0, {MAX_ALPHA}], got {alpha!r}')
        if not (_is_number(sigma) and math.isfinite(sigma) and sigma >= 1 and self.radius(sigma) <= MAX_R):
            raise ValueError(f'{name}: sigma must be a number from 1 on with int(8 sigma + 1) // 2 <= {MAX_R}, '
                             f'got {sigma!r}')
        self.alpha, self.sigma = float(alpha), float(sigma)
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

    @staticmethod
    def radius(sigma):
        """Taps on each side of the blur's centre (torchvision's kernel size)."""
        k = int(8 * float(sigma) + 1)
        return (k + (k % 2 == 0) - 1) // 2

    def fill_u8(self):
        return fill_u8(self.fill)

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        alpha, sigma, mode, fill = self.alpha, self.sigma, _MODES[self.interpolation], self.fill_u8()

        def device(ctx, images, out):
            L.elastic_batch(images, out, mode, fill, ctx.batch_ids, ctx.loader_seed, ctx.epoch, alpha, sigma, 0,
                            ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            L.elastic_batch_host(src, out_np, mode, fill, ids, seed, epoch, alpha, sigma, nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if min(shape[0], shape[1]) < 2 or max(shape[0], shape[1]) > 32767:
            raise TypeError(f'{self._name}: images of {shape[0]}x{shape[1]} have a side outside the supported '
                            '2 .. 32767')
        if self.radius(self.sigma) > min(shape[0], shape[1]) - 1:
            raise TypeError(f'{self._name}: sigma {self.sigma} blurs over {self.radius(self.sigma)} pixels a side, '
                            f'images of {shape[0]}x{shape[1]} carry {min(shape[0], shape[1]) - 1}')
        return self.declare_out_of_place(previous_state)
