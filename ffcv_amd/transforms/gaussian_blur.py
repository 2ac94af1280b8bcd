"""GaussianBlur (the reference has no blur: the semantics are
this project's own, pinned as arithmetic that numpy reproduces).

Each sample draws ``rand() < p`` and then ``sigma = uniform(sigma_lo,
sigma_hi)`` from its own MT19937 under the seeding contract (op id 11).  An
applied uint8 (H, W, 3) image is convolved with the ``kernel_size`` normalised
Gaussian weights of its sigma, rows then columns, in float32 with every
product and sum rounded on its own, the border reflected (reflect-101), and
rounded half to even back to uint8.

On device tensors it is the draw launch plus ONE launch
(ffcv_gaussian_blur_batch: a workgroup per image or per band of rows, the
float32 intermediate in LDS); images that are not applied are copied by the
same launch.  On host arrays it is the host twins over the Loader's threads.
"""
import math
import numbers
from typing import Callable, Optional, Tuple

import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .u8_image import _U8ImageOp


class GaussianBlur(_U8ImageOp):
    """Randomly blur the image with a Gaussian kernel of random sigma.
    Operates on raw arrays (not tensors).

    Parameters
    ----------
    kernel_size : int
        Odd number of taps per axis, 1 to 31.
    sigma : float or Tuple[float, float]
        The standard deviation, or the (low, high) range it is drawn from.
    p : float
        probability to blur
    """
    op_id = 11

    def __init__(self, kernel_size: int, sigma=(0.1, 2.0), p=0.5):
        super().__init__()
        if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Integral) or \
                not 1 <= kernel_size <= 31 or kernel_size % 2 == 0:
            raise ValueError(f'GaussianBlur: kernel_size must be an odd int in [1, 31], got {kernel_size!r}')
        try:
            lo, hi = (float(sigma),) * 2 if isinstance(sigma, numbers.Real) else (float(x) for x in sigma)
        except (TypeError, ValueError):
            raise ValueError(f'GaussianBlur: sigma must be a number or a (low, high) pair, got {sigma!r}')
        if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
            raise ValueError(f'GaussianBlur: sigma must be finite with 0 < low <= high, got {sigma!r}')
        self.kernel_size = int(kernel_size)
        self.sigma = (lo, hi)
        self.p = self.check_p('GaussianBlur', p)

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        ksize, (lo, hi), p = self.kernel_size, self.sigma, self.p
        key = ('gaussian_blur', id(self))

        def device(ctx, images, out):
            apply = ctx.device_buffer(key + ('apply',), ctx.batch_size, ch.uint8)
            sigma = ctx.device_buffer(key + ('sigma',), ctx.batch_size, ch.float64)
            weights = ctx.device_buffer(key + ('weights',), ctx.batch_size * L.BLUR_WROW, ch.float32)
            L.blur_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, lo, hi, ksize, apply, sigma, weights,
                              None, ctx.stream)
            L.gaussian_blur_batch(images, out, ksize, apply, weights, 0, ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            apply, _, weights = L.blur_draw_batch_host(ids, seed, epoch, p, lo, hi, ksize)
            L.gaussian_blur_batch_host(src, out_np, ksize, apply, weights, nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if (self.kernel_size - 1) // 2 >= min(shape[0], shape[1]):
            raise TypeError(f'GaussianBlur: kernel_size {self.kernel_size} reflects past a {shape[0]}x{shape[1]} '
                            'image ((kernel_size - 1) / 2 must be below its height and width)')
        return self.declare_out_of_place(previous_state)
