"""RandomAdjustSharpness (the reference has none: the semantics
are Pillow's ``ImageEnhance.Sharpness(img).enhance(factor)``, pinned as float32
arithmetic that numpy reproduces bit for bit, tests/sharpness_ref.py).

Each sample draws ``rand() < p`` from its own MT19937 under the seeding
contract (op id 19).  An applied uint8 (H, W, 3) image is blended with its
3 x 3 smoothed version, ``smooth + factor (image - smooth)``: factor 0 gives the
smoothed image, 1 the image itself, 2 a sharpened one.  The outermost ring of
pixels, and an image below 3 x 3, is unchanged.

On device tensors it is the draw launch plus ONE launch (ffcv_sharpness_batch:
a workgroup per image or per band of rows, the source staged in LDS); images
that are not applied are copied by the same launch.  On host arrays it is the
host twins over the Loader's threads.
"""
import math
import numbers
from typing import Callable, Optional, Tuple

import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .u8_image import _U8ImageOp


class RandomAdjustSharpness(_U8ImageOp):
    """Randomly adjust the sharpness of the image.
    Operates on raw arrays (not tensors).

    Parameters
    ----------
    sharpness_factor : float
        0 smooths the image, 1 leaves it as it is, 2 sharpens it; finite, in
        [0, 16].
    p : float
        probability to apply
    """
    op_id = 19

    def __init__(self, sharpness_factor, p=0.5):
        super().__init__()
        if isinstance(sharpness_factor, bool) or not isinstance(sharpness_factor, numbers.Real) or \
                not math.isfinite(sharpness_factor) or not 0 <= sharpness_factor <= 16:
            raise ValueError('RandomAdjustSharpness: sharpness_factor must be a finite number in [0, 16], got '
                             f'{sharpness_factor!r}')
        self.sharpness_factor = float(sharpness_factor)
        self.p = self.check_p('RandomAdjustSharpness', p)

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        factor, p = self.sharpness_factor, self.p
        key = ('sharpness', id(self))

        def device(ctx, images, out):
            apply = ctx.device_buffer(key + ('apply',), ctx.batch_size, ch.uint8)
            factors = ctx.device_buffer(key + ('factor',), ctx.batch_size, ch.float32)
            L.sharpness_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, factor, apply, factors, None,
                                   ctx.stream)
            L.sharpness_batch(images, out, apply, factors, 0, ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            apply, factors = L.sharpness_draw_batch_host(ids, seed, epoch, p, factor)
            L.sharpness_batch_host(src, out_np, apply, factors, nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        self.check_u8_images(previous_state)
        return self.declare_out_of_place(previous_state)
