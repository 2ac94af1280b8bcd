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

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from ..pipeline import runtime
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

        def adjust_sharpness(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                if not images.is_contiguous():
                    raise TypeError('RandomAdjustSharpness: a contiguous (B, H, W, 3) batch is required')
                B = int(images.shape[0])
                apply = ctx.device_buffer(key + ('apply',), ctx.batch_size, ch.uint8)
                factors = ctx.device_buffer(key + ('factor',), ctx.batch_size, ch.float32)
                L.sharpness_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, p, factor, apply, factors, None,
                                       ctx.stream)
                out = dst[:B]
                L.sharpness_batch(images, out, apply, factors, 0, ctx.stream)
                return out
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            src = images.numpy() if isinstance(images, ch.Tensor) else images
            src = np.ascontiguousarray(src)
            B = len(indices)
            out = dst[:B]
            out_np = out.numpy() if isinstance(out, ch.Tensor) else out
            from ..pipeline.compiler import Compiler
            apply, factors = L.sharpness_draw_batch_host(np.asarray(indices, np.uint64), seed, epoch, p, factor)
            L.sharpness_batch_host(src[:B], out_np, apply, factors, nthreads=max(1, int(Compiler.num_threads)))
            return out
        adjust_sharpness.is_parallel = True
        adjust_sharpness.with_indices = True
        return adjust_sharpness

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        self.check_u8_images(previous_state)
        return self.declare_out_of_place(previous_state)
