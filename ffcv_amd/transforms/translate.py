"""RandomTranslate (ffcv/transforms/translate.py:13-52).

The image sits at offset ``padding`` in a canvas of ``fill`` sized
``(H + 2p, W + 2p)``; ``y = randint(0, 2p + 1)`` is drawn first, then ``x``,
and the output is the ``H x W`` window at ``(y, x)`` (translate.py:35-44):
``out[r, c] = in[r + y - p, c + x - p]`` inside the image, otherwise ``fill``.
Both draws come from the sample's own MT19937 (op id 4) under the seeding
contract.

Fused into the small-image kernel (ffcv_simple_aug_batch) when it follows a
SimpleRGBImageDecoder of raw samples (the graph lowering does this);
otherwise it runs as its own device kernel into its own buffer (shifted reads
overlap the writes, so not in place), or on host numpy arrays.  On the device
it takes uint8 (H, W, 3) images only: behind ToTorchImage, NormalizeImage or
Convert it refuses the pipeline.
"""
import numbers
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..libffcv import fill_u8
from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from ..pipeline import runtime
from .rng import contract_seed
from .u8_image import _U8ImageOp


def translate_window(image, dst, y, x, padding, fill):
    """The H x W window at (y, x) of the padded canvas, without building the
    canvas: dst[r, c] = image[r + y - padding, c + x - padding] where that is
    inside the image, otherwise fill.  ``dst`` must not alias ``image``."""
    H, W = image.shape[0], image.shape[1]
    dy, dx = int(y) - padding, int(x) - padding
    dst[:] = fill
    r0, r1 = max(0, -dy), min(H, H - dy)
    c0, c1 = max(0, -dx), min(W, W - dx)
    if r1 > r0 and c1 > c0:
        dst[r0:r1, c0:c1] = image[r0 + dy:r1 + dy, c0 + dx:c1 + dx]
    return dst


class RandomTranslate(_U8ImageOp):
    """Translate each image randomly in vertical and horizontal directions
    up to specified number of pixels.

    Parameters
    ----------
    padding : int
        Max number of pixels to translate in any direction.
    fill : tuple
        An RGB color ((0, 0, 0) by default) to fill the area outside the shifted image.
    """

    def __init__(self, padding: int, fill: Tuple[int, int, int] = (0, 0, 0)):
        super().__init__()
        if isinstance(padding, bool) or not isinstance(padding, numbers.Integral) or padding < 0:
            raise ValueError(f'RandomTranslate: padding must be an int >= 0, got {padding!r}')
        self.padding = int(padding)
        self.fill = np.array(fill)

    def fill_u8(self):
        return fill_u8(self.fill)

    def generate_code(self) -> Callable:
        if self._absorbed:
            return self.identity()
        pad = self.padding
        fill = self.fill_u8()

        def translate(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                from .. import libffcv as L
                B = images.shape[0]
                yx = ch.empty((B, 2), dtype=ch.int32, device=images.device)
                L.translate_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, pad, yx, None, ctx.stream)
                out = dst[:B]
                L.translate_batch(images, out, yx, pad, fill, ctx.stream)
                return out
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            for i, sid in enumerate(indices):
                rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), 4))
                y = rs.randint(2 * pad + 1)
                x = rs.randint(2 * pad + 1)
                translate_window(images[i], dst[i], y, x, pad, fill)
            return dst[:len(indices)]
        translate.is_parallel = True
        translate.with_indices = True
        return translate

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        if self._absorbed:
            return previous_state, None
        if previous_state.device.type == 'cuda':   # the device kernel reads (B, H, W, 3) uint8
            self.check_u8_images(previous_state)
        return self.declare_out_of_place(previous_state)
