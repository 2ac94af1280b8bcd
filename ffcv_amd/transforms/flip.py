"""RandomHorizontalFlip (ffcv/transforms/flip.py:12-46).

Flip decision per sample: one double from the sample's MT19937 (op id 3)
``< flip_prob`` (the reference draws ``rand(B) < flip_prob`` for the batch,
flip.py:35).  Fused into the crop/resize kernel when it follows the
decoder; otherwise a device kernel or host numpy.  On the device it takes
uint8 (H, W, 3) images only: behind ToTorchImage, NormalizeImage or Convert it
refuses the pipeline.
"""
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.epilogue import Epilogue
from ..pipeline.state import State
from ..pipeline import runtime
from .rng import contract_seed
from .u8_image import _U8ImageOp


class RandomHorizontalFlip(_U8ImageOp):
    """Flip the image horizontally with probability flip_prob.

    Parameters
    ----------
    flip_prob : float
        The probability with which to flip each image in the batch horizontally.
    """

    def __init__(self, flip_prob: float = 0.5):
        super().__init__()
        self.flip_prob = flip_prob

    def generate_code(self) -> Callable:
        if self._absorbed:
            return self.identity()
        flip_prob = float(self.flip_prob)
        draws = Epilogue(flip=self)

        def flip(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                from .. import libffcv as L
                B = images.shape[0]
                flips = ch.empty(B, dtype=ch.uint8, device=images.device)
                p = draws.draw_params(ctx.loader_seed, ctx.epoch, 0, 0)
                L.draw_batch(ctx.batch_ids, None, p, None, None, flips, None, ctx.stream)
                out = dst[:B]
                L.flip_batch(images, out, flips, ctx.stream)
                return out
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            for i, sid in enumerate(indices):
                u = np.random.RandomState(contract_seed(seed, epoch, int(sid), 3)).uniform(0, 1)
                dst[i] = images[i, :, ::-1] if u < flip_prob else images[i]
            return dst[:len(indices)]
        flip.is_parallel = True
        flip.with_indices = True
        return flip

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        if self._absorbed:
            return previous_state, None
        if previous_state.device.type == 'cuda':   # the device kernel reads (B, H, W, 3) uint8
            self.check_u8_images(previous_state)
        return self.declare_out_of_place(previous_state)
