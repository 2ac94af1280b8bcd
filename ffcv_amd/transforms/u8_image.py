"""What the per-sample operations on uint8 (H, W, 3) images share: the check
of ``p``, the state they declare, and the fields the graph lowering sets on an
operation that another operation's launch runs for it."""
from dataclasses import replace
from typing import Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline import runtime
from ..pipeline.operation import Operation
from ..pipeline.state import State


def check_u8_images(label, previous_state: State):
    """(dtype, shape) of a state of uint8 (H, W, 3) images; anything else raises."""
    dt, shape = previous_state.dtype, previous_state.shape
    is_u8 = dt == ch.uint8 if isinstance(dt, ch.dtype) else np.dtype(dt) == np.uint8
    if not is_u8 or shape is None or len(shape) != 3 or shape[2] != 3:
        raise TypeError(f'{label} works on uint8 (H, W, 3) images, got {dt} {tuple(shape or ())}: '
                        'place it before ToTorchImage / NormalizeImage / Convert')
    return dt, shape


class _U8ImageOp(Operation):
    device_aware = True
    per_sample = True

    def __init__(self):
        super().__init__()
        self._absorbed = False   # the graph lowering: another operation's launch runs this one
        self._program = [self]   # the run this operation leads

    @property
    def _label(self):
        return getattr(self, '_name', type(self).__name__)

    @staticmethod
    def check_p(name, p):
        try:
            pf = float(p)
        except (TypeError, ValueError):
            raise ValueError(f'{name}: p must be a number, got {p!r}')
        if not 0 <= pf <= 1:
            raise ValueError(f'{name}: p must lie in [0, 1], got {p!r}')
        return p

    @staticmethod
    def identity():
        """The code of an absorbed operation."""
        def fused(images, *_):
            return images
        return fused

    def out_of_place_code(self, device, host):
        """The code of an operation that writes a batch into ``dst``.  On a
        device batch ``device(ctx, images, out)`` makes the draws and the pixel
        launches; on a host one ``host(seed, epoch, ids, src, out_np, nthreads)``
        makes the host draws and runs the host twins on C-contiguous arrays.
        ``out``: the batch's part of ``dst``, which the code returns."""
        label = self._label

        def code(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                if not images.is_contiguous():
                    raise TypeError(f'{label}: a contiguous (B, H, W, 3) batch is required')
                out = dst[:int(images.shape[0])]
                device(ctx, images, out)
                return out
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            src = np.ascontiguousarray(images.numpy() if isinstance(images, ch.Tensor) else images)
            B = len(indices)
            out = dst[:B]
            out_np = out.numpy() if isinstance(out, ch.Tensor) else out
            from ..pipeline.compiler import Compiler
            host(seed, epoch, np.asarray(indices, np.uint64), src[:B], out_np, max(1, int(Compiler.num_threads)))
            return out
        code.is_parallel = True
        code.with_indices = True
        return code

    def check_u8_images(self, previous_state: State):
        return check_u8_images(self._label, previous_state)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        """In place."""
        dt, _ = self.check_u8_images(previous_state)
        return replace(previous_state, jit_mode=previous_state.device.type == 'cpu'
                       and not isinstance(dt, ch.dtype)), None

    def declare_out_of_place(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        """Into a destination of the input's shape, on the input's device."""
        dt, shape = previous_state.dtype, previous_state.shape
        if previous_state.device.type == 'cuda':
            return (replace(previous_state, jit_mode=False),
                    AllocationQuery(tuple(shape), dt, previous_state.device))
        return (replace(previous_state, jit_mode=not isinstance(dt, ch.dtype)), AllocationQuery(tuple(shape), dt))
