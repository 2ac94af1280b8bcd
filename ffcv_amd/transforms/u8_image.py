"""What the per-sample operations on uint8 (H, W, 3) images share: the check
of ``p``, the state they declare, and the fields the graph lowering sets on an
operation that another operation's launch runs for it."""
from dataclasses import replace
from typing import Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
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
