"""ReplaceLabel (ffcv/transforms/replace_label.py:14-50): the samples whose
DATASET index is one of ``indices`` get ``new_label``.

Like Poison it depends on a sample's own index only (``per_sample``, keeps
launch groups).  On the host label column it is one vectorised searchsorted
assignment in place; on an int64 device tensor (after ToDevice) it is one
launch of ffcv_replace_label_batch on the batch's device ids, with no transfer
back and no synchronise.
"""
import numbers
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline import runtime
from .poison import DeviceIds, check_indices, sample_ids_for


class ReplaceLabel(Operation):
    """Replace label of specified images.

    Parameters
    ----------
    indices : Sequence[int]
        The dataset indices of images to relabel.
    new_label : int
        The new label to assign.
    """
    device_aware = True
    per_sample = True
    with_indices = True

    def __init__(self, indices, new_label: int):
        super().__init__()
        if isinstance(new_label, (bool, np.bool_)) or not isinstance(new_label, (numbers.Integral, np.integer)):
            raise ValueError(f'ReplaceLabel: new_label must be an int, got {new_label!r}')
        self.indices = check_indices('ReplaceLabel', indices)
        self.new_label = int(new_label)
        self._device = DeviceIds(self.indices)

    def generate_code(self) -> Callable:
        to_change, new_label, device = self.indices, self.new_label, self._device

        def replace_label(labels, temp_array, indices):
            n = int(labels.shape[0])
            if isinstance(labels, ch.Tensor) and labels.device.type == 'cuda':
                from .. import libffcv as L
                ids, = device.tensors(labels.device)
                sample_ids, stream = sample_ids_for(runtime.current(), indices, n, labels.device)
                L.replace_label_batch(labels, sample_ids, ids, new_label, stream)
                return labels
            if len(to_change):
                sample_ix = np.asarray(indices).reshape(-1)[:n].astype(np.uint64)
                position = np.minimum(np.searchsorted(to_change, sample_ix), len(to_change) - 1)
                chosen = to_change[position] == sample_ix
                # numpy array or host tensor, (B,) or (B, 1), in its own dtype
                labels[ch.from_numpy(chosen) if isinstance(labels, ch.Tensor) else chosen] = new_label
            return labels
        replace_label.is_parallel = True
        replace_label.with_indices = True
        return replace_label

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        if previous_state.device.type == 'cuda' and previous_state.dtype != ch.int64:
            raise TypeError(f'ReplaceLabel works on int64 labels on the device, got {previous_state.dtype}: '
                            'place it before Convert, or on the host label column')
        return previous_state, None
