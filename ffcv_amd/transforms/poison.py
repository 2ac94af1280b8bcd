"""Poison (ffcv/transforms/poisoning.py:14-69): stamp a mask with a given
opacity into the samples whose DATASET index is one of ``indices``.

For a chosen sample the reference runs, on a float32 temp,

    temp[:] = image; temp *= 1 - alpha3; temp += mask.astype(float) * alpha3
    np.clip(temp, lo, hi, out=temp); image[:] = temp

(``alpha3``: ``alpha`` repeated over the 3 channels), evaluated like numpy
without the numba compiler.  With ``keep = float64(1 - alpha3)`` and ``add =
float64(mask) * alpha3``, built once with numpy exactly as the reference builds
them, that is per uint8 value

    t1 = float32(float64(v) * keep)     two separate float32 roundings;
    t2 = float32(float64(t1) + add)     for a float32 alpha the first equals
    uint8(int(min(max(t2, lo), hi)))    numpy's float32 multiply

which one function computes for the kernel (ffcv_poison_batch) and its host
twin.  The operation depends on a sample's own index only: it is
``per_sample`` and keeps launch groups, draws nothing, and runs in place on the
device batch behind the decoder with ONE launch and no host work per batch
(the batch's ids are on the device already; membership is decided there).
"""
import numbers
import threading
from dataclasses import replace
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.compiler import Compiler
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline import runtime


def check_indices(name, indices):
    """The sorted unique uint64 ids of ``indices`` (non-negative integers; an
    empty set and duplicates are allowed)."""
    arr = np.asarray(indices)
    if arr.size == 0:
        return np.zeros(0, np.uint64)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f'{name}: indices must be integers, got dtype {arr.dtype}')
    arr = arr.reshape(-1)
    if (arr < 0).any() or (arr > np.iinfo(np.int64).max).any():
        raise ValueError(f'{name}: indices must be non-negative dataset indices')
    return np.unique(arr.astype(np.uint64))


class DeviceIds:
    """The sorted ids of an operation on each device, uploaded once (as int64:
    they are below 2^63) and visible to every stream before first use."""

    def __init__(self, ids):
        self.ids = ids
        self._dev = {}
        self._lock = threading.Lock()

    def tensors(self, device, *arrays):
        """(ids, *arrays) on ``device``; the arrays' device twins are cached
        with the ids."""
        got = self._dev.get(device)
        if got is None:
            with self._lock:
                got = self._dev.get(device)
                if got is None:
                    got = tuple(ch.from_numpy(np.ascontiguousarray(a)).to(device)
                                for a in (self.ids.astype(np.int64),) + arrays)
                    ch.cuda.synchronize(device)  # uploaded before any slot stream reads them
                    self._dev[device] = got
        return got


def sample_ids_for(ctx, indices, n, device):
    """The launch's device ids: the context's, or outside a Loader an upload
    of the passed indices."""
    if ctx is not None and ctx.stream is not None and ctx.batch_ids is not None and ctx.batch_ids.numel() == n:
        return ctx.batch_ids, ctx.stream
    ids = np.ascontiguousarray(np.asarray(indices).reshape(-1)[:n]).astype(np.int64)
    return ch.from_numpy(ids).to(device), None


class Poison(Operation):
    """Poison specified images by adding a mask with given opacity.  Works in
    place on uint8 ``(H, W, 3)`` device batches and on host arrays of any
    dtype (raw arrays, before ToTorchImage / NormalizeImage).

    Parameters
    ----------
    mask : ndarray
        The mask to apply to each image, ``(H, W, 3)``.
    alpha : ndarray
        The opacity of the mask, ``(H, W)``.
    indices : Sequence[int]
        The dataset indices of the images that should have the mask applied.
    clamp : Tuple[int, int]
        Clamps the final pixel values between these two values (default:
        (0, 255)).  ``0 <= lo <= hi <= 255`` is required: outside that range
        the reference's final cast into uint8 is undefined.
    """
    device_aware = True
    per_sample = True
    with_indices = True

    def __init__(self, mask: np.ndarray, alpha: np.ndarray, indices, clamp=(0, 255)):
        super().__init__()
        mask, alpha = np.asarray(mask), np.asarray(alpha)
        for what, arr in (('mask', mask), ('alpha', alpha)):
            if arr.dtype == object or not (np.issubdtype(arr.dtype, np.number) or arr.dtype == np.bool_) or \
                    np.issubdtype(arr.dtype, np.complexfloating):
                raise ValueError(f'Poison: {what} must be a real numeric array, got dtype {arr.dtype}')
        if mask.ndim != 3 or mask.shape[2] != 3 or mask.size == 0 or alpha.shape != mask.shape[:2]:
            raise ValueError(f'Poison: mask must be (H, W, 3) and alpha (H, W), got {mask.shape} and {alpha.shape}')
        if not np.isfinite(mask).all() or not np.isfinite(alpha).all():
            raise ValueError('Poison: mask and alpha must be finite')
        try:
            lo, hi = clamp
            ok = all(isinstance(c, numbers.Real) and not isinstance(c, bool) for c in (lo, hi)) and 0 <= lo <= hi <= 255
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'Poison: clamp must be (lo, hi) with 0 <= lo <= hi <= 255, got {clamp!r}')
        self.mask = mask
        self.alpha = alpha
        self.indices = check_indices('Poison', indices)
        self.clamp = (lo, hi)
        # poisoning.py:40-41, with numpy as there
        alpha3 = np.repeat(alpha[:, :, None], 3, axis=2)
        self._alpha3 = alpha3
        self._mask_alpha = mask.astype('float') * alpha3
        self.keep = np.ascontiguousarray(1 - alpha3, dtype=np.float64)
        self.add = np.ascontiguousarray(self._mask_alpha, dtype=np.float64)
        if not np.isfinite(self.add).all():
            raise ValueError('Poison: mask * alpha overflows')
        self._device = DeviceIds(self.indices)

    def generate_code(self) -> Callable:
        to_poison, clamp = self.indices, self.clamp
        keep, add, alpha3, mask_alpha = self.keep, self.add, self._alpha3, self._mask_alpha
        device = self._device

        def poison(images, temp_array, indices):
            from .. import libffcv as L
            n = int(images.shape[0])
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                ids, d_keep, d_add = device.tensors(images.device, keep, add)
                sample_ids, stream = sample_ids_for(runtime.current(), indices, n, images.device)
                L.poison_batch(images, sample_ids, ids, d_keep, d_add, clamp, stream)
                return images
            arr = images.numpy() if isinstance(images, ch.Tensor) else images
            if arr.dtype == np.uint8 and arr.flags.c_contiguous and arr.flags.writeable and \
                    arr.shape[1:] == keep.shape:
                L.poison_batch_host(arr, indices, to_poison, keep, add, clamp, nthreads=Compiler.num_threads)
                return images
            sample_ix = np.asarray(indices).reshape(-1)[:n].astype(np.uint64)
            position = np.minimum(np.searchsorted(to_poison, sample_ix), max(0, len(to_poison) - 1))
            chosen = np.nonzero(to_poison[position] == sample_ix)[0] if len(to_poison) else ()
            for i in chosen:
                temp = temp_array[i] if temp_array is not None else np.empty(arr.shape[1:], np.float32)
                temp[:] = arr[i]
                temp *= 1 - alpha3
                temp += mask_alpha
                np.clip(temp, clamp[0], clamp[1], out=temp)
                arr[i] = temp
            return images
        poison.is_parallel = True
        poison.with_indices = True
        return poison

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        dt, shape = previous_state.dtype, previous_state.shape
        on_dev = previous_state.device.type == 'cuda'
        if on_dev:
            if dt != ch.uint8 or shape is None or len(shape) != 3 or shape[2] != 3:
                raise TypeError(f'Poison works on uint8 (H, W, 3) images on the device, got {dt} '
                                f'{tuple(shape or ())}: place it before ToTorchImage / NormalizeImage / Convert')
        if shape is None or tuple(shape) != self.mask.shape:
            raise TypeError(f'Poison: the images are {tuple(shape or ())}, the mask is {self.mask.shape}')
        if on_dev:
            return previous_state, None      # in place, no temp
        return (replace(previous_state, jit_mode=not isinstance(dt, ch.dtype)),
                AllocationQuery(shape=shape, dtype=np.dtype('float32')))
