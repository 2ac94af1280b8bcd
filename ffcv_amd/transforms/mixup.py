"""ImageMixup, LabelMixup, MixupToOneHot (ffcv/transforms/mixup.py:17-117;
mixup: https://arxiv.org/abs/1710.09412).

The reference's mixup is deterministic: a batch seeds numpy with its last
sample index (mixup.py:40,76) and draws ``beta(alpha, alpha)`` once
(``same_lambda``) or once per sample; ``RandomState(int(indices[-1]))`` gives
the same stream.  Sample i is mixed with sample i - 1 of its batch, the first
with the last (mixup.py:46):

    out[i] = cast(float64(l_i) * float64(in[i]) + (1 - float64(l_i)) * float64(in[i - 1]))

evaluated like numpy without the numba compiler: float64, every multiply and
add rounded on its own, truncation into uint8, round-to-nearest-even into
float32.  Identical neighbours can therefore come out one BELOW the input
(``0.3 * 7 + 0.7 * 7 < 7``), as in the reference.

These are batch-level operations that keep launch groups (``per_batch``):
when the Loader runs several batches through the graph as one launch, the
operations cut their input at multiples of the Loader's batch size
(``BatchContext.launch_batch_size``), draw per batch from that batch's last
index, and the image operation is still ONE kernel call (ffcv_mixup_batch)
per launch.  Called outside a Loader, the whole input is one batch.

The lambdas are drawn on the host (legacy numpy beta is a rejection loop
with log and pow: not worth reproducing bit for bit on the device for B
doubles) and reach the device through a pinned per-slot buffer.
"""
import math
import numbers
from dataclasses import replace
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.compiler import Compiler
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline import runtime


def _check_args(name, alpha, same_lambda):
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not math.isfinite(alpha) or alpha <= 0:
        raise ValueError(f'{name}: alpha must be a finite number > 0, got {alpha!r}')
    if not isinstance(same_lambda, (bool, np.bool_)):
        raise ValueError(f'{name}: same_lambda must be a bool, got {same_lambda!r}')


def batch_bounds(n, batch_size):
    """[lo, hi) of the batches a launch of n samples holds."""
    bs = int(batch_size) if batch_size else int(n)
    return [(lo, min(int(n), lo + bs)) for lo in range(0, int(n), max(1, bs))]


def mixup_lambdas(indices, batch_size, alpha, same_lambda):
    """float64 lambdas of a launch: one per batch (``same_lambda``) or one per
    sample, each batch drawn from ``RandomState(int(its last index))``."""
    bounds = batch_bounds(len(indices), batch_size)
    lam = np.empty(len(bounds) if same_lambda else len(indices), np.float64)
    for s, (lo, hi) in enumerate(bounds):
        rs = np.random.RandomState(int(indices[hi - 1]))
        if same_lambda:
            lam[s] = rs.beta(alpha, alpha)
        else:
            lam[lo:hi] = rs.beta(alpha, alpha, hi - lo)
    return lam


def _launch_batch_size(ctx, n):
    bs = getattr(ctx, 'launch_batch_size', None) if ctx is not None else None
    return int(bs) if bs else int(n)


def _is_torch_dtype(dt, *allowed):
    return isinstance(dt, ch.dtype) and dt in allowed


class ImageMixup(Operation):
    """Mixup for images.  Works on uint8 or float32 device tensors and on host
    arrays of any dtype.

    Parameters
    ----------
    alpha : float
        Mixup parameter alpha
    same_lambda : bool
        Whether to use the same value of lambda across the whole batch, or an
        individually sampled lambda per image in the batch
    """
    device_aware = True
    per_batch = True

    def __init__(self, alpha: float, same_lambda: bool):
        super().__init__()
        _check_args('ImageMixup', alpha, same_lambda)
        self.alpha = alpha
        self.same_lambda = bool(same_lambda)

    def generate_code(self) -> Callable:
        alpha, same = float(self.alpha), self.same_lambda
        key = ('mixup_lam', id(self))

        def mixer(images, dst, indices):
            from .. import libffcv as L
            ctx = runtime.current()
            n = int(images.shape[0])
            bs = _launch_batch_size(ctx, n)
            lam = mixup_lambdas(indices, bs, alpha, same)
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                out = dst[:n]
                if images.dim() == 4 and not images.is_contiguous() and \
                        images.is_contiguous(memory_format=ch.channels_last):
                    # an NCHW view of channels-last storage: the same view of dst
                    b, c, h, w = images.shape
                    out = dst.reshape(dst.shape[0], h, w, c).permute(0, 3, 1, 2)[:n]
                if ctx is not None and ctx.stream is not None:
                    host_np, host, dev = ctx.pinned_f64(key, lam.size)
                    host_np[:lam.size] = lam
                    L.memcpy_h2d_async(dev, host, lam.size * 8, ctx.stream)
                    L.mixup_batch(images, out, dev, bs, same, ctx.stream)
                else:
                    L.mixup_batch(images, out, ch.from_numpy(lam).to(images.device), bs, same)
                return out
            src = images.numpy() if isinstance(images, ch.Tensor) else images
            out = (dst.numpy() if isinstance(dst, ch.Tensor) else dst)[:n]
            if src.dtype in (np.uint8, np.float32) and src.flags.c_contiguous and out.flags.c_contiguous:
                L.mixup_batch_host(src, out, lam, bs, same, nthreads=Compiler.num_threads)
            else:
                for s, (lo, hi) in enumerate(batch_bounds(n, bs)):
                    for i in range(lo, hi):
                        l = np.float64(lam[s] if same else lam[i])
                        nb = hi - 1 if i == lo else i - 1
                        out[i] = l * src[i].astype(np.float64) + (1 - l) * src[nb].astype(np.float64)
            return dst[:n]
        mixer.is_parallel = True
        mixer.with_indices = True
        return mixer

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        on_dev = previous_state.device.type == 'cuda'
        if on_dev and not _is_torch_dtype(previous_state.dtype, ch.uint8, ch.float32):
            raise TypeError(f'ImageMixup works on uint8 or float32 device tensors, got {previous_state.dtype}: '
                            'place it before NormalizeImage / Convert')
        # its own buffer: a sample's neighbour is read after it may have been written
        return (previous_state, AllocationQuery(previous_state.shape, previous_state.dtype,
                                                previous_state.device if on_dev else None))


class LabelMixup(Operation):
    """Mixup for labels.  Should be initialized in exactly the same way as
    :class:`ImageMixup`: the two then draw the same lambdas.  Takes the host
    ``(B, 1)`` label column and returns float32 ``(B, 3)`` rows of
    ``[label_i, label_{i-1}, lambda_i]``.
    """
    per_batch = True

    def __init__(self, alpha: float, same_lambda: bool):
        super().__init__()
        _check_args('LabelMixup', alpha, same_lambda)
        self.alpha = alpha
        self.same_lambda = bool(same_lambda)

    def generate_code(self) -> Callable:
        alpha, same = float(self.alpha), self.same_lambda

        def mixer(labels, temp_array, indices):
            ctx = runtime.current()
            n = int(labels.shape[0])
            bs = _launch_batch_size(ctx, n)
            lam = mixup_lambdas(indices, bs, alpha, same)
            col = np.asarray(labels).reshape(n, -1)[:, 0]
            out = temp_array[:n]
            for s, (lo, hi) in enumerate(batch_bounds(n, bs)):
                out[lo:hi, 0] = col[lo:hi]
                out[lo + 1:hi, 1] = col[lo:hi - 1]
                out[lo, 1] = col[hi - 1]
                out[lo:hi, 2] = lam[s] if same else lam[lo:hi]
            return out
        mixer.is_parallel = True
        mixer.with_indices = True
        return mixer

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        if previous_state.device.type != 'cpu' or isinstance(previous_state.dtype, ch.dtype):
            raise TypeError('LabelMixup works on the host label column: place it right after the label decoder, '
                            'before ToTensor / ToDevice')
        return (replace(previous_state, shape=(3,), dtype=np.dtype(np.float32)),
                AllocationQuery((3,), dtype=np.dtype(np.float32)))


class MixupToOneHot(Operation):
    """LabelMixup's ``(B, 3)`` rows as ``(B, num_classes)`` soft labels, in
    the input dtype: zeros, then ``out[i, a_i] = lambda_i``, then
    ``out[i, b_i] = 1 - lambda_i``.  When ``a_i == b_i`` the second store wins,
    so that row sums to ``1 - lambda_i`` and not to 1: this is the reference's
    behaviour (mixup.py:105-108) and is reproduced.  Unlike the reference the
    input's third column is left as it was.  A label outside
    ``[0, num_classes)`` writes nothing: on the host it raises ``IndexError``;
    on the device the sample is reported like a sample that failed to decode.

    Parameters
    ----------
    num_classes : int
        Number of classes (the width of the output).
    """
    device_aware = True
    per_sample = True

    def __init__(self, num_classes: int):
        super().__init__()
        if isinstance(num_classes, bool) or not isinstance(num_classes, numbers.Integral) or num_classes < 1:
            raise ValueError(f'MixupToOneHot: num_classes must be an int >= 1, got {num_classes!r}')
        self.num_classes = int(num_classes)

    def generate_code(self) -> Callable:
        C = self.num_classes
        key = ('onehot_status', id(self))

        def one_hotter(mixedup_labels, dst):
            n = int(mixedup_labels.shape[0])
            out = dst[:n]
            if mixedup_labels.device.type == 'cuda':
                from .. import libffcv as L
                ctx = runtime.current()
                if ctx is not None and ctx.stream is not None:
                    status = ctx.device_buffer(key, ctx.batch_size, ch.int32)[:n]
                    L.mixup_onehot_batch(mixedup_labels, out, status, ctx.stream)
                    ctx.check_status(status, 'MixupToOneHot')
                else:
                    status = ch.empty((n,), dtype=ch.int32, device=mixedup_labels.device)
                    L.mixup_onehot_batch(mixedup_labels, out, status)
                    bad = ch.nonzero(status).reshape(-1)
                    if bad.numel():
                        raise IndexError(f'MixupToOneHot: row {int(bad[0])} has a label outside [0, {C})')
                return out
            a, b = mixedup_labels[:, 0].long(), mixedup_labels[:, 1].long()
            bad = ch.nonzero((a < 0) | (a >= C) | (b < 0) | (b >= C)).reshape(-1)
            if bad.numel():
                raise IndexError(f'MixupToOneHot: row {int(bad[0])} has a label outside [0, {C})')
            rows = ch.arange(n)
            lam = mixedup_labels[:, 2]
            out.zero_()
            out[rows, a] = lam
            out[rows, b] = 1 - lam
            return out
        return one_hotter

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        dt = previous_state.dtype
        if not isinstance(dt, ch.dtype) or previous_state.shape is None or tuple(previous_state.shape) != (3,):
            raise TypeError(f'MixupToOneHot takes LabelMixup\'s (3,) rows as a tensor, got {dt} '
                            f'{tuple(previous_state.shape or ())}: place it after LabelMixup and ToTensor')
        if previous_state.device.type == 'cuda' and dt != ch.float32:
            raise TypeError(f'MixupToOneHot works on float32 device tensors, got {dt}')
        return (replace(previous_state, shape=(self.num_classes,)),
                AllocationQuery((self.num_classes,), dtype=dt, device=previous_state.device))
