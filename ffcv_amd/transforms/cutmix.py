"""ImageCutMix, LabelCutMix and the per-batch Mixup/CutMix switch
(CutMix: https://arxiv.org/abs/1905.04899; the pairing and the soft labels of
the timm / DeiT / ConvNeXt recipes: "Mixup or CutMix per batch").

The conventions are those of mixup.py.  Sample i's neighbour is i - 1 of its
batch, the first takes the last (torchvision's ``roll(1)``); a batch's draws
come from ``RandomState(int(its last index))``; label rows are
``[label_i, label_{i-1}, lambda_i]``, so :class:`MixupToOneHot` serves CutMix
unchanged.  For one batch of n samples of height H and width W::

    rs = np.random.RandomState(int(last))
    same_lambda:   lam = rs.beta(alpha, alpha);    cy = rs.randint(0, H);    cx = rs.randint(0, W)
    otherwise:     lam = rs.beta(alpha, alpha, n); cy = rs.randint(0, H, n); cx = rs.randint(0, W, n)
    r  = 0.5 * np.sqrt(1.0 - lam)                        # float64
    rh = floor(r * H); rw = floor(r * W)                 # float64 product, then floor
    y1 = max(cy - rh, 0); y2 = min(cy + rh, H); x1 = max(cx - rw, 0); x2 = min(cx + rw, W)
    out[i] = in[i];  out[i][y1:y2, x1:x2, :] = in[i-1][y1:y2, x1:x2, :]      # i = 0: the batch's last sample
    lam_adj = 1.0 - ((y2 - y1) * (x2 - x1)) / float64(H * W)                 # float64, stored as float32
    label row i = [label_i, label_{i-1}, lam_adj_i]                          # float32 (n, 3)

The draws come in the order beta, rows, columns.  ``lam = 1`` gives an empty
box, which is the identity.

CutMix is a pure select: it commutes with every per-pixel operation, so
:class:`ImageCutMix` may sit AFTER ``NormalizeImage`` on the float16 batch,
where it leaves the decoder's fused epilogue alone (``ImageMixup`` has to sit
before it).  The kernel (ffcv_cutmix_batch) moves bytes and serves every
dtype and the NCHW view of channels-last storage that ``ToTorchImage`` hands
on.

These are batch-level operations that keep launch groups (``per_batch``): a
launch of several batches is cut at multiples of the Loader's batch size, drawn
per batch, and is still ONE kernel call.  The boxes are computed on the host
and reach the device through the slot's pinned float64 buffer, viewed as
int32, in one copy per launch.

The switch pair draws ``u = rs.random_sample()`` first; ``u < switch_prob``
chooses CutMix, whose draws continue on the same stream with ``cutmix_alpha``;
otherwise Mixup draws ``rs.beta(mixup_alpha, mixup_alpha[, n])``.  The leading
draw shifts the stream: a switch with ``switch_prob`` 0 or 1 does NOT draw the
lambdas or boxes of the stand-alone :class:`ImageMixup` / :class:`ImageCutMix`.
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
from .mixup import _check_args, _launch_batch_size, _is_torch_dtype, batch_bounds

LAYOUTS = ('auto', 'hwc', 'chw')


def _check_layout(name, layout):
    if layout not in LAYOUTS:
        raise ValueError(f'{name}: layout must be one of {LAYOUTS}, got {layout!r}')


def _check_image_size(name, image_size):
    ok = isinstance(image_size, (tuple, list)) and len(image_size) == 2 and all(
        isinstance(v, numbers.Integral) and not isinstance(v, bool) and v > 0 for v in image_size)
    if not ok:
        raise ValueError(f'{name}: image_size must be (height, width), two ints > 0, got {image_size!r}')
    return int(image_size[0]), int(image_size[1])


def _check_switch_prob(name, p):
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0 <= p <= 1:   # False for a NaN
        raise ValueError(f'{name}: switch_prob must be a number in [0, 1], got {p!r}')


def box_draws(rs, alpha, same_lambda, n, H, W):
    """One batch's CutMix draws on the stream ``rs``: int32 ``(m, 4)`` boxes of
    ``(y1, x1, y2, x2)`` and float64 ``(m,)`` adjusted lambdas, m = 1 with
    ``same_lambda`` and n otherwise."""
    if same_lambda:
        lam = np.array([rs.beta(alpha, alpha)])
        cy = np.array([rs.randint(0, H)], np.int64)
        cx = np.array([rs.randint(0, W)], np.int64)
    else:
        lam = rs.beta(alpha, alpha, n)
        cy = rs.randint(0, H, n).astype(np.int64)
        cx = rs.randint(0, W, n).astype(np.int64)
    r = 0.5 * np.sqrt(1.0 - lam)
    rh = np.floor(r * H).astype(np.int64)
    rw = np.floor(r * W).astype(np.int64)
    y1, y2 = np.maximum(cy - rh, 0), np.minimum(cy + rh, H)
    x1, x2 = np.maximum(cx - rw, 0), np.minimum(cx + rw, W)
    lam_adj = 1.0 - ((y2 - y1) * (x2 - x1)) / np.float64(H * W)
    return np.stack([y1, x1, y2, x2], 1).astype(np.int32), lam_adj


def cutmix_boxes(indices, batch_size, alpha, same_lambda, H, W):
    """The boxes and adjusted lambdas of a launch: one per batch
    (``same_lambda``) or one per sample, each batch drawn from
    ``RandomState(int(its last index))``."""
    bounds = batch_bounds(len(indices), batch_size)
    m = len(bounds) if same_lambda else len(indices)
    boxes, lam = np.empty((m, 4), np.int32), np.empty(m, np.float64)
    for s, (lo, hi) in enumerate(bounds):
        where = slice(s, s + 1) if same_lambda else slice(lo, hi)
        boxes[where], lam[where] = box_draws(np.random.RandomState(int(indices[hi - 1])), alpha, same_lambda,
                                             hi - lo, H, W)
    return boxes, lam


def switch_draws(indices, batch_size, mixup_alpha, cutmix_alpha, switch_prob, same_lambda, H, W):
    """The switch's draws of a launch, per sample: ``cut`` bool (batches,),
    float64 lambdas (n,) (mixup's, or CutMix's adjusted ones) and int32 boxes
    (n, 4) (empty for the mixup batches)."""
    n = len(indices)
    bounds = batch_bounds(n, batch_size)
    cut = np.zeros(len(bounds), bool)
    lam, boxes = np.empty(n, np.float64), np.zeros((n, 4), np.int32)
    for s, (lo, hi) in enumerate(bounds):
        rs = np.random.RandomState(int(indices[hi - 1]))
        cut[s] = rs.random_sample() < switch_prob
        if cut[s]:
            boxes[lo:hi], lam[lo:hi] = box_draws(rs, cutmix_alpha, same_lambda, hi - lo, H, W)
        else:
            lam[lo:hi] = rs.beta(mixup_alpha, mixup_alpha) if same_lambda else \
                rs.beta(mixup_alpha, mixup_alpha, hi - lo)
    return cut, lam, boxes


def _label_rows(labels, out, bounds, lam):
    n = int(labels.shape[0])
    col = np.asarray(labels).reshape(n, -1)[:, 0]
    for lo, hi in bounds:
        out[lo:hi, 0] = col[lo:hi]
        out[lo + 1:hi, 1] = col[lo:hi - 1]
        out[lo, 1] = col[hi - 1]
    out[:, 2] = lam
    return out


def _storage_views(images, dst, layout, who):
    """``(out, (H, W))``: the first rows of the destination buffer, viewed like
    the images (an NCHW view of channels-last storage gets the same view of
    dst), and the image size under ``layout``."""
    from .. import libffcv as L
    n = int(images.shape[0])
    _, H, W, _ = L.cutmix_geometry(who, images, layout)
    if isinstance(dst, ch.Tensor) and isinstance(images, ch.Tensor) and dst.dtype != images.dtype:
        if dst.element_size() != images.element_size():
            raise TypeError(f'{who}: {images.dtype} images for a {dst.dtype} buffer')
        dst = dst.view(images.dtype)       # bytes are moved: the buffer takes the images' dtype
    out = dst[:n]
    if isinstance(images, ch.Tensor) and images.dim() == 4 and tuple(images.shape[2:]) == (H, W) and \
            not images.is_contiguous():
        c = int(images.shape[1])
        out = dst.reshape(dst.shape[0], H, W, c).permute(0, 3, 1, 2)[:n]
    return out, (H, W)


def _host_cutmix(images, out, boxes, bs, same, layout):
    """The host twin on host tensors or arrays of any dtype."""
    from .. import libffcv as L
    if isinstance(images, ch.Tensor):
        if not images.is_contiguous():      # the NCHW view: the twin takes the storage order
            images, out = images.permute(0, 2, 3, 1), out.permute(0, 2, 3, 1)
            layout = 'hwc'
        images, out = images.numpy(), out.numpy()
    if not (images.flags.c_contiguous and out.flags.c_contiguous):
        raise TypeError('ImageCutMix: host images and their destination must be contiguous')
    L.cutmix_batch_host(images, out, boxes, bs, same, 'hwc' if layout == 'auto' else layout,
                        nthreads=Compiler.num_threads)


class ImageCutMix(Operation):
    """CutMix for images: a box of each image is replaced by the same box of
    its neighbour in the batch.  Works on host arrays of any dtype and on
    device tensors of itemsize 1, 2 or 4, before or after ``NormalizeImage``.

    Parameters
    ----------
    alpha : float
        CutMix parameter alpha: lambda is drawn from ``beta(alpha, alpha)``
        and the box covers about ``1 - lambda`` of the image
    same_lambda : bool
        Whether to use the same lambda and box across the whole batch, or
        individually sampled ones per image in the batch
    layout : str
        ``'auto'``: a 4-D tensor with channels-last strides is the NCHW view
        that ``ToTorchImage`` hands on (``H, W = shape[2:]``); anything
        contiguous is ``(B, H, W, C)``.  ``'chw'`` declares a contiguous
        ``(B, C, H, W)``, as after ``ToTorchImage(channels_last=False)`` (and
        for single-channel NCHW images, which ``'auto'`` cannot tell from
        ``(B, H, W, C)``).  ``'hwc'`` requires the contiguous ``(B, H, W, C)``.
    """
    device_aware = True
    per_batch = True

    def __init__(self, alpha: float, same_lambda: bool, layout: str = 'auto'):
        super().__init__()
        _check_args('ImageCutMix', alpha, same_lambda)
        _check_layout('ImageCutMix', layout)
        self.alpha = alpha
        self.same_lambda = bool(same_lambda)
        self.layout = layout

    def generate_code(self) -> Callable:
        alpha, same, layout = float(self.alpha), self.same_lambda, self.layout
        key = ('cutmix_boxes', id(self))

        def cutmixer(images, dst, indices):
            from .. import libffcv as L
            ctx = runtime.current()
            n = int(images.shape[0])
            bs = _launch_batch_size(ctx, n)
            out, (H, W) = _storage_views(images, dst, layout, 'ImageCutMix')
            boxes, _ = cutmix_boxes(indices, bs, alpha, same, H, W)
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                if ctx is not None and ctx.stream is not None:
                    # two float64 hold a box; sized for the slot's largest launch at once
                    host_np, host, dev = ctx.pinned_f64(key, 2 * max(n, int(ctx.batch_size)))
                    host_np.view(np.int32)[:boxes.size] = boxes.reshape(-1)
                    L.memcpy_h2d_async(dev, host, boxes.size * 4, ctx.stream)
                    L.cutmix_batch(images, out, dev.view(ch.int32), bs, same, layout, ctx.stream)
                else:
                    L.cutmix_batch(images, out, ch.from_numpy(boxes).to(images.device), bs, same, layout)
                return out
            _host_cutmix(images, out, boxes, bs, same, layout)
            return out
        cutmixer.is_parallel = True
        cutmixer.with_indices = True
        return cutmixer

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        on_dev = previous_state.device.type == 'cuda'
        dt = previous_state.dtype
        if on_dev:
            # a device state may carry a numpy dtype (NormalizeImage declares float16 as its int16 bit pattern):
            # the buffer gets the torch dtype of that size and is viewed as the tensor's own dtype when it runs
            if not isinstance(dt, ch.dtype):
                dt = ch.from_numpy(np.zeros((), dtype=dt)).dtype
            if dt.itemsize not in (1, 2, 4):
                raise TypeError(f'ImageCutMix works on device tensors of itemsize 1, 2 or 4, got {previous_state.dtype}')
        # its own buffer: a sample's neighbour is read after it may have been written
        return (previous_state, AllocationQuery(previous_state.shape, dt, previous_state.device if on_dev else None))


def _declare_labels(name, previous_state):
    if previous_state.device.type != 'cpu' or isinstance(previous_state.dtype, ch.dtype):
        raise TypeError(f'{name} works on the host label column: place it right after the label decoder, '
                        'before ToTensor / ToDevice')
    return (replace(previous_state, shape=(3,), dtype=np.dtype(np.float32)),
            AllocationQuery((3,), dtype=np.dtype(np.float32)))


class LabelCutMix(Operation):
    """CutMix for labels.  Should be initialized with the ``alpha`` and
    ``same_lambda`` of :class:`ImageCutMix` and the size of the images it
    works on: the two then draw the same boxes.  Takes the host ``(B, 1)``
    label column and returns float32 ``(B, 3)`` rows of
    ``[label_i, label_{i-1}, lam_adj_i]``, lam_adj being the share of the
    image outside the (clipped) box.

    Parameters
    ----------
    alpha : float
    same_lambda : bool
    image_size : (int, int)
        Height and width of the images at the place of :class:`ImageCutMix`:
        the adjusted lambda depends on it, and the label pipeline cannot see
        the image.
    """
    per_batch = True

    def __init__(self, alpha: float, same_lambda: bool, image_size: Tuple[int, int]):
        super().__init__()
        _check_args('LabelCutMix', alpha, same_lambda)
        self.image_size = _check_image_size('LabelCutMix', image_size)
        self.alpha = alpha
        self.same_lambda = bool(same_lambda)

    def generate_code(self) -> Callable:
        alpha, same, (H, W) = float(self.alpha), self.same_lambda, self.image_size

        def cutmixer(labels, temp_array, indices):
            n = int(labels.shape[0])
            bs = _launch_batch_size(runtime.current(), n)
            bounds = batch_bounds(n, bs)
            _, lam = cutmix_boxes(indices, bs, alpha, same, H, W)
            if same:
                lam = np.repeat(lam, [hi - lo for lo, hi in bounds])
            return _label_rows(labels, temp_array[:n], bounds, lam)
        cutmixer.is_parallel = True
        cutmixer.with_indices = True
        return cutmixer

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        return _declare_labels('LabelCutMix', previous_state)


class ImageMixupCutMix(Operation):
    """Mixup or CutMix per batch, for images.  Per batch ``u =
    RandomState(last).random_sample()``; ``u < switch_prob`` chooses CutMix
    with ``cutmix_alpha``, else Mixup with ``mixup_alpha``, both drawing on
    from the same stream (so neither draws what the stand-alone operations
    draw).  On the device, consecutive batches of a launch with the same
    choice are one call of ffcv_mixup_batch or ffcv_cutmix_batch: at most as
    many calls as the launch has batches.  Works on host arrays of any dtype
    and on uint8 or float32 device tensors (mixup's rule).

    Parameters
    ----------
    mixup_alpha, cutmix_alpha : float
    switch_prob : float
        Probability of CutMix, in [0, 1]
    same_lambda : bool
    layout : str
        As for :class:`ImageCutMix`.
    """
    device_aware = True
    per_batch = True

    def __init__(self, mixup_alpha: float, cutmix_alpha: float, switch_prob: float, same_lambda: bool,
                 layout: str = 'auto'):
        super().__init__()
        _check_args('ImageMixupCutMix', mixup_alpha, same_lambda)
        _check_args('ImageMixupCutMix', cutmix_alpha, same_lambda)
        _check_switch_prob('ImageMixupCutMix', switch_prob)
        _check_layout('ImageMixupCutMix', layout)
        self.mixup_alpha, self.cutmix_alpha, self.switch_prob = mixup_alpha, cutmix_alpha, switch_prob
        self.same_lambda = bool(same_lambda)
        self.layout = layout

    def generate_code(self) -> Callable:
        ma, ca, p = float(self.mixup_alpha), float(self.cutmix_alpha), float(self.switch_prob)
        same, layout = self.same_lambda, self.layout
        key = ('mixup_cutmix_draws', id(self))

        def switcher(images, dst, indices):
            from .. import libffcv as L
            ctx = runtime.current()
            n = int(images.shape[0])
            bs = _launch_batch_size(ctx, n)
            out, (H, W) = _storage_views(images, dst, layout, 'ImageMixupCutMix')
            cut, lam, boxes = switch_draws(indices, bs, ma, ca, p, same, H, W)
            bounds = batch_bounds(n, bs)
            # runs of consecutive batches with one choice: [lo, hi) in samples
            runs = []
            for s, (lo, hi) in enumerate(bounds):
                if runs and runs[-1][0] == cut[s]:
                    runs[-1][2] = hi
                else:
                    runs.append([cut[s], lo, hi])
            on_dev = isinstance(images, ch.Tensor) and images.device.type == 'cuda'
            if on_dev:
                # one copy per launch: n float64 lambdas, then n int32 boxes
                if ctx is not None and ctx.stream is not None:
                    host_np, host, dev = ctx.pinned_f64(key, 3 * max(n, int(ctx.batch_size)))
                    host_np[:n] = lam
                    host_np[n:3 * n].view(np.int32)[:] = boxes.reshape(-1)
                    L.memcpy_h2d_async(dev, host, 3 * n * 8, ctx.stream)
                    stream = ctx.stream
                else:
                    dev = ch.from_numpy(np.concatenate([lam, boxes.reshape(-1).view(np.float64)])).to(images.device)
                    stream = None
                d_lam, d_boxes = dev[:n], dev[n:3 * n].view(ch.int32).view(n, 4)
                for is_cut, lo, hi in runs:
                    if is_cut:
                        L.cutmix_batch(images[lo:hi], out[lo:hi], d_boxes[lo:hi], bs, False, layout, stream)
                    else:
                        L.mixup_batch(images[lo:hi], out[lo:hi], d_lam[lo:hi], bs, False, stream)
                return out
            for is_cut, lo, hi in runs:
                if is_cut:
                    _host_cutmix(images[lo:hi], out[lo:hi], boxes[lo:hi], bs, False, layout)
                    continue
                src = images[lo:hi].numpy() if isinstance(images, ch.Tensor) else images[lo:hi]
                o = out[lo:hi].numpy() if isinstance(out, ch.Tensor) else out[lo:hi]
                if src.dtype in (np.uint8, np.float32) and src.flags.c_contiguous and o.flags.c_contiguous:
                    L.mixup_batch_host(src, o, lam[lo:hi], bs, False, nthreads=Compiler.num_threads)
                else:
                    for b_lo, b_hi in batch_bounds(hi - lo, bs):
                        for i in range(b_lo, b_hi):
                            l = np.float64(lam[lo + i])
                            nb = b_hi - 1 if i == b_lo else i - 1
                            o[i] = l * src[i].astype(np.float64) + (1 - l) * src[nb].astype(np.float64)
            return out
        switcher.is_parallel = True
        switcher.with_indices = True
        return switcher

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        on_dev = previous_state.device.type == 'cuda'
        if on_dev and not _is_torch_dtype(previous_state.dtype, ch.uint8, ch.float32):
            raise TypeError(f'ImageMixupCutMix works on uint8 or float32 device tensors, got {previous_state.dtype}: '
                            'place it before NormalizeImage / Convert')
        # its own buffer: a sample's neighbour is read after it may have been written
        return (previous_state, AllocationQuery(previous_state.shape, previous_state.dtype,
                                                previous_state.device if on_dev else None))


class LabelMixupCutMix(Operation):
    """Mixup or CutMix per batch, for labels.  Should be initialized like
    :class:`ImageMixupCutMix`, with the size of the images it works on: the
    two then make the same choices and draws.  Returns float32 ``(B, 3)`` rows
    of ``[label_i, label_{i-1}, lambda_i]`` with mixup's lambda or CutMix's
    adjusted lambda.
    """
    per_batch = True

    def __init__(self, mixup_alpha: float, cutmix_alpha: float, switch_prob: float, same_lambda: bool,
                 image_size: Tuple[int, int]):
        super().__init__()
        _check_args('LabelMixupCutMix', mixup_alpha, same_lambda)
        _check_args('LabelMixupCutMix', cutmix_alpha, same_lambda)
        _check_switch_prob('LabelMixupCutMix', switch_prob)
        self.image_size = _check_image_size('LabelMixupCutMix', image_size)
        self.mixup_alpha, self.cutmix_alpha, self.switch_prob = mixup_alpha, cutmix_alpha, switch_prob
        self.same_lambda = bool(same_lambda)

    def generate_code(self) -> Callable:
        ma, ca, p = float(self.mixup_alpha), float(self.cutmix_alpha), float(self.switch_prob)
        same, (H, W) = self.same_lambda, self.image_size

        def switcher(labels, temp_array, indices):
            n = int(labels.shape[0])
            bs = _launch_batch_size(runtime.current(), n)
            _, lam, _ = switch_draws(indices, bs, ma, ca, p, same, H, W)
            return _label_rows(labels, temp_array[:n], batch_bounds(n, bs), lam)
        switcher.is_parallel = True
        switcher.with_indices = True
        return switcher

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        return _declare_labels('LabelMixupCutMix', previous_state)
