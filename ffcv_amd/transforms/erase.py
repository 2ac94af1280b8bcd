"""RandomErasing (https://arxiv.org/abs/1708.04896): the
``reprob`` / ``remode='pixel'`` piece of the timm / DeiT / ConvNeXt recipes,
with torchvision's ``get_params``.  The reference has none.

Each sample draws from its own MT19937 under the seeding contract (op id 21)::

    rs = np.random.RandomState(contract_seed(seed, epoch, sample, 21))
    apply = rs.random_sample() < p                   # always drawn first
    for _ in range(10):                              # drawn whether or not apply holds
        ea = (H * W) * rs.uniform(scale[0], scale[1])
        ar = exp(rs.uniform(log(ratio[0]), log(ratio[1])))
        h = int(round(sqrt(ea * ar))); w = int(round(sqrt(ea / ar)))      # half to even
        if 0 < h < H and 0 < w < W:
            y = rs.randint(H - h + 1); x = rs.randint(W - w + 1); break
    erased  <=>  apply and a try was accepted

and ``[y:y+h, x:x+w]`` of every channel becomes ``value`` (a number, or one
per channel), or with ``value='pixel'`` noise: every element takes its own
entry of a table of 4096 normal quantiles, ``mean + std * T[k]`` converted once
to the tensor's dtype, chosen by a hash of the sample's key (op id 22) and the
element's index in its sample IN STORAGE ORDER (:func:`noise_table`; HWC and
planar storage give different, both deterministic, patterns).  Nothing on that
path is floating point, so the host twin, the kernel and numpy agree bit for
bit.

It is ``per_sample`` and keeps launch groups; on device tensors it is the draw
launch plus ONE fill launch in place (ffcv_erase_batch), with no host work per
batch.  It may sit where :class:`ImageCutMix` may: before ``ToTensor`` on uint8
or after ``NormalizeImage`` on the float16 NCHW view of channels-last storage,
where ``value='pixel'`` with ``noise=(0, 1)`` is N(0, 1) in normalized units.
"""
import math
import numbers
import statistics
from dataclasses import replace
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.compiler import Compiler
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline import runtime
from .cutmix import LAYOUTS
from .poison import sample_ids_for

TABLE = 4096
_DEVICE_DTYPES = {ch.uint8: np.uint8, ch.float16: np.float16, ch.float32: np.float32}
_quantiles = None


def noise_table(mean, std, dtype):
    """``mean + std * T`` in ``dtype``, ``T[k]`` the standard normal quantile
    of ``(k + 0.5) / 4096``: float16 / float32 by numpy's cast (round to
    nearest even), uint8 as ``clip(rint(.), 0, 255)``."""
    global _quantiles
    if _quantiles is None:
        nd = statistics.NormalDist()
        _quantiles = np.array([nd.inv_cdf((k + 0.5) / TABLE) for k in range(TABLE)], np.float64)
    t = float(mean) + float(std) * _quantiles
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(t), 0, 255).astype(np.uint8)
    if dtype not in (np.float16, np.float32):
        raise TypeError(f'RandomErasing: value=\'pixel\' works on uint8, float16 and float32, got {dtype}')
    return t.astype(dtype)


def _finite(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)


def _two(name, v, lo_ok, what):
    try:
        a, b = v
        ok = _finite(a) and _finite(b) and lo_ok(a) and a <= b
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'RandomErasing: {name} must be {what}, got {v!r}')
    return float(a), float(b)


class RandomErasing(Operation):
    """Randomly erase a rectangle of each image, in place.  Works on host
    arrays and on uint8, float16 and float32 device tensors.

    Parameters
    ----------
    p : float
        probability that a sample is erased
    scale : (float, float)
        range of the erased share of the image's area, within [0, 1]
    ratio : (float, float)
        range of the box's aspect ratio (height over width), > 0
    value : number, sequence of numbers or ``'pixel'``
        The fill: one number, one per channel, or per-element noise.  On
        uint8 the numbers must be integers in 0..255.
    noise : (float, float)
        mean and standard deviation of the ``'pixel'`` noise, in the units of
        the tensor it is applied to
    layout : str
        As for :class:`ImageCutMix`: what "channel" and "storage order" mean.
    """
    device_aware = True
    per_sample = True
    with_indices = True

    def __init__(self, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0, noise=(0.0, 1.0), layout='auto'):
        super().__init__()
        if not _finite(p) or not 0 <= p <= 1:
            raise ValueError(f'RandomErasing: p must be a number in [0, 1], got {p!r}')
        self.p = float(p)
        self.scale = _two('scale', scale, lambda a: a >= 0, 'two increasing numbers in [0, 1]')
        if self.scale[1] > 1:
            raise ValueError(f'RandomErasing: scale must be two increasing numbers in [0, 1], got {scale!r}')
        self.ratio = _two('ratio', ratio, lambda a: a > 0, 'two increasing numbers > 0')
        if isinstance(value, str):
            if value != 'pixel':
                raise ValueError(f'RandomErasing: value must be a finite number, a sequence of them or \'pixel\', '
                                 f'got {value!r}')
            self.value = 'pixel'
        else:
            vals = [value] if isinstance(value, numbers.Real) else value
            try:
                vals = list(vals)
                ok = len(vals) > 0 and all(_finite(v) for v in vals)
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f'RandomErasing: value must be a finite number, a sequence of them or \'pixel\', '
                                 f'got {value!r}')
            self.value = tuple(vals)
        try:
            mean, std = noise
            ok = _finite(mean) and _finite(std) and std >= 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'RandomErasing: noise must be (mean, std) with a finite mean and std >= 0, got {noise!r}')
        self.noise = (float(mean), float(std))
        if layout not in LAYOUTS:
            raise ValueError(f'RandomErasing: layout must be one of {LAYOUTS}, got {layout!r}')
        self.layout = layout
        self._fills = {}

    def fill_for(self, dtype, channels):
        """(numpy fill, noise mode): the table in ``dtype``, or the pixel of
        ``channels`` values in it (the bytes are the same for HWC and planar
        storage)."""
        dtype = np.dtype(dtype)
        if dtype == np.int16:       # NormalizeImage hands float16 on as its int16 bit pattern on the host
            dtype = np.dtype(np.float16)
        got = self._fills.get((dtype, channels))
        if got is None:
            if self.value == 'pixel':
                got = noise_table(self.noise[0], self.noise[1], dtype), True
            else:
                if len(self.value) not in (1, channels):
                    raise TypeError(f'RandomErasing: value has {len(self.value)} numbers, the images {channels} '
                                    'channels')
                vals = np.broadcast_to(np.asarray(self.value, np.float64), (channels,))
                if dtype.kind in 'iu':
                    info = np.iinfo(dtype)
                    if (vals != np.rint(vals)).any() or (vals < info.min).any() or (vals > info.max).any():
                        raise ValueError(f'RandomErasing: on {dtype} images value must hold integers in '
                                         f'{info.min}..{info.max}, got {self.value!r}')
                got = np.ascontiguousarray(vals.astype(dtype)).view(np.uint8), False
            self._fills[(dtype, channels)] = got
        return got

    def generate_code(self) -> Callable:
        p, scale, ratio, layout = self.p, self.scale, self.ratio, self.layout
        key = ('erase', id(self))

        def on_device(images, indices, ctx):
            from .. import libffcv as L
            n = int(images.shape[0])
            np_dt = _DEVICE_DTYPES.get(images.dtype)
            if np_dt is None:
                raise TypeError(f'RandomErasing works on uint8, float16 and float32 device tensors, got {images.dtype}')
            planes, H, W, pb = L.cutmix_geometry('RandomErasing', images, layout)
            fill_np, noisy = self.fill_for(np_dt, planes * pb // images.element_size())
            ids, stream = sample_ids_for(ctx, indices, n, images.device)
            if stream is not None:
                cap = max(n, int(ctx.batch_size))
                boxes = ctx.device_buffer(key + ('boxes',), 4 * cap, ch.int32)
                keys = ctx.device_buffer(key + ('keys',), cap, ch.int64) if noisy else None
                fkey = key + ('fill', images.dtype)
                fresh = fkey not in ctx._staging
                fill = ctx.device_buffer(fkey, fill_np.size, ch.from_numpy(fill_np[:0]).dtype)
                if fresh:   # once per slot, in stream order in front of the slot's first fill
                    with ch.cuda.stream(stream):
                        fill.copy_(ch.from_numpy(fill_np))
                seed, epoch = ctx.loader_seed, ctx.epoch
            else:
                boxes = ch.empty(4 * n, dtype=ch.int32, device=images.device)
                keys = ch.empty(n, dtype=ch.int64, device=images.device) if noisy else None
                fill = ch.from_numpy(fill_np).to(images.device)
                seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            L.erase_draw_batch(ids, seed, epoch, p, scale, ratio, H, W, boxes, keys, None, stream)
            L.erase_batch(images, boxes, fill, keys, layout, stream)
            return images

        def erase(images, _, indices):
            from .. import libffcv as L
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                return on_device(images, indices, ctx)
            arr, lay = images, layout
            if isinstance(images, ch.Tensor):
                if not images.is_contiguous():      # the NCHW view: the twin takes the storage order
                    L.cutmix_geometry('RandomErasing', images, layout)
                    arr, lay = images.permute(0, 2, 3, 1), 'hwc'
                arr = arr.numpy()
            if not (arr.flags.c_contiguous and arr.flags.writeable):
                raise TypeError('RandomErasing: host images must be contiguous and writeable')
            n = int(arr.shape[0])
            planes, H, W, pb = L.cutmix_geometry('RandomErasing', arr, lay)
            fill_np, noisy = self.fill_for(arr.dtype, planes * pb // arr.itemsize)
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            ids = np.asarray(indices).reshape(-1)[:n].astype(np.uint64)
            boxes, keys = L.erase_draw_batch_host(ids, seed, epoch, p, scale, ratio, H, W)
            L.erase_batch_host(arr, boxes, fill_np, keys if noisy else None, lay,
                               nthreads=max(1, int(Compiler.num_threads)))
            return images
        erase.is_parallel = True
        erase.with_indices = True
        return erase

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        dt = previous_state.dtype
        on_dev = previous_state.device.type == 'cuda'
        # NormalizeImage declares float16 as its int16 bit pattern: on the device the dtype is the tensor's own when
        # it runs, on the host an int16 array is taken as float16 bits
        np_dt = _DEVICE_DTYPES.get(dt) if isinstance(dt, ch.dtype) else np.dtype(dt)
        declared_bits = not isinstance(dt, ch.dtype) and np_dt == np.int16
        if on_dev and not declared_bits and (np_dt is None or np_dt not in _DEVICE_DTYPES.values()):
            raise TypeError(f'RandomErasing works on uint8, float16 and float32 device tensors, got {dt}')
        if self.value == 'pixel' and not declared_bits and (np_dt is None or np_dt not in _DEVICE_DTYPES.values()):
            raise TypeError(f'RandomErasing: value=\'pixel\' works on uint8, float16 and float32, got {dt}')
        # (a per-channel value of the wrong length fails at the first run, where the layout is known)
        if on_dev:
            return previous_state, None      # in place, no memory
        return replace(previous_state, jit_mode=not isinstance(dt, ch.dtype)), None
