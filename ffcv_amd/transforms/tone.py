"""RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
(the reference has none of them: the semantics are Pillow's
``ImageOps.posterize`` / ``autocontrast`` (cutoff 0) / ``equalize`` (no mask) /
``invert``, pinned as arithmetic that numpy reproduces bit for bit).

Each operation makes ONE draw per sample, ``rand() < p``, from the sample's
own MT19937 under the seeding contract (op id 15 posterize, 16 autocontrast,
17 equalize, 18 invert) and, where the draw says so, maps every channel of the
uint8 HWC image through a 256-entry table of its own: fixed for posterize and
invert, built from the channel's first and last occupied value for
autocontrast and from its histogram for equalize (the ``*_table`` functions
below are the statements).

On device tensors a run of adjacent table operations is ONE draw launch plus
ONE ffcv_tone_batch (the graph lowering makes the first operation of the run
carry the program); on host arrays each operation runs the numpy statement, in
place.
"""
import numbers
from typing import Callable

import numpy as np
import torch as ch

from ..pipeline import runtime
from .rng import contract_seed
from .u8_image import _U8ImageOp

OP_POSTERIZE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT = 15, 16, 17, 18
_IDENT = np.arange(256, dtype=np.uint8)


def posterize_table(bits):
    """ImageOps.posterize: keep the ``bits`` high bits of every byte."""
    return _IDENT & np.uint8(0xFF & ~(2 ** (8 - bits) - 1))


def invert_table():
    return (255 - _IDENT).astype(np.uint8)


def autocontrast_table(h):
    """ImageOps.autocontrast (cutoff 0) for a channel with histogram ``h``:
    float64, the product and the sum each rounded on its own, truncated."""
    nz = np.flatnonzero(h)
    if nz.size == 0 or nz[-1] <= nz[0]:
        return _IDENT.copy()
    lo, hi = int(nz[0]), int(nz[-1])
    scale = np.float64(255.0) / np.float64(hi - lo)
    offset = np.float64(-lo) * scale
    return np.clip(np.trunc(_IDENT.astype(np.float64) * scale + offset), 0, 255).astype(np.uint8)


def equalize_table(h):
    """ImageOps.equalize (no mask) for a channel with histogram ``h``."""
    h = np.asarray(h, dtype=np.int64)
    nz = np.flatnonzero(h)
    if nz.size < 2:
        return _IDENT.copy()
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return _IDENT.copy()
    below = np.cumsum(h) - h
    return np.minimum(255, (step // 2 + below) // step).astype(np.uint8)


def _map_channels(image, table_of):
    for c in range(3):
        plane = image[..., c]
        plane[...] = table_of(np.bincount(plane.reshape(-1), minlength=256))[plane]
    return image


def posterize_np(image, bits):
    """In place on one uint8 (H, W, 3) image."""
    image[...] = posterize_table(bits)[image]
    return image


def invert_np(image, _bits=None):
    image[...] = invert_table()[image]
    return image


def autocontrast_np(image, _bits=None):
    return _map_channels(image, autocontrast_table)


def equalize_np(image, _bits=None):
    return _map_channels(image, equalize_table)


def tone_draw(seed, epoch, sample, op_id, p):
    """The decision of one sample under the seeding contract."""
    return bool(np.random.RandomState(contract_seed(seed, epoch, int(sample), op_id)).rand() < p)


class _Tone(_U8ImageOp):
    op_id = 0      # seeding-contract op id
    kind = 0       # FFCV_TONE_*
    bits = 8       # posterize's parameter
    host_fn = None

    def __init__(self, p):
        super().__init__()
        self.p = self.check_p(type(self).__name__, p)

    def generate_code(self) -> Callable:
        if self._absorbed:
            return self.identity()
        program = list(self._program)
        kinds, op_ids, ps = [op.kind for op in program], [op.op_id for op in program], [float(op.p) for op in program]
        bits = next((op.bits for op in program if op.kind == 1), 8)
        needs_stats = any(op.kind in (2, 3) for op in program)
        key = ('tone', id(self))

        def tone(images, dst, indices):
            ctx = runtime.current()
            if isinstance(images, ch.Tensor) and images.device.type == 'cuda':
                from .. import libffcv as L
                B, n = int(images.shape[0]), len(program)
                apply = ctx.device_buffer(key + ('apply',), n * B, ch.uint8)[:n * B].view(n, B)
                L.tone_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, op_ids, ps, apply, None, ctx.stream)
                ws = None
                if needs_stats and int(images.shape[1]) * int(images.shape[2]) * 3 > L.tone_lds_bytes():
                    ws = ctx.device_buffer(key + ('ws',), 768 * B, ch.int32)[:768 * B]
                L.tone_batch(images, kinds, bits, apply, ws, ctx.stream)
                return images
            seed, epoch = (ctx.loader_seed, ctx.epoch) if ctx else (0, 0)
            arr = images.numpy() if isinstance(images, ch.Tensor) else images
            for i, sid in enumerate(indices):
                for op in program:
                    if tone_draw(seed, epoch, sid, op.op_id, op.p):
                        type(op).host_fn(arr[i], op.bits)
            return images
        tone.is_parallel = True
        tone.with_indices = True
        return tone


class RandomPosterize(_Tone):
    """Randomly keep only the high bits of every byte. Operates on raw arrays
    (not tensors).

    Parameters
    ----------
    bits : int
        bits kept per channel; in [1, 8]
    p : float
        probability to posterize
    """
    op_id, kind, host_fn = OP_POSTERIZE, 1, staticmethod(posterize_np)

    def __init__(self, bits, p=0.5):
        if isinstance(bits, bool) or not isinstance(bits, numbers.Integral) or not 1 <= bits <= 8:
            raise ValueError(f'RandomPosterize: bits must be an int in [1, 8], got {bits!r}')
        super().__init__(p)
        self.bits = int(bits)


class RandomAutocontrast(_Tone):
    """Randomly stretch every channel so that its darkest value becomes 0 and
    its lightest 255. Operates on raw arrays (not tensors).

    Parameters
    ----------
    p : float
        probability to apply autocontrast
    """
    op_id, kind, host_fn = OP_AUTOCONTRAST, 2, staticmethod(autocontrast_np)

    def __init__(self, p=0.5):
        super().__init__(p)


class RandomEqualize(_Tone):
    """Randomly equalize every channel's histogram. Operates on raw arrays
    (not tensors).

    Parameters
    ----------
    p : float
        probability to equalize
    """
    op_id, kind, host_fn = OP_EQUALIZE, 3, staticmethod(equalize_np)

    def __init__(self, p=0.5):
        super().__init__(p)


class RandomInvert(_Tone):
    """Randomly invert every byte. Operates on raw arrays (not tensors).

    Parameters
    ----------
    p : float
        probability to invert
    """
    op_id, kind, host_fn = OP_INVERT, 4, staticmethod(invert_np)

    def __init__(self, p=0.5):
        super().__init__(p)
