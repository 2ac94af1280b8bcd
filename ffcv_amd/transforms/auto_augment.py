"""TrivialAugmentWide (the reference has no augmentation
policy: the operations are this project's own, at the strengths of the
TrivialAugment paper's wide space).

Every sample runs exactly ONE of 14 operations at a random strength.  It draws
three values from its own MT19937 under the seeding contract (op id 20),
always all three::

    op  = min(13, int(rand() * 14))
    bin = min(nbins - 1, int(rand() * nbins))
    neg = rand() < 0.5

and looks its strength up in ``value_table(nbins)[op, bin]``, negated where
``neg`` and the operation is signed:

    0 Identity                 5 Rotate (degrees, +-)        10 Posterize (bits)
    1 / 2 ShearX / ShearY      6 / 7 / 8 Brightness / Color  11 Solarize (threshold)
          (degrees, +-)              / Contrast (ratio 1 +- v) 12 AutoContrast
    3 / 4 TranslateX / Y       9 Sharpness (factor 1 +- v)   13 Equalize
          (whole pixels, +-)

The arithmetic of each is that of the sibling operation: RandomAffine's
matrix and warp, RandomBrightness / RandomSaturation / RandomContrast /
RandomSolarization, RandomAdjustSharpness, RandomPosterize /
RandomAutocontrast / RandomEqualize.

On device tensors it is one draw launch (ffcv_policy_draw_batch: which sample
runs what is decided on the device, the host does nothing per batch) and five
pixel launches, each of which skips the images that drew another operation:
colour jitter (two programs: a colour program has at most three steps, and
there are four colour operations) and the tone tables in place on the input,
the warp into the output (it copies every image that is not warped), sharpness into the output
(only the images that drew it).  On host arrays it is the host twins of the
same entries.
"""
import numbers
from typing import Callable, Optional, Tuple

import numpy as np
import torch as ch

from ..libffcv import fill_u8
from ..pipeline.allocation_query import AllocationQuery
from ..pipeline.state import State
from .affine import _MODES
from .u8_image import _U8ImageOp

NUM_OPS = 14
OP_NAMES = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast',
            'Sharpness', 'Posterize', 'Solarize', 'AutoContrast', 'Equalize')
SIGNED_OPS = range(1, 10)
# FFCV_CJ_BRIGHTNESS, SATURATION, CONTRAST | SOLARIZE: rows 0 .. 2 and row 3 of the draws' colour arrays (a
# colour program has at most three steps, so solarize is a program of its own)
_CJ_STEPS, _SOLARIZE_STEPS = (1, 3, 2), (5,)
_TONE_STEPS = (1, 2, 3)       # FFCV_TONE_POSTERIZE, AUTOCONTRAST, EQUALIZE


def value_table(nbins):
    """float64 (14, nbins): the strength of every operation at every bin, with
    m = bin / (nbins - 1).  Built once, on the host; the draws index it."""
    b = np.arange(nbins, dtype=np.int64)
    m = b.astype(np.float64) / np.float64(nbins - 1)
    t = np.zeros((NUM_OPS, nbins), np.float64)
    t[1] = t[2] = np.degrees(np.arctan(np.float64(0.99) * m))
    t[3] = t[4] = (32 * b) // (nbins - 1)
    t[5] = np.float64(135.0) * m
    t[6] = t[7] = t[8] = t[9] = np.float64(0.99) * m
    t[10] = 8 - (12 * b + (nbins - 1)) // (2 * (nbins - 1))      # 8 - round-half-up(6 m): 8 .. 2
    t[11] = 255 - (255 * b) // (nbins - 1)                       # 255 - floor(255 m): 255 .. 0
    return t


class TrivialAugmentWide(_U8ImageOp):
    """Apply one randomly chosen operation of 14, at a random strength, to
    every image.  Operates on raw arrays (not tensors).

    Parameters
    ----------
    num_magnitude_bins : int
        The number of strengths an operation is drawn from, in [2, 256].
    interpolation : str
        'nearest' or 'bilinear', for the geometric operations.
    fill : int or Tuple[int, int, int]
        The colour outside the source image, for the geometric operations.
    """
    op_id = 20

    def __init__(self, num_magnitude_bins=31, interpolation='nearest', fill=(0, 0, 0)):
        super().__init__()
        name = 'TrivialAugmentWide'
        if isinstance(num_magnitude_bins, bool) or not isinstance(num_magnitude_bins, numbers.Integral) or \
                not 2 <= num_magnitude_bins <= 256:
            raise ValueError(f'{name}: num_magnitude_bins must be an int in [2, 256], got {num_magnitude_bins!r}')
        if not isinstance(interpolation, str) or interpolation not in _MODES:
            raise ValueError(f"{name}: interpolation must be 'bilinear' or 'nearest', got {interpolation!r}")
        try:
            f = np.asarray(fill)
            ok = f.dtype.kind in 'iuf' and f.size in (1, 3) and np.isfinite(f).all()
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'{name}: fill must be a number or an RGB triple, got {fill!r}')
        self.num_magnitude_bins = int(num_magnitude_bins)
        self.interpolation = interpolation
        self.fill = f
        self.table = value_table(self.num_magnitude_bins)
        self._dev_tables = {}

    def device_table(self, device):
        t = self._dev_tables.get(device)
        if t is None:
            t = self._dev_tables[device] = ch.from_numpy(self.table).to(device)
        return t

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        nbins, mode, fill, table = self.num_magnitude_bins, _MODES[self.interpolation], fill_u8(self.fill), self.table
        key = ('trivial_augment', id(self))

        def device(ctx, images, out):
            B, H, W = (int(x) for x in images.shape[:3])
            d = {}
            for name, dt, shape in L.POLICY_ARRAYS:
                shp = shape(B)
                n = int(np.prod(shp))
                d[name] = ctx.device_buffer(key + (name,), int(np.prod(shape(ctx.batch_size))),
                                            getattr(ch, np.dtype(dt).name))[:n].view(shp)
            L.policy_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, nbins, self.device_table(images.device),
                                H, W, d, None, ctx.stream)
            cj_ws = tone_ws = None
            if H * W * 3 > L.color_jitter_lds_bytes():
                cj_ws = ctx.device_buffer(key + ('cj_ws',), ctx.batch_size, ch.int64)[:B]
            if H * W * 3 > L.tone_lds_bytes():
                tone_ws = ctx.device_buffer(key + ('tone_ws',), 768 * ctx.batch_size, ch.int32)[:768 * B]
            L.color_jitter_batch(images, _CJ_STEPS, d['cj_apply'][:3], d['cj_ratio'][:3], cj_ws, ctx.stream)
            L.color_jitter_batch(images, _SOLARIZE_STEPS, d['cj_apply'][3:], d['cj_ratio'][3:], None, ctx.stream)
            L.tone_batch_bits(images, _TONE_STEPS, d['tone_apply'], d['tone_bits'], tone_ws, ctx.stream)
            L.affine_batch(images, out, mode, fill, d['aff_apply'], d['aff_coef'], 0, ctx.stream)
            L.sharpness_batch(images, out, d['sharp_apply'], d['sharp_factor'], 0, ctx.stream)

        def host(seed, epoch, ids, src, out_np, nthreads):
            H, W = src.shape[1:3]
            d = L.policy_draw_batch_host(ids, seed, epoch, nbins, table, H, W)
            L.color_jitter_batch_host(src, _CJ_STEPS, d['cj_apply'][:3], d['cj_ratio'][:3])
            L.color_jitter_batch_host(src, _SOLARIZE_STEPS, d['cj_apply'][3:], d['cj_ratio'][3:])
            L.tone_batch_bits_host(src, _TONE_STEPS, d['tone_apply'], d['tone_bits'])
            L.affine_batch_host(src, out_np, mode, fill, d['aff_apply'], d['aff_coef'], nthreads=nthreads)
            L.sharpness_batch_host(src, out_np, d['sharp_apply'], d['sharp_factor'], nthreads=nthreads)
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if max(shape[0], shape[1]) > 32767:
            raise TypeError(f'TrivialAugmentWide: images of {shape[0]}x{shape[1]} exceed the supported 32767 per side')
        return self.declare_out_of_place(previous_state)
