"""TrivialAugmentWide and RandAugment (the reference has
no augmentation policy: the operations are this project's own, at the strengths
of the TrivialAugment paper's wide space and of torchvision's RandAugment).
RandAugment, which runs several operations per sample, is described at its
class below; this text is TrivialAugmentWide's.

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

from ..libffcv import fill_u8, RANDAUGMENT_MAX_OPS as MAX_NUM_OPS
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


def randaugment_table(nbins, H, W):
    """float64 (14, nbins): RandAugment's strength of every operation at every
    bin for H x W images, with m = bin / (nbins - 1): the ranges of
    torchvision's RandAugment (shear to 0.3, translation to 150 / 331 of the
    side, rotation to 30 degrees, the ratios to 0.9, posterize 8 down to 4 bits,
    solarize 255 down to 0).  Posterize rounds half up (8 - round-half-up(4 m)),
    the convention of ``value_table``; torch's ``round`` is half-to-even and
    differs only at exact ties."""
    b = np.arange(nbins, dtype=np.int64)
    m = b.astype(np.float64) / np.float64(nbins - 1)
    t = np.zeros((NUM_OPS, nbins), np.float64)
    t[1] = t[2] = np.degrees(np.arctan(np.float64(0.3) * m))
    t[3] = (150 * int(W) * b) // (331 * (nbins - 1))
    t[4] = (150 * int(H) * b) // (331 * (nbins - 1))
    t[5] = np.float64(30.0) * m
    t[6] = t[7] = t[8] = t[9] = np.float64(0.9) * m
    t[10] = 8 - (8 * b + (nbins - 1)) // (2 * (nbins - 1))       # 8 - round-half-up(4 m): 8 .. 4
    t[11] = 255 - (255 * b) // (nbins - 1)                       # 255 - floor(255 m): 255 .. 0
    return t


class RandAugment(_U8ImageOp):
    """Apply ``num_ops`` randomly chosen operations of the 14 of
    TrivialAugmentWide in sequence to every image, each on the uint8 result of
    the one before, all at the strength of bin ``magnitude`` (the
    parameters are torchvision's ``RandAugment``).  Operates on raw arrays (not
    tensors).

    Every sample draws from one MT19937 under the seeding contract (op id 23),
    two values per slot s = 0 .. num_ops - 1, always both::

        op_s  = min(13, int(rand() * 14))
        neg_s = rand() < 0.5

    and looks its strength up in ``randaugment_table(nbins, H, W)[op, magnitude]``,
    negated where ``neg`` and the operation is signed.  The arithmetic of every
    operation is the sibling operation's, as in TrivialAugmentWide.  Posterize's
    bits round half up (torch's ``round`` is half-to-even and differs only at
    exact ties).

    On device tensors it is one draw launch (ffcv_randaugment_draw_batch) and,
    for images up to 64 x 64 (``libffcv.randaugment_lds_bytes()``), ONE pixel
    launch that keeps the image in LDS across its slots (ffcv_randaugment_batch);
    beyond, slot after slot, the five pixel launches of TrivialAugmentWide on
    the slot's slices of the draws.  On host arrays it is the host twins of
    those launches.

    Parameters
    ----------
    num_ops : int
        Operations per image, in [1, 8].
    magnitude : int
        The strength bin of every operation, in [0, num_magnitude_bins - 1].
    num_magnitude_bins : int
        The number of strength bins, in [2, 256].
    interpolation : str
        'nearest' or 'bilinear', for the geometric operations.
    fill : int or Tuple[int, int, int]
        The colour outside the source image, for the geometric operations.
    """
    op_id = 23

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31, interpolation='nearest', fill=(0, 0, 0)):
        super().__init__()
        name = 'RandAugment'

        def is_int(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)
        if not is_int(num_ops) or not 1 <= num_ops <= MAX_NUM_OPS:
            raise ValueError(f'{name}: num_ops must be an int in [1, {MAX_NUM_OPS}], got {num_ops!r}')
        if not is_int(num_magnitude_bins) or not 2 <= num_magnitude_bins <= 256:
            raise ValueError(f'{name}: num_magnitude_bins must be an int in [2, 256], got {num_magnitude_bins!r}')
        if not is_int(magnitude) or not 0 <= magnitude <= num_magnitude_bins - 1:
            raise ValueError(f'{name}: magnitude must be an int in [0, {int(num_magnitude_bins) - 1}], '
                             f'got {magnitude!r}')
        if not isinstance(interpolation, str) or interpolation not in _MODES:
            raise ValueError(f"{name}: interpolation must be 'bilinear' or 'nearest', got {interpolation!r}")
        try:
            f = np.asarray(fill)
            ok = f.dtype.kind in 'iuf' and f.size in (1, 3) and np.isfinite(f).all()
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'{name}: fill must be a number or an RGB triple, got {fill!r}')
        self.num_ops = int(num_ops)
        self.magnitude = int(magnitude)
        self.num_magnitude_bins = int(num_magnitude_bins)
        self.interpolation = interpolation
        self.fill = f
        self.table = None          # built in declare_state_and_memory, where the shape is known
        self._tables = {}
        self._dev_tables = {}

    def table_for(self, H, W):
        """The value table of H x W images, built once per shape."""
        t = self._tables.get((H, W))
        if t is None:
            t = self._tables[(H, W)] = randaugment_table(self.num_magnitude_bins, H, W)
        return t

    def device_table(self, H, W, device):
        t = self._dev_tables.get((H, W, device))
        if t is None:
            t = self._dev_tables[(H, W, device)] = ch.from_numpy(self.table_for(H, W)).to(device)
        return t

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        S, nbins, mag = self.num_ops, self.num_magnitude_bins, self.magnitude
        mode, fill = _MODES[self.interpolation], fill_u8(self.fill)
        key = ('rand_augment', id(self))

        def device(ctx, images, out):
            B, H, W = (int(x) for x in images.shape[:3])
            d = {}
            for name, dt, shape in L.randaugment_arrays(S):
                shp = shape(B)
                n = int(np.prod(shp))
                d[name] = ctx.device_buffer(key + (name,), int(np.prod(shape(ctx.batch_size))),
                                            getattr(ch, np.dtype(dt).name))[:n].view(shp)
            L.randaugment_draw_batch(ctx.batch_ids, ctx.loader_seed, ctx.epoch, S, nbins, mag,
                                     self.device_table(H, W, images.device), H, W, d, None, ctx.stream)
            if 6 * H * W <= L.randaugment_lds_bytes():
                L.randaugment_batch(images, out, S, mode, fill, d, ctx.stream)
                return
            # rounds: slot after slot the launches of TrivialAugmentWide, from the current buffer into the next
            cj_ws = tone_ws = None
            if H * W * 3 > L.color_jitter_lds_bytes():
                cj_ws = ctx.device_buffer(key + ('cj_ws',), ctx.batch_size, ch.int64)[:B]
            if H * W * 3 > L.tone_lds_bytes():
                tone_ws = ctx.device_buffer(key + ('tone_ws',), 768 * ctx.batch_size, ch.int32)[:768 * B]
            cur = images
            for s in range(S):
                nxt = out if s == S - 1 else ctx.device_buffer(
                    key + ('round', s % 2), ctx.batch_size * H * W * 3, ch.uint8)[:B * H * W * 3].view(images.shape)
                a = L.randaugment_slot(d, s)
                L.color_jitter_batch(cur, _CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3], cj_ws, ctx.stream)
                L.color_jitter_batch(cur, _SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:], None, ctx.stream)
                L.tone_batch_bits(cur, _TONE_STEPS, a['tone_apply'], a['tone_bits'], tone_ws, ctx.stream)
                L.affine_batch(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'], 0, ctx.stream)
                L.sharpness_batch(cur, nxt, a['sharp_apply'], a['sharp_factor'], 0, ctx.stream)
                cur = nxt

        def host(seed, epoch, ids, src, out_np, nthreads):
            H, W = src.shape[1:3]
            d = L.randaugment_draw_batch_host(ids, seed, epoch, S, nbins, mag, self.table_for(H, W), H, W)
            cur, spare = src, [None, None]
            for s in range(S):
                if s == S - 1:
                    nxt = out_np
                else:
                    if spare[s % 2] is None:
                        spare[s % 2] = np.empty_like(src)
                    nxt = spare[s % 2]
                a = L.randaugment_slot(d, s)
                L.color_jitter_batch_host(cur, _CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
                L.color_jitter_batch_host(cur, _SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
                L.tone_batch_bits_host(cur, _TONE_STEPS, a['tone_apply'], a['tone_bits'])
                L.affine_batch_host(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'], nthreads=nthreads)
                L.sharpness_batch_host(cur, nxt, a['sharp_apply'], a['sharp_factor'], nthreads=nthreads)
                cur = nxt[:len(src)]
        return self.out_of_place_code(device, host)

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, Optional[AllocationQuery]]:
        _, shape = self.check_u8_images(previous_state)
        if max(shape[0], shape[1]) > 32767:
            raise TypeError(f'RandAugment: images of {shape[0]}x{shape[1]} exceed the supported 32767 per side')
        self.table = self.table_for(int(shape[0]), int(shape[1]))
        return self.declare_out_of_place(previous_state)
