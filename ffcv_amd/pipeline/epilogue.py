"""The fused epilogue on the Python side: the Cutout, RandomHorizontalFlip and
fp16 NormalizeImage that a crop-and-resize launch applies itself (``Epilogue``
in csrc/device_common.h).  The graph lowering hands them to ``fuse()``; the
launch's parameter structures are filled here, once for every consumer: the
crop decoders, the RandomResizedCrop transform, the fused
SimpleRGBImageDecoder path, and the standalone Cutout / RandomHorizontalFlip
device branches (for their draws).
"""
import torch as ch

from .. import libffcv as L
from ..libffcv import fill_u8


class Epilogue:

    def __init__(self, cutout=None, flip=None, cutout_before_flip=False, normalize=None):
        self.cutout = cutout
        self.flip = flip
        self.cutout_before_flip = cutout_before_flip
        self.normalize = normalize
        self._dp_cache = None

    def __bool__(self):
        return any(x is not None for x in (self.cutout, self.flip, self.normalize))

    def output_dtype(self, default=ch.uint8):
        return ch.float16 if self.normalize is not None else default

    def fill_cutout(self, params):
        """The cutout size and fill bytes of an RRCParams or a SimpleAugParams."""
        if self.cutout is not None:
            params.cutout_size = int(self.cutout.crop_size)
            params.cutout_fill[:3] = fill_u8(self.cutout.fill).tolist()
        return params

    def fill_rrc_params(self, rp):
        """The same, and the order flag (cutout_fill[3]: Cutout runs before the flip)."""
        if self.cutout is not None:
            self.fill_cutout(rp).cutout_fill[3] = int(self.cutout_before_flip)
        return rp

    def draw_params(self, seed, epoch, out_h, out_w, crop=None):
        """The DrawParams of the cutout origin and the flip decision in out_h x
        out_w images; ``crop(p)`` adds a decoder's crop fields.  Built once per
        (seed, epoch, size): per batch this is one tuple comparison."""
        key = (seed, epoch, out_h, out_w)
        cached = self._dp_cache
        if cached is not None and cached[0] == key:
            return cached[1]
        p = L.DrawParams()
        p.out_h, p.out_w = out_h, out_w
        if self.cutout is not None:
            p.cutout_size = int(self.cutout.crop_size)
        if self.flip is not None:
            p.flip_prob = float(self.flip.flip_prob)
        p.loader_seed, p.epoch = L._seed64(seed), int(epoch)
        if crop is not None:
            crop(p)
        self._dp_cache = (key, p)
        return p


class FusesEpilogue:
    """An operation whose launch applies an Epilogue: the graph lowering's
    ``fuse()`` hook and the names it and the tests read."""

    def fuse(self, cutout=None, flip=None, cutout_before_flip=False, normalize=None):
        self._epilogue = Epilogue(cutout, flip, cutout_before_flip, normalize)

    _fused_cutout = property(lambda self: self._epilogue.cutout)
    _fused_flip = property(lambda self: self._epilogue.flip)
    _cutout_before_flip = property(lambda self: self._epilogue.cutout_before_flip)
    _fused_normalize = property(lambda self: self._epilogue.normalize)
