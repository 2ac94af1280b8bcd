"""The parameter structures of the fused epilogue (pipeline/epilogue.py): the
exact RRCParams, DrawParams and SimpleAugParams fields that the crop decoders,
the RandomResizedCrop transform, the fused SimpleRGBImageDecoder path and the
standalone Cutout / RandomHorizontalFlip draws hand to the library, across a
table of configurations.  ctypes structures only: no library, no GPU.

The expected values are those of the five hand-written builders that the
shared object replaced.
"""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.fields.rgb_image import (CenterCropRGBImageDecoder, RandomResizedCropRGBImageDecoder,
                                       SimpleRGBImageDecoder)
from ffcv_amd.libffcv import fill_u8
from ffcv_amd.pipeline.epilogue import Epilogue
from ffcv_amd.transforms import Cutout, NormalizeImage, RandomHorizontalFlip, RandomResizedCrop, RandomTranslate

EPOCH, OUT_H, OUT_W = 3, 24, 24

# name: (Cutout arguments or None, flip_prob or None, cutout_before_flip, normalize, seed,
#        expected RRCParams (cutout_size, cutout_fill[0:4]),
#        expected DrawParams (cutout_size, flip_prob, loader_seed))
CASES = {
    'nothing':            (None, None, False, False, 0, (0, [0, 0, 0, 0]), (0, 0.0, 0)),
    'scalar fill':        ((8, 7), None, True, False, 11, (8, [7, 7, 7, 1]), (8, 0.0, 11)),
    'one-element fill':   ((8, [200]), None, True, False, 11, (8, [200, 200, 200, 1]), (8, 0.0, 11)),
    'triple fill':        ((32, (124, 116, 103)), None, True, False, 0, (32, [124, 116, 103, 1]), (32, 0.0, 0)),
    'with normalize':     ((32, (124, 116, 103)), None, True, True, 0, (32, [124, 116, 103, 1]), (32, 0.0, 0)),
    'cutout before flip': ((16, (1, 2, 3)), 0.5, True, True, 7, (16, [1, 2, 3, 1]), (16, 0.5, 7)),
    'cutout after flip':  ((16, (1, 2, 3)), 0.5, False, False, 7, (16, [1, 2, 3, 0]), (16, 0.5, 7)),
    'flip only':          (None, 0.25, False, False, 5, (0, [0, 0, 0, 0]), (0, 0.25, 5)),
    'normalize only':     (None, None, False, True, 5, (0, [0, 0, 0, 0]), (0, 0.0, 5)),
    'seed -1':            ((4, 9), 1.0, True, False, -1, (4, [9, 9, 9, 1]), (4, 1.0, 2 ** 64 - 1)),
    'seed 2**64 + 5':     ((4, 9), 1.0, False, True, 2 ** 64 + 5, (4, [9, 9, 9, 0]), (4, 1.0, 5)),
}
NORMALIZE = NormalizeImage(np.array([120., 110., 100.]), np.array([60., 61., 62.]), np.float16)


def _fused(name):
    cut, prob, before, norm, seed, want_rp, want_dp = CASES[name]
    kw = dict(cutout=Cutout(*cut) if cut else None, flip=RandomHorizontalFlip(prob) if prob is not None else None,
              cutout_before_flip=before, normalize=NORMALIZE if norm else None)
    return kw, seed, want_rp, want_dp


def _rrc_fields(rp):
    return (rp.cutout_size, list(rp.cutout_fill)), (rp.out_h, rp.out_w, rp.lut, rp.out_stride)


def _draw_fields(dp):
    return (dp.cutout_size, dp.flip_prob, dp.loader_seed), (dp.out_h, dp.out_w, dp.epoch)


def _crop_fields(dp):
    return dp.crop_kind, list(dp.scale), list(dp.ratio), dp.center_ratio


# what each consumer hands to the library -----------------------------------
def rrc_params(op):
    return op._epilogue.fill_rrc_params(L.RRCParams())


def decoder_draw_params(dec, seed, epoch, out_h, out_w):
    return dec._draw_params(seed, epoch, out_h, out_w)


def transform_draw_params(rrc, seed, epoch):
    return rrc._epilogue.draw_params(seed, epoch, rrc.size, rrc.size)


def simple_params(dec, seed, epoch, height, width):
    return dec._aug_params()[0], dec._epilogue.draw_params(seed, epoch, height, width)


def cutout_draw_params(op, seed, epoch, height, width):
    return Epilogue(cutout=op).draw_params(seed, epoch, height, width)


def flip_draw_params(op, seed, epoch):
    return Epilogue(flip=op).draw_params(seed, epoch, 0, 0)


# ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_epilogue_object(name):
    kw, seed, want_rp, want_dp = _fused(name)
    ep = Epilogue(**kw)
    assert bool(ep) == any(kw[k] is not None for k in ('cutout', 'flip', 'normalize'))
    assert ep.output_dtype(ch.uint8) == (ch.float16 if kw['normalize'] is not None else ch.uint8)
    assert ep.output_dtype(np.dtype('u1')) == (ch.float16 if kw['normalize'] is not None else np.dtype('u1'))
    rp = L.RRCParams()
    assert ep.fill_rrc_params(rp) is rp
    assert _rrc_fields(rp) == (want_rp, (0, 0, None, 0))
    dp = ep.draw_params(seed, EPOCH, OUT_H, OUT_W)
    assert _draw_fields(dp) == (want_dp, (OUT_H, OUT_W, EPOCH))
    assert _crop_fields(dp) == (0, [0.0, 0.0], [0.0, 0.0], 0.0)
    # built once per (seed, epoch, size)
    assert ep.draw_params(seed, EPOCH, OUT_H, OUT_W) is dp
    other = ep.draw_params(seed, EPOCH + 1, OUT_H, OUT_W)
    assert other is not dp and _draw_fields(other) == (want_dp, (OUT_H, OUT_W, EPOCH + 1))
    assert _draw_fields(ep.draw_params(seed, EPOCH, 32, 40))[1] == (32, 40, EPOCH)


@pytest.mark.parametrize('name', sorted(CASES))
def test_decoders_and_transform_agree(name):
    kw, seed, want_rp, want_dp = _fused(name)
    dec = RandomResizedCropRGBImageDecoder((OUT_H, OUT_W), scale=(0.25, 1.0), ratio=(0.5, 2.0))
    cen = CenterCropRGBImageDecoder((OUT_H, OUT_W), 0.875)
    rrc = RandomResizedCrop((0.08, 1.0), (0.75, 4 / 3), OUT_H)
    for op in (dec, cen, rrc):
        assert op._fused_cutout is None and op._fused_flip is None and op._fused_normalize is None
        assert not op._cutout_before_flip and not op.fused
        op.fuse(**kw)
        assert (op._fused_cutout, op._fused_flip, op._cutout_before_flip, op._fused_normalize) == \
            (kw['cutout'], kw['flip'], kw['cutout_before_flip'], kw['normalize'])
    assert dec.output_dtype == cen.output_dtype == (ch.float16 if kw['normalize'] is not None else ch.uint8)
    assert rrc.fused == any(kw[k] is not None for k in ('cutout', 'flip', 'normalize'))
    assert not dec.fused and dec._fused_steps == ()      # the crop decoders have no step list

    rps = [rrc_params(op) for op in (dec, cen, rrc)]
    assert all(_rrc_fields(rp)[0] == want_rp for rp in rps)
    for rp in rps:    # the decoders set the size per batch, the transform once
        rp.out_h, rp.out_w = OUT_H, OUT_W
    assert bytes(rps[0]) == bytes(rps[1]) == bytes(rps[2])

    dps = [decoder_draw_params(dec, seed, EPOCH, OUT_H, OUT_W), decoder_draw_params(cen, seed, EPOCH, OUT_H, OUT_W),
           transform_draw_params(rrc, seed, EPOCH)]
    assert all(_draw_fields(dp) == (want_dp, (OUT_H, OUT_W, EPOCH)) for dp in dps)
    assert _crop_fields(dps[0]) == (0, [0.25, 1.0], [0.5, 2.0], 0.0)
    assert _crop_fields(dps[1]) == (1, [0.0, 0.0], [0.0, 0.0], 0.875)
    assert _crop_fields(dps[2]) == (0, [0.0, 0.0], [0.0, 0.0], 0.0)   # its crop has a draw launch of its own


@pytest.mark.parametrize('order', ['tfc', 'cft', 'ftc', 't', 'tc', 'ft'])
@pytest.mark.parametrize('seed,seed64', [(0, 0), (-1, 2 ** 64 - 1), (2 ** 64 + 5, 5)])
def test_simple_decoder_params(order, seed, seed64):
    ops = {'t': RandomTranslate(3, (9, 8, 7)), 'f': RandomHorizontalFlip(0.75), 'c': Cutout(6, 250)}
    code = {'f': L.AUG_FLIP, 't': L.AUG_TRANSLATE, 'c': L.AUG_CUTOUT}
    dec = SimpleRGBImageDecoder()
    assert not dec.fused and dec._fused_steps == () and dec._fused_normalize is None and dec.output_dtype == ch.uint8
    dec.fuse(steps=[ops[k] for k in order], normalize=NORMALIZE)
    assert dec.fused and list(dec._fused_steps) == [ops[k] for k in order]
    assert dec._fused_normalize is NORMALIZE and dec.output_dtype == ch.float16
    ap, dp = simple_params(dec, seed, EPOCH, 32, 40)
    assert ap.n_steps == len(order)
    assert list(ap.steps) == [code[k] for k in order] + [0] * (4 - len(order))
    assert (ap.padding, list(ap.translate_fill)) == (3, [9, 8, 7, 0])
    assert (ap.cutout_size, list(ap.cutout_fill)) == ((6, [250, 250, 250, 0]) if 'c' in order else (0, [0] * 4))
    assert _draw_fields(dp) == ((6 if 'c' in order else 0, 0.75 if 'f' in order else 0.0, seed64), (32, 40, EPOCH))
    assert _crop_fields(dp) == (0, [0.0, 0.0], [0.0, 0.0], 0.0)
    dec.fuse(steps=[], normalize=NORMALIZE)      # a table without steps is not fused
    assert not dec.fused and dec._fused_normalize is None and dec.output_dtype == ch.uint8


@pytest.mark.parametrize('seed,seed64', [(12, 12), (-1, 2 ** 64 - 1), (2 ** 64 + 5, 5)])
def test_standalone_draw_params(seed, seed64):
    dp = cutout_draw_params(Cutout(8, (1, 2, 3)), seed, EPOCH, 32, 40)
    assert _draw_fields(dp) == ((8, 0.0, seed64), (32, 40, EPOCH))
    assert _crop_fields(dp) == (0, [0.0, 0.0], [0.0, 0.0], 0.0)
    dp = flip_draw_params(RandomHorizontalFlip(0.3), seed, EPOCH)
    assert _draw_fields(dp) == ((0, 0.3, seed64), (0, 0, EPOCH))
    assert _crop_fields(dp) == (0, [0.0, 0.0], [0.0, 0.0], 0.0)


def test_fill_u8():
    for fill, want in ((7, [7, 7, 7]), (np.array(7), [7, 7, 7]), ([200], [200] * 3), (np.array([200]), [200] * 3),
                       ((1, 2, 3), [1, 2, 3]), (np.array([1, 2, 3]), [1, 2, 3]), (np.array(300), [44] * 3)):
        got = fill_u8(fill)
        assert got.dtype == np.uint8 and got.shape == (3,) and got.tolist() == want
        assert got.flags.writeable and got.flags.c_contiguous and got is not fill_u8(fill)
    for bad in ((1, 2), np.arange(4), ()):
        with pytest.raises(ValueError):
            fill_u8(bad)
    with pytest.raises(ValueError):
        Epilogue(cutout=Cutout(4, (1, 2))).fill_rrc_params(L.RRCParams())
