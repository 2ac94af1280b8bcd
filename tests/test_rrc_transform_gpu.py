"""The RandomResizedCrop transform on the MI355X, bit for bit against the
oracle (tests/rrc_transform_ref.py): ffcv_rrc_images_batch in both regimes
(one workgroup per image in LDS; the band kernel behind the descriptor
kernel) on forced crops of every resize kind, unaligned inputs inside a
guarded allocation, strided outputs, u8 and fp16 with flip and cutout in both
orders; crop validation on the device; the device draws against the host
draws; and Loaders whose chains are lowered into the transform's launch, left
alone, grouped, staged over PCIe and fed by the JPEG decoder."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd.loader import Loader, OrderOption
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomHorizontalFlip,
                                 RandomTranslate, RandomBrightness, RandomResizedCrop, Poison)
from tests.helpers import NaturalDS, write
from tests import color_jitter_ref as CJ
from tests.poison_ref import poison_np
from tests.translate_ref import apply_steps, cutout_draw, flip_draw, translate_draw, translate_np
from tests.rrc_transform_ref import (DEFAULT_RATIO, DEFAULT_SCALE, SAMPLE_OK, SAMPLE_RANGE, crop_draw,
                                     every_size_crops, expected_epilogue, expected_resize, expected_transform,
                                     forced_crops, invalid_crops, kinds)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)  # normalize.py:42-49
FILL = (200, 201, 202)
GUARD = 4096
OUTS = [(32, 32), (30, 30), (33, 33), (24, 40)]


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


@pytest.fixture(scope='module')
def lut_dev():
    return ch.from_numpy(LUT.view(np.int16)).to(DEV)


def past_limit():
    """The smallest square source whose H * W * 3 exceeds the LDS limit."""
    from ffcv_amd import libffcv as L
    s = 1
    while s * s * 3 <= L.rrc_images_lds_bytes():
        s += 1
    return s


def guarded(imgs):
    """The batch as a device view at byte offset 1 of an allocation with
    GUARD bytes of 0xEE on both sides: (view, whole allocation)."""
    flat = np.ascontiguousarray(imgs).reshape(-1)
    host = np.full(GUARD + 1 + flat.size + GUARD, 0xEE, np.uint8)
    host[GUARD + 1:GUARD + 1 + flat.size] = flat
    whole = ch.from_numpy(host).to(DEV)
    view = whole[GUARD + 1:GUARD + 1 + flat.size]
    assert view.data_ptr() % 16 == 1
    return view, whole


def run_images(L, view, B, H, W, crops, oh, ow, lut=None, flips=None, cyx=None, cut=0, cut_before_flip=False,
               pad=4):
    """One ffcv_rrc_images_batch call into a pre-filled, strided output:
    (images, status, bytes between the images)."""
    p = L.RRCParams()
    p.out_h, p.out_w = oh, ow
    es = 2 if lut is not None else 1
    dense = oh * ow * 3 * es
    stride = dense + pad
    p.out_stride = stride
    if cut:
        p.cutout_size = cut
        for c in range(3):
            p.cutout_fill[c] = FILL[c]
        p.cutout_fill[3] = int(cut_before_flip)
    if lut is not None:
        p.lut = lut.data_ptr()
    out = ch.full((B * stride,), 0xAB, dtype=ch.uint8, device=DEV)
    status = ch.full((B,), -1, dtype=ch.int32, device=DEV)
    d_crops = ch.from_numpy(np.ascontiguousarray(crops, np.int32)).to(DEV)
    d_flips = ch.from_numpy(np.ascontiguousarray(flips, np.uint8)).to(DEV) if flips is not None else None
    d_cyx = ch.from_numpy(np.ascontiguousarray(cyx, np.int32)).to(DEV) if cyx is not None else None
    nws = L.rrc_images_workspace_bytes(B, H, W, oh, ow)
    ws = ch.empty(nws, dtype=ch.uint8, device=DEV) if nws else None
    L.rrc_images_batch(view, H * W * 3, B, H, W, d_crops, d_cyx, d_flips, p, out, status, ws)
    got = out.cpu().numpy().reshape(B, stride)
    imgs = got[:, :dense].copy()
    imgs = imgs.view(np.uint16).reshape(B, oh, ow, 3) if lut is not None else imgs.reshape(B, oh, ow, 3)
    return imgs, status.cpu().numpy(), got[:, dense:], nws


SOURCES = [(32, 32), (33, 35), (64, 64), (40, 56), 'past']


@pytest.mark.parametrize('B', [1, 70])
@pytest.mark.parametrize('src', SOURCES, ids=[str(s) for s in SOURCES])
def test_abi_both_regimes(hip_lib, oracle, lut_dev, src, B):
    from ffcv_amd import libffcv as L
    H, W = (past_limit(),) * 2 if src == 'past' else src
    lds = src != 'past'
    rng = np.random.default_rng(H * 131 + W + B)
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    imgs[::7] = np.where(imgs[::7] > 127, 255, 0)              # saturated extremes now and then
    crops = forced_crops(H, W, 70, seed=H + W)[:B] if B > 1 else forced_crops(H, W, 70, seed=H + W)[-1:]
    if B > 1 and min(H, W) >= 64:
        assert kinds(crops, 32, 32) == {0, 1, 2, 3}
    view, whole = guarded(imgs)
    flips = rng.integers(0, 2, B).astype(np.uint8)
    for oh, ow in OUTS:
        want, _ = expected_resize(oracle, imgs, crops, oh, ow)
        got, st, gaps, nws = run_images(L, view, B, H, W, crops, oh, ow)
        assert (nws == 0) == lds, (H, W, nws)
        assert np.array_equal(got, want), (H, W, oh, ow, np.argwhere((got != want).any(axis=(1, 2, 3)))[:5])
        assert (st == SAMPLE_OK).all() and (gaps == 0xAB).all()
        # an output stride that leaves every second image misaligned: the narrow stores
        got, st, gaps, _ = run_images(L, view, B, H, W, crops, oh, ow, pad=1)
        assert np.array_equal(got, want) and (gaps == 0xAB).all()
        cut = 5
        cyx = np.stack([rng.integers(0, oh - cut + 1, B), rng.integers(0, ow - cut + 1, B)], 1).astype(np.int32)
        for cbf in (False, True):
            w16 = expected_epilogue(want, flips, cyx, cut, FILL, cbf, LUT).view(np.uint16)
            got, st, gaps, _ = run_images(L, view, B, H, W, crops, oh, ow, lut_dev, flips, cyx, cut, cbf, pad=8)
            assert np.array_equal(got, w16), (H, W, oh, ow, cbf)
            assert (st == SAMPLE_OK).all() and (gaps == 0xAB).all()
        # u8 with the epilogue, flip only, and an fp16 stride that is no multiple of 8
        w8 = expected_epilogue(want, flips, cyx, cut, FILL, True)
        got, _, _, _ = run_images(L, view, B, H, W, crops, oh, ow, None, flips, cyx, cut, True)
        assert np.array_equal(got, w8)
        w16 = expected_epilogue(want, flips, lut=LUT).view(np.uint16)
        got, _, gaps, _ = run_images(L, view, B, H, W, crops, oh, ow, lut_dev, flips, pad=2)
        assert np.array_equal(got, w16) and (gaps == 0xAB).all()
    assert (whole[:GUARD + 1] == 0xEE).all() and (whole[-GUARD:] == 0xEE).all()


def test_cutout_across_quads_in_the_lds_regime(hip_lib, oracle, lut_dev):
    """The raw dispatch test's cutout group through the image kernel: 52 x 44
    images (staged source 52 * ((3 * 44 + 30) >> 4) * 16 + 16 = 8,336 bytes: the
    LDS regime), out 20 x 16, crops 10 x 9 (linear walk), 30 x 24 (area, scales
    1.5) and 50 x 40 (area, scales 2.5), a cutout of 5 at (y 13, x 6) that cuts
    through the quads of columns 4..7 and 8..11, flip 0 and 1, cut before and
    after the flip, u8 and fp16 with the group stores (aligned strides)."""
    from ffcv_amd import libffcv as L
    H, W, oh, ow, cut = 52, 44, 20, 16, 5
    crops = np.array([c for c in ((1, 2, 10, 9), (3, 4, 30, 24), (1, 2, 50, 40)) for _ in (0, 1)], np.int32)
    B = len(crops)
    assert kinds(crops, oh, ow) == {2, 3}
    flips = np.array([0, 1] * 3, np.uint8)
    cyx = np.tile(np.array([[13, 6]], np.int32), (B, 1))
    imgs = np.random.default_rng(11).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    view, whole = guarded(imgs)
    want, _ = expected_resize(oracle, imgs, crops, oh, ow)
    for cbf in (False, True):
        w8 = expected_epilogue(want, flips, cyx, cut, FILL, cbf)
        got, st, gaps, nws = run_images(L, view, B, H, W, crops, oh, ow, None, flips, cyx, cut, cbf, pad=4)
        assert nws == 0, nws
        assert np.array_equal(got, w8), (cbf, np.argwhere((got != w8).any(axis=(1, 2, 3))).ravel())
        assert (st == SAMPLE_OK).all() and (gaps == 0xAB).all()
        w16 = expected_epilogue(want, flips, cyx, cut, FILL, cbf, LUT).view(np.uint16)
        got, st, gaps, _ = run_images(L, view, B, H, W, crops, oh, ow, lut_dev, flips, cyx, cut, cbf, pad=8)
        assert np.array_equal(got, w16), (cbf, np.argwhere((got != w16).any(axis=(1, 2, 3))).ravel())
        assert (st == SAMPLE_OK).all() and (gaps == 0xAB).all()
    assert (whole[:GUARD + 1] == 0xEE).all() and (whole[-GUARD:] == 0xEE).all()


def test_every_crop_size_of_32(hip_lib, oracle):
    """A window of every size of a 32 x 32 source to 32 x 32 (1,024 images in
    one launch): every linear tap pattern, the copy among them."""
    from ffcv_amd import libffcv as L
    crops = every_size_crops(32, 32)
    imgs = np.random.default_rng(4).integers(0, 256, (len(crops), 32, 32, 3), dtype=np.uint8)
    view, _ = guarded(imgs)
    got, st, _, _ = run_images(L, view, len(crops), 32, 32, crops, 32, 32)
    want, _ = expected_resize(oracle, imgs, crops, 32, 32)
    assert np.array_equal(got, want) and (st == SAMPLE_OK).all()


@pytest.mark.parametrize('src', [(40, 56), 'past'], ids=['lds', 'band'])
def test_invalid_crops(hip_lib, oracle, lut_dev, src):
    """One window of each kind of violation among valid neighbours: zero
    images and FFCV_SAMPLE_RANGE there, everything else exact."""
    from ffcv_amd import libffcv as L
    H, W = (past_limit(),) * 2 if src == 'past' else src
    bad = invalid_crops(H, W)
    good = forced_crops(H, W, len(bad) + 1, seed=2)
    B = 2 * len(bad) + 1
    crops = np.empty((B, 4), np.int32)
    crops[0::2], crops[1::2] = good, bad
    imgs = np.random.default_rng(6).integers(1, 256, (B, H, W, 3), dtype=np.uint8)
    view, whole = guarded(imgs)
    want, wst = expected_resize(oracle, imgs, crops, 32, 32)
    assert (wst[1::2] == SAMPLE_RANGE).all() and (wst[0::2] == SAMPLE_OK).all()
    got, st, gaps, _ = run_images(L, view, B, H, W, crops, 32, 32)
    assert np.array_equal(st, wst) and np.array_equal(got, want) and (gaps == 0xAB).all()
    assert (got[1::2] == 0).all() and all(o.any() for o in got[0::2])
    flips = np.ones(B, np.uint8)
    w16 = expected_epilogue(want, flips, lut=LUT, status=wst).view(np.uint16)
    got, st, gaps, _ = run_images(L, view, B, H, W, crops, 32, 32, lut_dev, flips, pad=8)
    assert np.array_equal(st, wst) and np.array_equal(got, w16) and (gaps == 0xAB).all()
    assert (got[1::2] == 0).all()
    assert (whole[:GUARD + 1] == 0xEE).all() and (whole[-GUARD:] == 0xEE).all()


def test_device_draws_match_host(hip_lib):
    """2,000 ids per case.  A crop takes at most 44 words of its stream, so
    FFCV_SAMPLE_RNG cannot be provoked through this entry point: the status
    array is checked to be written, all FFCV_SAMPLE_OK."""
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(9)
    ids = rng.integers(0, 2 ** 40, 2000).astype(np.int64)
    ids[:8] = np.arange(8)
    d_ids = ch.from_numpy(ids).to(DEV)
    for (H, W), scale, ratio in (((32, 32), DEFAULT_SCALE, DEFAULT_RATIO), ((40, 56), DEFAULT_SCALE, DEFAULT_RATIO),
                                 ((56, 40), (1.5, 2.0), (0.2, 0.3)), ((40, 56), (1.5, 2.0), (2, 3)),
                                 ((64, 64), (0.25, 1), (0.5, 2)), ((32, 32), (1, 1), (1, 1))):
        crops = ch.full((2000, 4), -7, dtype=ch.int32, device=DEV)
        status = ch.full((2000,), -1, dtype=ch.int32, device=DEV)
        L.crop_draw_batch(d_ids, H, W, scale, ratio, 77, 3, crops, status)
        want = L.crop_draw_batch_host(ids.astype(np.uint64), H, W, scale, ratio, 77, 3)
        assert np.array_equal(crops.cpu().numpy(), want), (H, W, scale, ratio)
        assert (status.cpu().numpy() == SAMPLE_OK).all()
    L.crop_draw_batch(d_ids[:3], 32, 32, DEFAULT_SCALE, DEFAULT_RATIO, 77, 3, crops, None)   # status is optional


def test_abi_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = hip_lib
    S = past_limit()
    img = ch.full((2, 8, 8, 3), 77, dtype=ch.uint8, device=DEV)
    big = ch.full((2, S, S, 3), 77, dtype=ch.uint8, device=DEV)
    out = ch.full((2, 4, 4, 3), 55, dtype=ch.uint8, device=DEV)
    crops = ch.tensor([[0, 0, 8, 8]] * 2, dtype=ch.int32, device=DEV)
    cyx = ch.zeros((2, 2), dtype=ch.int32, device=DEV)
    ws = ch.empty(L.rrc_images_workspace_bytes(2, S, S, 4, 4) + 16, dtype=ch.uint8, device=DEV)
    assert L.rrc_images_workspace_bytes(2, 8, 8, 4, 4) == 0 and ws.numel() > 16
    p = L.RRCParams()
    p.out_h = p.out_w = 4
    ch.cuda.synchronize()
    good = dict(inp=img.data_ptr(), in_stride=192, batch=2, height=8, width=8, crops=crops.data_ptr(), cut=None,
                p=ctypes.byref(p), out=out.data_ptr(), ws=None, ws_bytes=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ffcv_rrc_images_batch(None, a['inp'], a['in_stride'], a['batch'], a['height'], a['width'],
                                         a['crops'], a['cut'], None, a['p'], a['out'], None, a['ws'], a['ws_bytes'])
    bigger = L.RRCParams()
    bigger.out_h = bigger.out_w = 4
    bigger.cutout_size = 5
    zero = L.RRCParams()
    zero.out_h, zero.out_w = 0, 4
    for kw in (dict(inp=None), dict(crops=None), dict(p=None), dict(out=None), dict(batch=-1), dict(height=0),
               dict(width=-1), dict(in_stride=191), dict(out=img.data_ptr() + 96), dict(p=ctypes.byref(zero)),
               dict(p=ctypes.byref(bigger), cut=cyx.data_ptr()),
               dict(inp=big.data_ptr(), in_stride=S * S * 3, height=S, width=S),                       # no workspace
               dict(inp=big.data_ptr(), in_stride=S * S * 3, height=S, width=S, ws=ws.data_ptr(), ws_bytes=64),
               dict(inp=big.data_ptr(), in_stride=S * S * 3, height=S, width=S, ws=ws.data_ptr() + 4,
                    ws_bytes=ws.numel() - 16)):
        assert call(**kw) == -1, kw
        assert b'ffcv_rrc_images_batch' in lib.ffcv_last_error()
    assert call(batch=0) == 0
    ch.cuda.synchronize()
    assert (out == 55).all()                                   # nothing was launched
    ids = ch.arange(4, dtype=ch.int64, device=DEV)
    cr = ch.full((4, 4), -7, dtype=ch.int32, device=DEV)
    two = ctypes.c_double * 2
    for args in ((None, 4, 8, 8, two(0.08, 1), two(0.75, 1.33), cr.data_ptr()),
                 (ids.data_ptr(), -1, 8, 8, two(0.08, 1), two(0.75, 1.33), cr.data_ptr()),
                 (ids.data_ptr(), 4, 0, 8, two(0.08, 1), two(0.75, 1.33), cr.data_ptr()),
                 (ids.data_ptr(), 4, 8, 8, None, two(0.75, 1.33), cr.data_ptr()),
                 (ids.data_ptr(), 4, 8, 8, two(0.08, 1), two(0, 1), cr.data_ptr()),
                 (ids.data_ptr(), 4, 8, 8, two(0.08, 1), two(0.75, 1.33), None)):
        i, b, h, w, s, r, c = args
        assert lib.ffcv_crop_draw_batch(None, i, b, h, w, s, r, 0, 0, c, None) == -1, args
        assert b'ffcv_crop_draw_batch' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert (cr == -7).all()
    assert call() == 0
    ch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all()


# ------------------------------------------------------------------ Loader --
def _raw_beton(tmpdir_m, hw, n=70, seed=3):
    fn = os.path.join(tmpdir_m, f'raw_{hw[0]}x{hw[1]}.beton')
    ds = NaturalDS(n, hw=hw, seed=seed)
    if not os.path.exists(fn):
        write(fn, ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn, ds


def _tail():
    return [ToTensor(), ToDevice(DEV), ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)]


def _loader(fn, ops, seed, batch_size=16, **kw):
    return Loader(fn, batch_size=batch_size, seed=seed, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder()] + ops, 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)


def _lut16(u8):
    return np.stack([LUT[u8[..., c], c] for c in range(3)], -1).view(np.uint16)


@pytest.mark.parametrize('hw', [(32, 32), (64, 64)])
def test_loader_chain_lowered_into_one_launch(tmpdir_m, oracle, hw):
    fn, ds = _raw_beton(tmpdir_m, hw)
    seed = 21
    rrc = RandomResizedCrop(DEFAULT_SCALE, DEFAULT_RATIO, 32)
    ops = [rrc, RandomHorizontalFlip(0.5), Cutout(6, FILL)] + _tail()
    loader = _loader(fn, ops, seed)
    assert rrc._fused_flip is ops[1] and rrc._fused_cutout is ops[2] and rrc._fused_normalize is ops[-1]
    for epoch in range(2):
        n = flips = 0
        for b, (images, labels) in enumerate(loader):
            assert images.dtype == ch.float16 and tuple(images.shape[1:]) == (3, 32, 32)
            assert images.is_contiguous(memory_format=ch.channels_last)
            got = images.permute(0, 2, 3, 1).cpu().numpy().view(np.uint16)
            for k in range(got.shape[0]):
                sid = b * 16 + k
                u8 = expected_transform(oracle, ds.imgs[sid], seed, epoch, sid, 32, chain='fc', cut=6, fill=FILL)
                assert np.array_equal(got[k], _lut16(u8)), (epoch, sid)
                assert int(labels[k]) == sid % 10
                flips += flip_draw(seed, epoch, sid, 0.5)
                n += 1
        assert n == 70 and 0 < flips < 70


def test_loader_operation_in_between_nothing_absorbed(tmpdir_m, oracle):
    fn, ds = _raw_beton(tmpdir_m, (32, 32))
    seed = 5
    rrc = RandomResizedCrop((0.25, 1), DEFAULT_RATIO, 24)
    ops = [rrc, RandomBrightness(0.4, 0.7), RandomHorizontalFlip(0.5), Cutout(6, FILL)] + _tail()
    loader = _loader(fn, ops, seed)
    assert not rrc.fused and not any(getattr(o, '_absorbed', False) for o in ops[1:])
    n = 0
    for b, (images, labels) in enumerate(loader):
        got = images.permute(0, 2, 3, 1).cpu().numpy().view(np.uint16)
        for k in range(got.shape[0]):
            sid = b * 16 + k
            u8 = expected_transform(oracle, ds.imgs[sid], seed, 0, sid, 24, (0.25, 1), DEFAULT_RATIO)
            apply, ratio = CJ.jitter_draw(seed, 0, sid, CJ.BRIGHTNESS, 0.7, 0.4)
            if apply:
                u8 = CJ.jitter_np(u8, CJ.BRIGHTNESS, ratio)
            u8 = apply_steps(u8, 'fc', flip_draw(seed, 0, sid, 0.5), None, cutout_draw(seed, 0, sid, 24, 24, 6),
                             cut=6, cfill=FILL)
            assert np.array_equal(got[k], _lut16(u8)), sid
            n += 1
    assert n == 70


def test_loader_translate_and_poison_in_front(tmpdir_m, oracle):
    fn, ds = _raw_beton(tmpdir_m, (32, 32))
    seed = 8
    rng = np.random.default_rng(1)
    mask = rng.integers(0, 256, (32, 32, 3)).astype(np.uint8)
    alpha = rng.random((32, 32)).astype(np.float32)
    poisoned = list(range(0, 70, 3))
    rrc = RandomResizedCrop(DEFAULT_SCALE, DEFAULT_RATIO, 32)
    ops = [RandomTranslate(2, (9, 8, 7)), Poison(mask, alpha, poisoned), rrc, RandomHorizontalFlip(0.5),
           ToTensor(), ToDevice(DEV)]
    loader = _loader(fn, ops, seed)
    assert loader.pipeline_specs['image'].decoder.fused and rrc._fused_flip is ops[3]
    n = 0
    for b, (images, labels) in enumerate(loader):
        got = images.cpu().numpy()
        assert got.dtype == np.uint8 and got.shape[1:] == (32, 32, 3)
        for k in range(got.shape[0]):
            sid = b * 16 + k
            y, x = translate_draw(seed, 0, sid, 2)
            img = translate_np(ds.imgs[sid], y, x, 2, (9, 8, 7))
            img = poison_np(img[None], mask, alpha, [sid], poisoned)[0]
            want = expected_transform(oracle, img, seed, 0, sid, 32, chain='f')
            assert np.array_equal(got[k], want), sid
            n += 1
    assert n == 70


def test_loader_groups_and_pcie_match(tmpdir_m):
    """Launch groups hand out the batches of one launch per batch; the PCIe
    path (device_cache=False) equals the device cache."""
    fn, ds = _raw_beton(tmpdir_m, (64, 64))

    def mk(**kw):
        return Loader(fn, batch_size=16, order=OrderOption.RANDOM, seed=7, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomResizedCrop(DEFAULT_SCALE, DEFAULT_RATIO, 32),
                      RandomHorizontalFlip(0.5), Cutout(6, FILL)] + _tail(),
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    a, b, c, d = mk(batches_per_launch=1), mk(), mk(batches_per_launch=3), mk(device_cache=False)
    assert d.device_dataset.data is None
    for epoch in range(2):
        n = 0
        for (ia, la), (ib, lb), (ic, lc), (id_, ld) in zip(a, b, c, d):
            assert ch.equal(la, lb) and ch.equal(la, lc) and ch.equal(la, ld)
            for other in (ib, ic, id_):
                assert ch.equal(ia.view(ch.int16), other.view(ch.int16))
            n += len(la)
        assert n == 70


def test_loader_jpeg_fixed_size_dataset(tmpdir_m, oracle):
    """JPEG samples of one size: the transform crops what SimpleRGBImageDecoder
    decoded (a second Loader's output)."""
    fn = os.path.join(tmpdir_m, 'jpg_40x56.beton')
    write(fn, NaturalDS(20, hw=(40, 56), seed=9), {'image': RGBImageField(write_mode='jpg'), 'label': IntField()})
    seed = 6
    plain = _loader(fn, [ToTensor(), ToDevice(DEV)], seed, batch_size=8)
    loader = _loader(fn, [RandomResizedCrop(DEFAULT_SCALE, DEFAULT_RATIO, 24), ToTensor(), ToDevice(DEV)], seed,
                     batch_size=8)
    n = 0
    for b, ((images, _), (decoded, _)) in enumerate(zip(loader, plain)):
        got, dec = images.cpu().numpy(), decoded.cpu().numpy()
        assert got.shape[1:] == (24, 24, 3) and dec.shape[1:] == (40, 56, 3)
        for k in range(got.shape[0]):
            sid = b * 8 + k
            i, j, h, w = crop_draw(oracle, seed, 0, sid, 40, 56)
            assert np.array_equal(got[k], oracle.resize_crop(dec[k], i, i + h, j, j + w, 24, 24)), sid
            n += 1
    assert n == 20
