"""RandomAffine / RandomRotation on the MI355X, bit for bit against numpy
(tests/affine_ref.py): ffcv_affine_batch with numpy's integer coefficients in
every regime (a workgroup per image; tiles that stage their footprint; tiles
that read global memory directly; tiles that read nothing) with src and dst at
every byte alignment inside guarded buffers, the device draws against the host
twin under the coefficient guard, and device Loaders against the CPU Loader
under the same seed."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomHorizontalFlip,
                                 RandomAffine)
from tests import affine_ref as R
from tests.helpers import NaturalDS, write
from tests.test_affine import FILL, MODES, SEED, SHAPES, WHOLE, coef_sets
from tests.test_blur import make_inputs, mixed_apply

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# one shape per regime runs all 16 alignments of src: whole image, tiles (staged, direct and empty ones)
ALL_ALIGNMENTS = ((32, 32), (97, 131))


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_warp(imgs, mode, apply, coef, slead=0, dlead=0, fill=FILL):
    """ffcv_affine_batch with imgs `slead` bytes into a device buffer and the
    output `dlead` bytes into a 0xA5-guarded one; returns the output and
    checks the guards and the source."""
    nb = imgs.size
    sbuf = ch.full((slead + nb + 33,), 0x3C, dtype=ch.uint8, device=DEV)
    dbuf = ch.full((dlead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    src = sbuf[slead:slead + nb].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    dst = dbuf[dlead:dlead + nb].view(imgs.shape)
    L.affine_batch(src, dst, mode, fill, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                   ch.from_numpy(np.ascontiguousarray(coef, np.int64)).to(DEV))
    out, back = dbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (out[:dlead] == 0xA5).all() and (out[dlead + nb:] == 0xA5).all()
    assert np.array_equal(back[slead:slead + nb].reshape(imgs.shape), imgs)
    return out[dlead:dlead + nb].reshape(imgs.shape)


def _tile_sizes(H, W, mode, q):
    if 3 * H * W <= WHOLE:
        return [L.affine_tile_bytes(H, W, mode, q, 0, 0)]
    th, tw = L.affine_tile_shape()
    return [L.affine_tile_bytes(H, W, mode, q, r, c) for r in range(-(-H // th)) for c in range(-(-W // tw))]


def test_regime_constants_and_cases():
    assert L.affine_whole_bytes() == WHOLE
    assert 3 * 43 * 127 <= WHOLE < 3 * 43 * 128 and (43, 127) in SHAPES and (43, 128) in SHAPES
    lds = L.affine_tile_lds()
    staged = direct = empty = 0
    for shape in SHAPES:
        if 3 * shape[0] * shape[1] <= WHOLE:
            continue
        for mode in MODES:
            sizes = _tile_sizes(*shape, mode, coef_sets(*shape)['scale_quarter'])
            staged += sum(0 < s <= lds for s in sizes)
            direct += sum(s > lds for s in sizes)
            empty += sum(s == 0 for s in sizes)
    assert staged and direct and empty           # scale 1/4 lands on both sides of the bound


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_kernel_matches_numpy(shape):
    """Batches of 7 images (random, all-0, all-255, checkerboard) with mixed
    apply flags under every coefficient set and both modes: unapplied images
    come out equal to the input."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    imgs = make_inputs(rng, shape)
    apply = mixed_apply()
    sets = coef_sets(*shape)
    wide = shape in ALL_ALIGNMENTS
    for mode in MODES:
        for i, (name, q) in enumerate(sets.items()):
            coef = np.stack([q] * len(imgs))
            want = R.warp_batch(imgs, coef, mode, apply, FILL)
            sweep = wide and name in ('rot33.7_shear', 'scale_quarter')
            for a in (range(16) if sweep else ((5 * i + 3) & 15,)):
                got = _device_warp(imgs, mode, apply, coef, slead=a, dlead=(11 * a + 5) & 15)
                bad = [k for k in range(len(imgs)) if not np.array_equal(got[k], want[k])]
                assert not bad, (shape, mode, name, a, bad)
            assert np.array_equal(want[1], imgs[1]) and np.array_equal(want[4], imgs[4])
        # every image its own coefficients, all applied
        names = list(sets)
        coef = np.stack([sets[names[(3 * k + 1) % len(names)]] for k in range(len(imgs))])
        ones = np.ones(len(imgs), np.uint8)
        got = _device_warp(imgs, mode, ones, coef, slead=9, dlead=2)
        assert np.array_equal(got, R.warp_batch(imgs, coef, mode, ones, FILL)), (shape, mode)


def test_padded_dst_stride():
    rng = np.random.default_rng(2)
    for shape in ((33, 31), (50, 70)):            # whole image; tiles
        imgs = make_inputs(rng, shape)
        B, img = len(imgs), imgs[0].size
        coef = np.stack([coef_sets(*shape)['rot33.7_shear']] * B)
        stride = img + 7
        dbuf = ch.full((B * stride + 16,), 0xA5, dtype=ch.uint8, device=DEV)
        src = ch.from_numpy(imgs).to(DEV)
        L.affine_batch(src, dbuf[1:], R.BILINEAR, FILL, ch.from_numpy(mixed_apply()).to(DEV),
                       ch.from_numpy(coef).to(DEV), dst_stride=stride)
        out = dbuf.cpu().numpy()
        want = R.warp_batch(imgs, coef, R.BILINEAR, mixed_apply(), FILL)
        for k in range(B):
            o = 1 + k * stride
            assert np.array_equal(out[o:o + img].reshape(imgs[k].shape), want[k]), (shape, k)
            assert (out[o + img:o + stride] == 0xA5).all()
        assert out[0] == 0xA5


def test_invalid_arguments_are_rejected_before_any_launch():
    lib = L.lib()
    img = ch.full((2, 40, 40, 3), 77, dtype=ch.uint8, device=DEV)
    other = ch.full((2, 40, 40, 3), 66, dtype=ch.uint8, device=DEV)
    apply = ch.ones((2,), dtype=ch.uint8, device=DEV)
    coef = ch.from_numpy(np.stack([np.array(R.IDENTITY, np.int64)] * 2)).to(DEV)
    fill = np.zeros(3, np.uint8)
    fp = fill.ctypes.data
    ch.cuda.synchronize()
    for off in (0, 1, 4799, 9599):
        assert lib.ffcv_affine_batch(None, img.data_ptr(), img.data_ptr() + off, 2, 40, 40, 0, fp, apply.data_ptr(),
                                     coef.data_ptr(), 0) == -1
        assert b'overlap' in lib.ffcv_last_error()
    for h, w, mode, n in ((40, 40, 2, 2), (0, 40, 0, 2), (40, 32768, 0, 2), (40, 40, 0, -1)):
        assert lib.ffcv_affine_batch(None, img.data_ptr(), other.data_ptr(), n, h, w, mode, fp, apply.data_ptr(),
                                     coef.data_ptr(), 0) == -1
    assert lib.ffcv_affine_batch(None, img.data_ptr(), other.data_ptr(), 2, 40, 40, 0, fp, None, coef.data_ptr(),
                                 0) == -1
    assert lib.ffcv_affine_batch(None, img.data_ptr(), other.data_ptr(), 0, 40, 40, 0, fp, apply.data_ptr(),
                                 coef.data_ptr(), 0) == 0
    with pytest.raises(L.FFCVError, match='overlap'):
        L.affine_batch(img, img, 0, fill, apply, coef)
    ch.cuda.synchronize()
    assert (img == 77).all() and (other == 66).all()


@pytest.mark.parametrize('config', range(3))
def test_device_draws_equal_host_draws_under_the_guard(config):
    cfg = R.CONFIGS[config]
    ids = np.arange(256, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for H, W in R.GUARD_SHAPES:
        rg = R.ranges(H, W, **cfg)
        for i in range(256):
            assert R.guard_holds(R.draw_coefficients(SEED, 0, i, 0.5, rg, H, W)[1]), (config, H, W, i)
        for p in (0.5, 1.0):
            apply = ch.full((256,), 9, dtype=ch.uint8, device=DEV)
            coef = ch.full((256, 6), -7, dtype=ch.int64, device=DEV)
            status = ch.full((256,), -1, dtype=ch.int32, device=DEV)
            L.affine_draw_batch(d_ids, SEED, 0, p, rg, H, W, apply, coef, status)
            ha, hq = L.affine_draw_batch_host(ids, SEED, 0, p, rg, H, W)
            assert (status == 0).all()
            assert np.array_equal(apply.cpu().numpy(), ha) and (ha.all() if p == 1.0 else 0 < ha.sum() < 256)
            assert np.array_equal(coef.cpu().numpy(), hq), (config, H, W)
        assert np.array_equal(hq[5], R.draw_coefficients(SEED, 0, 5, 1.0, rg, H, W)[2])


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m):
    fn = os.path.join(tmpdir_m, 'affine_raw.beton')
    if not os.path.exists(fn):
        write(fn, NaturalDS(64, hw=(32, 32), seed=4), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn


@pytest.fixture(scope='module')
def cpu_epochs(tmpdir_m):
    """Two epochs of the CPU Loader per interpolation, computed once."""
    fn = _beton(tmpdir_m)
    out = {}
    for interpolation in ('bilinear', 'nearest'):
        cpu = Loader(fn, batch_size=16, device='cpu', seed=SEED, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomAffine(interpolation=interpolation, fill=FILL, p=0.8,
                                                            **R.CONFIGS[0]), ToTensor()]})
        out[interpolation] = [np.concatenate([im.numpy() for im, _ in cpu]) for _ in range(2)]
        assert not np.array_equal(out[interpolation][0], out[interpolation][1])
    return out


@pytest.mark.parametrize('interpolation', ('bilinear', 'nearest'))
def test_device_loader_matches_cpu_loader(tmpdir_m, cpu_epochs, interpolation):
    """32 x 32 raw, 64 samples, seed 7, the first configuration: one batch per
    launch and two batches per launch group, bit for bit against the CPU
    Loader."""
    fn = _beton(tmpdir_m)
    want = cpu_epochs[interpolation]
    for i in range(64):     # the guard, for every sample and both epochs the comparison uses
        for epoch in range(2):
            rg = R.ranges(32, 32, **R.CONFIGS[0])
            assert R.guard_holds(R.draw_coefficients(SEED, epoch, i, 0.8, rg, 32, 32)[1]), (epoch, i)

    def dev(**kw):
        return Loader(fn, batch_size=16, seed=SEED, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomAffine(interpolation=interpolation, fill=FILL, p=0.8,
                                                            **R.CONFIGS[0]), ToTensor(), ToDevice(DEV)],
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict(batches_per_launch=2)):
        loader = dev(**kw)
        assert loader.graph.groupable()                     # launch groups are kept
        assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
        assert launch_group(loader, len(loader)) == kw['batches_per_launch']
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            assert got.dtype == np.uint8 and got.shape == want_u8.shape
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (interpolation, kw, bad[:8])


def test_chain_with_flip_and_normalize_matches_cpu_loader(tmpdir_m):
    """[decoder, ToTensor, ToDevice, RandomAffine, RandomHorizontalFlip,
    ToTorchImage, NormalizeImage fp16] on the device against the CPU Loader's
    uint8 images through the normalisation table."""
    fn = _beton(tmpdir_m)
    mean, std = np.array([125.307, 122.961, 113.8575]), np.array([51.5865, 50.847, 51.255])
    lut = ((np.arange(256)[:, None] - mean[None, :]) / std[None, :]).astype(np.float16)   # normalize.py:42-49

    def ops():
        return [RandomAffine(180, fill=FILL), RandomHorizontalFlip()]
    cpu = Loader(fn, batch_size=16, device='cpu', seed=SEED, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder()] + ops() + [ToTensor()]})
    loader = Loader(fn, batch_size=16, seed=SEED, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder(), ToTensor(), ToDevice(DEV)] + ops() +
                 [ToTorchImage(), NormalizeImage(mean, std, np.float16)],
        'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]})
    assert loader.graph.groupable()
    assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
    rg = R.ranges(32, 32, **R.CONFIGS[1])
    for i in range(64):
        assert R.guard_holds(R.draw_coefficients(SEED, 0, i, 1.0, rg, 32, 32)[1]), i
    want_u8 = np.concatenate([im.numpy() for im, _ in cpu])
    got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in loader])
    assert got.dtype == np.float16 and got.shape == want_u8.shape
    want = np.stack([lut[want_u8[..., c], c] for c in range(3)], -1)
    bad = [k for k in range(len(got)) if not np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16))]
    assert not bad, bad[:8]
