"""RandomTranslate and the fused small-image launch on the MI355X, bit for bit
against numpy applying the operations one after another with the seeding
contract's draws (tests/translate_ref.py): every ordering of flip / translate
/ cutout behind a SimpleRGBImageDecoder of raw samples (one launch,
ffcv_simple_aug_batch), its edges and its fp16 epilogue, the staged paths
(PCIe gather; JPEG samples, where RandomTranslate runs its standalone kernel),
launch groups and epochs, and the new C ABI's argument checks."""
import ctypes
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd.loader import Loader, OrderOption
from ffcv_amd.reader import Reader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomHorizontalFlip,
                                 RandomTranslate)
from tests.helpers import NaturalDS, write, samples_of
from tests.translate_ref import apply_chain, apply_steps, translate_draw, translate_np

pytestmark = pytest.mark.gpu
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
TFILL, CFILL = (9, 8, 7), (200, 201, 202)
CHAINS = ['t', 'tf', 'ft', 'tc', 'ct'] + [''.join(p) for p in itertools.permutations('ftc')]


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _ops(chain, pad, cut, tfill=TFILL, cfill=CFILL):
    mk = {'f': lambda: RandomHorizontalFlip(0.5), 't': lambda: RandomTranslate(pad, tfill),
          'c': lambda: Cutout(cut, cfill)}
    return [mk[s]() for s in chain]


def _raw_beton(tmpdir_m, name, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    ds = NaturalDS(n, hw=hw, seed=seed)
    if not os.path.exists(fn):
        write(fn, ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn, ds


def _loader(fn, chain, pad, cut, seed, batch_size=8, tail=(), **kw):
    return Loader(fn, batch_size=batch_size, seed=seed, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder()] + _ops(chain, pad, cut) + [ToTensor(), ToDevice('cuda:0')] + list(tail),
        'label': [IntDecoder(), ToTensor(), ToDevice('cuda:0')]}, **kw)


def _check_epoch(loader, imgs, chain, pad, cut, seed, epoch, batch_size=8):
    """One epoch in sequential order against numpy; returns (samples, flipped)."""
    n = flips = 0
    for b, (images, labels) in enumerate(loader):
        got = images.cpu().numpy()
        assert got.dtype == np.uint8 and got.shape[1:] == imgs[0].shape
        for k in range(got.shape[0]):
            sid = b * batch_size + k
            want, f = apply_chain(imgs[sid], chain, seed, epoch, sid, pad=pad, tfill=TFILL, cut=cut, cfill=CFILL)
            assert np.array_equal(got[k], want), (chain, epoch, sid)
            assert int(labels[k]) == sid % 10
            flips += f
            n += 1
    return n, flips


@pytest.mark.parametrize('chain', CHAINS)
def test_every_order_fused(tmpdir_m, chain):
    """Odd width, rows of 30 bytes, samples at offsets that are no multiple of
    4, a short last batch: every chain that contains translate is one launch."""
    fn, ds = _raw_beton(tmpdir_m, 'odd.beton', 37, (13, 10), 3)
    ptrs = Reader(fn).metadata['f0']['data_ptr']
    assert (ptrs % 4 != 0).any() and (ptrs % 16 != 0).any()
    seed = 21
    loader = _loader(fn, chain, 3, 4, seed)
    dec = loader.pipeline_specs['image'].decoder
    assert dec.fused and len(dec._fused_steps) == len(chain)
    for epoch in range(2):
        n, flips = _check_epoch(loader, ds.imgs, chain, 3, 4, seed, epoch)
        assert n == 37
        if 'f' in chain:
            assert 0 < flips < 37


@pytest.mark.parametrize('hw,pad,chain,cut', [
    ((1, 1), 0, 't', 0), ((1, 1), 1, 't', 0), ((1, 1), 9, 't', 0), ((1, 1), 1, 'ftc', 1),
    ((5, 7), 0, 't', 0), ((5, 7), 1, 'ft', 0), ((5, 7), 9, 't', 0), ((5, 7), 9, 'ctf', 5),
    ((6, 6), 1, 'tc', 6), ((6, 6), 1, 'ct', 6),
    ((40, 300), 5, 'ftc', 11), ((40, 300), 45, 'tcf', 40)])
def test_edges(tmpdir_m, hw, pad, chain, cut):
    """Tiny images, padding 0 (identity) / 1 / larger than the image (some
    samples all fill), a cutout as large as the image, and an image whose rows
    one workgroup cannot stage at once (40 x 300: three bands of rows)."""
    n = 12 if hw == (40, 300) else 30
    fn, ds = _raw_beton(tmpdir_m, f'edge_{hw[0]}x{hw[1]}.beton', n, hw, 5)
    seed = 4
    loader = _loader(fn, chain, pad, cut, seed)
    assert loader.pipeline_specs['image'].decoder.fused
    got_n, _ = _check_epoch(loader, ds.imgs, chain, pad, cut, seed, 0)
    assert got_n == n
    if chain == 't':
        outs = np.concatenate([im.cpu().numpy() for im, _ in loader])  # epoch 1
        if pad == 0:
            assert np.array_equal(outs, np.stack(ds.imgs))
        if pad == 9:
            whole = [(o == np.array(TFILL, np.uint8)).all() for o in outs]
            assert any(whole) and (hw == (1, 1) or not all(whole))


def test_fp16_epilogue_cifar_chain(tmpdir_m):
    """flip -> translate(2) -> cutout(4) -> ToTorchImage -> NormalizeImage(fp16)
    on 32x32 raw images: bits equal lut[u8] of the numpy expectation, NCHW
    view of channels-last storage."""
    fn, ds = _raw_beton(tmpdir_m, 'cifar.beton', 64, (32, 32), 7)
    seed = 31
    loader = _loader(fn, 'ftc', 2, 4, seed, batch_size=32,
                     tail=[ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)])
    dec = loader.pipeline_specs['image'].decoder
    assert dec.fused and dec.output_dtype == ch.float16
    lut = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)  # normalize.py:42-49
    n = 0
    for b, (images, labels) in enumerate(loader):
        assert images.shape == (32, 3, 32, 32) and images.dtype == ch.float16
        assert images.is_contiguous(memory_format=ch.channels_last)
        got = images.permute(0, 2, 3, 1).cpu().numpy()
        for k in range(32):
            sid = b * 32 + k
            u8, _ = apply_chain(ds.imgs[sid], 'ftc', seed, 0, sid, pad=2, tfill=TFILL, cut=4, cfill=CFILL)
            want = np.stack([lut[u8[..., c], c] for c in range(3)], -1)
            assert np.array_equal(got[k].view(np.uint16), want.view(np.uint16)), sid
            n += 1
    assert n == 64


def test_pcie_gather_matches_device_cache(tmpdir_m):
    fn, ds = _raw_beton(tmpdir_m, 'odd.beton', 37, (13, 10), 3)
    a = _loader(fn, 'ctf', 3, 4, 8, device_cache=True)
    b = _loader(fn, 'ctf', 3, 4, 8, device_cache=False)
    assert a.pipeline_specs['image'].decoder.fused and b.pipeline_specs['image'].decoder.fused
    assert a.device_dataset.data is not None and b.device_dataset.data is None
    for epoch in range(2):
        n = 0
        for (ia, la), (ib, lb) in zip(a, b):
            assert ch.equal(la, lb) and ch.equal(ia, ib)
            n += len(la)
        assert n == 37
    _check_epoch(b, ds.imgs, 'ctf', 3, 4, 8, 2)


def test_jpeg_samples_run_standalone_translate(tmpdir_m, oracle):
    """A field with JPEG samples is not lowered: the JPEG decode kernels run,
    then RandomTranslate's own kernel (ffcv_translate_batch) with the
    contract's draws shifts the decoded images."""
    fn = os.path.join(tmpdir_m, 'tr_jpg.beton')
    write(fn, NaturalDS(20, hw=(24, 40), seed=9), {'image': RGBImageField(write_mode='jpg'), 'label': IntField()})
    samples = samples_of(fn)
    seed = 6
    loader = _loader(fn, 't', 5, 0, seed)
    dec = loader.pipeline_specs['image'].decoder
    assert not dec.fused and dec._has_jpg
    moved = 0
    for b, (images, labels) in enumerate(loader):
        got = images.cpu().numpy()
        for k in range(got.shape[0]):
            sid = b * 8 + k
            y, x = translate_draw(seed, 0, sid, 5)
            want = translate_np(oracle.jpeg_decode(samples[sid][0]), y, x, 5, TFILL)
            assert np.array_equal(got[k], want), sid
            moved += (y, x) != (5, 5)
    assert moved > 0


def test_epochs_seeds_and_launch_groups(tmpdir_m):
    """Two epochs differ, the same seed repeats, and grouped launches hand out
    the batches that one launch per batch gives (short last batch included)."""
    fn, ds = _raw_beton(tmpdir_m, 'grp.beton', 100, (16, 12), 6)

    def mk(**kw):
        return Loader(fn, batch_size=16, order=OrderOption.RANDOM, seed=7, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), RandomTranslate(2, TFILL),
                      Cutout(4, CFILL), ToTensor(), ToDevice('cuda:0'), ToTorchImage(),
                      NormalizeImage(MEAN, STD, np.float16)],
            'label': [IntDecoder(), ToTensor(), ToDevice('cuda:0')]}, **kw)
    a, b, c, d = mk(batches_per_launch=1), mk(), mk(batches_per_launch=3), mk(batches_per_launch=1)
    assert all(l.pipeline_specs['image'].decoder.fused for l in (a, b, c, d))
    for epoch in range(2):
        n = 0
        for (ia, la), (ib, lb), (ic, lc) in zip(a, b, c):
            assert ch.equal(la, lb) and ch.equal(la, lc)
            assert ch.equal(ia.view(ch.int16), ib.view(ch.int16))
            assert ch.equal(ia.view(ch.int16), ic.view(ch.int16))
            n += len(la)
            if epoch == 0 and n == len(la):
                first = ia.clone()
        assert n == 100
    e0 = next(iter(d))[0]
    assert ch.equal(e0.view(ch.int16), first.view(ch.int16))       # same seed, same epoch: same batch
    # sequential order: the same samples in the same places, new draws every epoch
    s = Loader(fn, batch_size=50, seed=7, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomTranslate(2, TFILL), ToTensor(), ToDevice('cuda:0')]})
    x0 = next(iter(s))[0].cpu().clone()
    x1 = next(iter(s))[0].cpu().clone()
    assert not ch.equal(x0, x1)
    for k in range(50):
        assert np.array_equal(x1[k].numpy(), apply_chain(ds.imgs[k], 't', 7, 1, k, pad=2, tfill=TFILL)[0])


def test_abi_direct_rows_wider_than_the_stage(hip_lib):
    """ffcv_simple_aug_batch called directly with chosen decisions: rows of
    16,500 bytes (wider than one workgroup's stage: read from global memory),
    samples at odd byte offsets, an output stride that leaves every second
    sample misaligned, u8 and fp16."""
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(2)
    H, W, B = 3, 5500, 4
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    nb = H * W * 3
    offs = np.array([1, nb + 4, 2 * nb + 11, 3 * nb + 12], np.uint64)
    base = np.zeros(int(offs[-1]) + nb + 16, np.uint8)
    table = np.zeros(B, L.SAMPLE_DTYPE)
    for k in range(B):
        base[int(offs[k]):int(offs[k]) + nb] = imgs[k].reshape(-1)
    table['offset'], table['size'], table['height'], table['width'], table['mode'] = offs, nb, H, W, 1
    flips = np.array([1, 0, 1, 0], np.uint8)
    tyx = np.array([[0, 0], [4, 4], [2, 3], [1, 4]], np.int32)   # padding 2
    cyx = np.array([[0, 0], [1, 5000], [0, 5497], [1, 17]], np.int32)
    dev = 'cuda:0'
    d = {k: ch.from_numpy(v).to(dev) for k, v in dict(base=base, table=table.view(np.uint8), flips=flips,
                                                      tyx=tyx, cyx=cyx).items()}
    lut_np = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)
    lut = ch.from_numpy(lut_np.view(np.int16)).to(dev)
    for chain in ('ftc', 'ctf'):
        p = L.SimpleAugParams()
        p.n_steps = 3
        for i, s in enumerate(chain):
            p.steps[i] = {'f': L.AUG_FLIP, 't': L.AUG_TRANSLATE, 'c': L.AUG_CUTOUT}[s]
        p.padding, p.cutout_size = 2, 2
        for c in range(3):
            p.translate_fill[c], p.cutout_fill[c] = TFILL[c], CFILL[c]
        want = np.stack([apply_steps(imgs[k], chain, flips[k], tyx[k], cyx[k], 2, TFILL, 2, CFILL)
                         for k in range(B)])
        stride = nb + 1
        out = ch.zeros(B * stride, dtype=ch.uint8, device=dev)
        L.simple_aug_batch(d['base'], d['table'], B, H, W, p, d['flips'], d['cyx'], d['tyx'], None, out, stride)
        got = out.cpu().numpy().reshape(B, stride)
        assert np.array_equal(got[:, :nb].reshape(B, H, W, 3), want), chain
        assert (got[:, nb] == 0).all()  # the byte between samples is not written
        stride16 = 2 * nb + 2
        out16 = ch.zeros(B * stride16 // 2, dtype=ch.int16, device=dev)
        L.simple_aug_batch(d['base'], d['table'], B, H, W, p, d['flips'], d['cyx'], d['tyx'], lut, out16, stride16)
        got16 = out16.cpu().numpy().view(np.uint16).reshape(B, stride16 // 2)
        want16 = np.stack([lut_np[want[..., c], c] for c in range(3)], -1).view(np.uint16)
        assert np.array_equal(got16[:, :nb].reshape(B, H, W, 3), want16), chain
        assert (got16[:, nb] == 0).all()


def test_abi_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    dev = 'cuda:0'
    img = ch.full((2, 4, 4, 3), 77, dtype=ch.uint8, device=dev)
    yx = ch.zeros((2, 2), dtype=ch.int32, device=dev)
    fill = (ctypes.c_uint8 * 3)(1, 2, 3)
    ch.cuda.synchronize()
    rc = lib.ffcv_translate_batch(None, img.data_ptr(), img.data_ptr(), 2, 4, 4, yx.data_ptr(), 1, fill)
    assert rc == -1 and b'ffcv_translate_batch' in lib.ffcv_last_error()
    base = ch.zeros(256, dtype=ch.uint8, device=dev)
    smp = ch.zeros(2 * 32, dtype=ch.uint8, device=dev)
    flips = ch.zeros(2, dtype=ch.uint8, device=dev)
    out = ch.full((2, 4, 4, 3), 55, dtype=ch.uint8, device=dev)

    def call(p):
        return lib.ffcv_simple_aug_batch(None, base.data_ptr(), smp.data_ptr(), 2, 4, 4, ctypes.byref(p),
                                         flips.data_ptr(), yx.data_ptr(), yx.data_ptr(), None, out.data_ptr(), 0)
    p = L.SimpleAugParams()
    p.n_steps = 0
    assert call(p) == -1 and b'1 to 3 steps' in lib.ffcv_last_error()
    p.n_steps = 4
    assert call(p) == -1 and b'1 to 3 steps' in lib.ffcv_last_error()
    p.n_steps = 2
    p.steps[0] = p.steps[1] = L.AUG_TRANSLATE
    assert call(p) == -1 and b'repeated' in lib.ffcv_last_error()
    p.steps[1] = 9
    assert call(p) == -1 and b'unknown step' in lib.ffcv_last_error()
    p.steps[1] = L.AUG_CUTOUT
    p.cutout_size = 5
    assert call(p) == -1 and b'cutout_size' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert (img == 77).all() and (out == 55).all()  # nothing was launched
    with pytest.raises(L.FFCVError, match='in-place'):
        L.translate_batch(img, img, yx, 1, (1, 2, 3))
