"""RandomHue / RandomColorJitter on the MI355X, bit for bit against the host
twin (itself pinned to numpy in tests/test_hue.py): ffcv_hue_batch on all 2^24
RGB triples, on small shapes in both regimes at every byte alignment inside
guarded buffers, the device draws against the host draws, and device Loaders
against the CPU Loader under the same seed."""
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
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomGrayscale, RandomHue,
                                 RandomColorJitter)
from tests import hue_ref as R
from tests.helpers import NaturalDS, write

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


@pytest.fixture(scope='module')
def triples():
    return R.all_triples()[None]


def _host(imgs, apply, shift):
    out = np.ascontiguousarray(imgs).copy()
    L.hue_batch_host(out, apply, shift)
    return out


def _device_hue(imgs, apply, shift, lead=0):
    """ffcv_hue_batch on a copy of imgs placed GUARD + lead bytes into a 16-byte
    aligned device buffer with GUARD bytes behind it; returns the images and
    checks that the guard bytes on both sides came back as they were."""
    nb = imgs.size
    buf = ch.full((GUARD + lead + nb + GUARD + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + lead
    view = buf[lo:lo + nb].view(imgs.shape)
    view.copy_(ch.from_numpy(imgs))
    L.hue_batch(view, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                ch.from_numpy(np.ascontiguousarray(shift, np.float64)).to(DEV))
    out = buf.cpu().numpy()
    assert (out[:lo] == 0xA5).all() and (out[lo + nb:] == 0xA5).all()
    return out[lo:lo + nb].reshape(imgs.shape)


@pytest.mark.parametrize('d', (0.05, 0.23, -0.37))
def test_all_triples_equal_the_host_twin(triples, d):
    """4096 x 4096: 4,096 tiles of one image.  These d are the ones at which a
    fused multiply-add changes triples (tests/test_hue.py)."""
    got = _device_hue(triples, [1], [d])
    want = _host(triples, [1], [d])
    assert np.array_equal(got, want), int((got != want).any(-1).sum())


@pytest.mark.parametrize('lead', (0, 1, 7, 15))
@pytest.mark.parametrize('shape', ((1, 1), (5, 7), (32, 32), (73, 75)), ids=str)
def test_small_shapes_at_every_alignment(shape, lead):
    """Whole image: 1 x 1, 5 x 7 (105 bytes: images straddle 16-byte chunks),
    32 x 32; tiles: 73 x 75 (16,425 bytes, a last tile of 1,379 pixels).  B = 5,
    images 1 and 4 not applied: they and the guards stay byte-identical."""
    assert (shape[0] * shape[1] * 3 > L.color_jitter_lds_bytes()) == (shape == (73, 75))
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    imgs = rng.integers(0, 256, (5,) + shape + (3,), dtype=np.uint8)
    imgs[2] //= 16
    imgs[3, ..., 1] = imgs[3, ..., 0]      # ties between the channels
    apply = [1, 0, 1, 1, 0]
    shift = [0.05, 0.3, -0.37, 0.23, -0.5]
    got = _device_hue(imgs, apply, shift, lead)
    want = _host(imgs, apply, shift)
    assert np.array_equal(got[[1, 4]], imgs[[1, 4]])
    bad = [k for k in range(5) if not np.array_equal(got[k], want[k])]
    assert not bad, (shape, lead, bad)
    assert not np.array_equal(want[0], imgs[0]) or shape == (1, 1)


def test_device_draws_equal_host_draws():
    rng = np.random.default_rng(8)
    n = 4096
    ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    ids[:16] = np.arange(16)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for seed, epoch, p, m in ((0, 0, 0.5, 0.1), (2 ** 63 + 5, 7, 0.25, 0.5), (12345, 400, 1.0, 0.0)):
        apply = ch.full((n,), 9, dtype=ch.uint8, device=DEV)
        shift = ch.zeros((n,), dtype=ch.float64, device=DEV)
        status = ch.full((n,), -1, dtype=ch.int32, device=DEV)
        L.hue_draw_batch(d_ids, seed, epoch, p, m, apply, shift, status)
        ha, hs = L.hue_draw_batch_host(ids, seed, epoch, p, m)
        assert (status == 0).all()
        assert np.array_equal(apply.cpu().numpy(), ha)
        assert np.array_equal(shift.cpu().numpy().view(np.uint64), hs.view(np.uint64))
        if p == 0.5:
            assert 1500 < int(ha.sum()) < 2600 and -0.1 <= hs.min() < -0.09 and 0.09 < hs.max() <= 0.1
    for seed, epoch, p, mags in ((3, 1, 0.8, (0.4, 0.4, 0.2, 0.1)), (2 ** 63 + 5, 7, 0.5, (0.0, 1.5, 0.0, 0.5)),
                                 (9, 2, 1.0, (0.3, 0.0, 0.0, 0.0))):
        rows = L.color_jitter_joint_rows(mags)
        apply = ch.full((rows + 1, n), 9, dtype=ch.uint8, device=DEV)
        ratio = ch.full((rows + 1, n), -7.0, dtype=ch.float64, device=DEV)
        status = ch.full((n,), -1, dtype=ch.int32, device=DEV)
        L.color_jitter_joint_draw_batch(d_ids, seed, epoch, p, mags, apply, ratio, status)
        ha, hr = L.color_jitter_joint_draw_batch_host(ids, seed, epoch, p, mags)
        assert (status == 0).all() and ha.shape == (rows, n)
        assert np.array_equal(apply.cpu().numpy()[:rows], ha) and (apply[rows] == 9).all()
        assert np.array_equal(ratio.cpu().numpy()[:rows].view(np.uint64), hr.view(np.uint64))
        assert (ratio[rows] == -7.0).all()


def test_abi_rejects_bad_arguments_before_a_launch():
    lib = L.lib()
    n = 4
    img = ch.full((n, 80, 80, 3), 77, dtype=ch.uint8, device=DEV)
    img[..., 0] = 99                                                   # coloured: a launch would change it
    before = img.clone()
    apply = ch.ones((4, n), dtype=ch.uint8, device=DEV)
    shift = ch.full((4, n), 0.25, dtype=ch.float64, device=DEV)
    ids = ch.arange(n, dtype=ch.int64, device=DEV)
    mags = np.array([0.4, 0.4, 0.2, 0.1])
    ch.cuda.synchronize()
    i, a, s, d = img.data_ptr(), apply.data_ptr(), shift.data_ptr(), ids.data_ptr()
    for args in ((None, n, 80, 80, a, s), (i, n, 80, 80, None, s), (i, n, 80, 80, a, None), (i, -1, 80, 80, a, s),
                 (i, n, 0, 80, a, s), (i, n, 80, -3, a, s), (i, n, 26755, 26755, a, s)):
        assert lib.ffcv_hue_batch(None, *args) == -1 and b'ffcv_hue_batch:' in lib.ffcv_last_error()
    for args in ((None, n, 0, 0, 0.5, 0.1, a, s, None), (d, n, 0, 0, 0.5, 0.1, None, s, None),
                 (d, n, 0, 0, 0.5, 0.1, a, None, None), (d, n, 0, 0, 1.5, 0.1, a, s, None),
                 (d, n, 0, 0, 0.5, 0.6, a, s, None), (d, n, 0, 0, 0.5, float('nan'), a, s, None)):
        assert lib.ffcv_hue_draw_batch(None, *args) == -1 and b'ffcv_hue_draw_batch:' in lib.ffcv_last_error()
    m = mags.ctypes.data
    for args in ((None, n, 0, 0, 0.5, m, a, s, None), (d, n, 0, 0, 0.5, None, a, s, None),
                 (d, n, 0, 0, 0.5, m, None, s, None), (d, n, 0, 0, 0.5, m, a, None, None),
                 (d, n, 0, 0, -0.1, m, a, s, None)):
        assert lib.ffcv_color_jitter_joint_draw_batch(None, *args) == -1
        assert b'ffcv_color_jitter_joint_draw_batch:' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert ch.equal(img, before) and (apply == 1).all() and (shift == 0.25).all()   # nothing was launched
    assert lib.ffcv_hue_batch(None, i, 0, 80, 80, a, s) == 0                       # an empty batch is fine
    with pytest.raises(TypeError):
        L.hue_batch(img.permute(0, 2, 1, 3), apply[0], shift[0])


# ------------------------------------------------------------- Loaders --
def _chains():
    return {'hue': lambda: [RandomHue(0.1, p=0.5)],
            'joint_gray': lambda: [RandomColorJitter(0.4, 0.4, 0.2, 0.1, p=0.8), RandomGrayscale(0.2)]}


@pytest.mark.parametrize('case', sorted(_chains()))
def test_device_loader_matches_cpu_loader(tmpdir_m, case):
    """[decoder, ToTensor, ToDevice, the new operations, ToTorchImage,
    NormalizeImage fp16] on the device Loader, one batch per launch, with the
    Loader's own launch groups and with groups of 3, over two epochs, against
    the CPU Loader ([decoder, the new operations, ToTensor]) under the same
    seed."""
    fn = os.path.join(tmpdir_m, 'hue_raw.beton')
    if not os.path.exists(fn):
        write(fn, NaturalDS(40, hw=(32, 32), seed=4), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    ops, seed = _chains()[case], 17
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder()] + ops() + [ToTensor()]})
    want = [np.concatenate([im.numpy() for im, _ in cpu]) for _ in range(2)]
    plain = np.concatenate([im.numpy() for im, _ in Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False,
                                                           pipelines={'image': [SimpleRGBImageDecoder(), ToTensor()]})])
    changed = [(w != plain).any(axis=(1, 2, 3)) for w in want]
    assert not np.array_equal(want[0], want[1]) and 5 < changed[0].sum() < 40   # some applied, some left alone

    def dev(**kw):
        return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), ToTensor(), ToDevice(DEV)] + ops() +
                     [ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)],
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict(), dict(batches_per_launch=3)):
        loader = dev(**kw)
        assert loader.graph.groupable()                     # launch groups are kept
        assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
        assert launch_group(loader, len(loader)) == (kw.get('batches_per_launch') or len(loader))
        for want_u8 in want:
            got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in loader])
            assert got.dtype == np.float16 and got.shape == want_u8.shape
            lut = np.stack([LUT[want_u8[..., c], c] for c in range(3)], -1)
            bad = [k for k in range(len(got)) if not np.array_equal(got[k].view(np.uint16), lut[k].view(np.uint16))]
            assert not bad, (case, kw, bad[:8])
