"""RandomBrightness / RandomContrast / RandomSaturation on the MI355X, bit for
bit against numpy applying the operations one after another
(tests/color_jitter_ref.py): ffcv_color_jitter_batch with every program in
both regimes (whole image in LDS; tiles, two passes with contrast), the
reference's own image pairs, device draws against host draws, and device
Loaders against the CPU Loader under the same seed."""
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomHorizontalFlip,
                                 RandomBrightness, RandomContrast, RandomSaturation)
from tests.helpers import NaturalDS, write
from tests.color_jitter_ref import (BRIGHTNESS, CONTRAST, SATURATION, OP_ID, apply_program_batch,
                                    near_integer_triples)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = (BRIGHTNESS, CONTRAST, SATURATION)
PROGRAMS = [p for n in (1, 2, 3) for p in itertools.permutations(KINDS, n)]   # 3 + 6 + 6
RATIOS = (0.0, 0.3, 0.5000000001, 0.97, 1.0, 1.4, 3.7)
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
CFILL = (200, 201, 202)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'color_jitter.npz')


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_program(imgs, kinds, apply, ratio, lead=1):
    """ffcv_color_jitter_batch on a copy of imgs placed `lead` bytes into a
    guarded device buffer; returns the images and checks the guards."""
    B, H, W, _ = imgs.shape
    nb = imgs.size
    buf = ch.full((lead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    view = buf[lead:lead + nb].view(B, H, W, 3)
    view.copy_(ch.from_numpy(imgs))
    ws = None
    if H * W * 3 > L.color_jitter_lds_bytes() and CONTRAST in kinds:
        ws = ch.full((B,), -1, dtype=ch.int64, device=DEV)    # the call zeroes it
    L.color_jitter_batch(view, list(kinds), ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                         ch.from_numpy(np.ascontiguousarray(ratio, np.float64)).to(DEV), ws)
    out = buf.cpu().numpy()
    assert (out[:lead] == 0xA5).all() and (out[lead + nb:] == 0xA5).all()
    return out[lead:lead + nb].reshape(imgs.shape)


def _shapes():
    lds = 16384   # asserted against the library below
    return [(1, 1), (1, 7), (3, 5), (32, 32), (33, 31), (43, 127), (2, 2731), (231, 227)], lds


@pytest.mark.parametrize('shape', _shapes()[0])
def test_every_program_matches_numpy(shape):
    """All one-, two- and three-step programs on 67 images with mixed apply
    flags (two images with every flag 0: untouched), images at every byte
    alignment.  43 x 127 is the largest image of the one-workgroup regime
    (16,383 bytes), 2 x 2731 the first beyond it (16,386: two tiles), 231 x 227
    spans 13 tiles with a short last one."""
    lds = L.color_jitter_lds_bytes()
    assert lds == _shapes()[1] and 43 * 127 * 3 <= lds < 2 * 2731 * 3 and lds - 43 * 127 * 3 < 3
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    B = 67
    imgs = rng.integers(0, 256, (B,) + shape + (3,), dtype=np.uint8)
    imgs[1] //= 16          # dark: a contrast mean near 0
    imgs[3] |= 0xF0         # bright
    for kinds in PROGRAMS:
        n = len(kinds)
        apply = rng.integers(0, 2, (n, B)).astype(np.uint8)
        apply[:, 0] = 1
        apply[:, [2, 66]] = 0
        ratio = np.where(rng.random((n, B)) < 0.5, rng.choice(RATIOS, (n, B)), rng.uniform(0, 2.5, (n, B)))
        got = _device_program(imgs, kinds, apply, ratio, lead=1 + len(kinds))
        want = apply_program_batch(imgs, kinds, apply, ratio)
        bad = [k for k in range(B) if not np.array_equal(got[k], want[k])]
        assert not bad, (shape, kinds, bad[:5])
        assert np.array_equal(got[2], imgs[2]) and np.array_equal(got[66], imgs[66])


def test_near_integer_triples():
    """The 1,704 RGB triples whose float64 gray sum lies within 1e-9 of an
    integer (a fused multiply-add changes 276 of them), 24 x 71, under
    contrast and saturation, alone and chained."""
    t = near_integer_triples()
    assert len(t) == 1704
    img = t.reshape(24, 71, 3)
    imgs = np.stack([img] * len(RATIOS))
    for kinds in ((CONTRAST,), (SATURATION,), (SATURATION, CONTRAST), (CONTRAST, SATURATION)):
        apply = np.ones((len(kinds), len(RATIOS)), np.uint8)
        ratio = np.stack([np.roll(RATIOS, i) for i in range(len(kinds))])
        got = _device_program(imgs, kinds, apply, ratio, lead=3)
        assert np.array_equal(got, apply_program_batch(imgs, kinds, apply, ratio)), kinds
    # the host twin computes the same (same pixel functions)
    host = imgs.copy()
    L.color_jitter_batch_host(host, [SATURATION], np.ones((1, len(RATIOS)), np.uint8), np.array([RATIOS]))
    assert np.array_equal(host, _device_program(imgs, (SATURATION,), np.ones((1, len(RATIOS)), np.uint8),
                                                np.array([RATIOS])))


def test_golden_pairs_through_the_kernel():
    z = np.load(GOLDEN)
    n = len(z['meta_op'])
    assert n >= 90
    applied = 0
    for k in range(n):
        kind, seed, m, p = int(z['meta_op'][k]), int(z['meta_seed'][k]), float(z['meta_magnitude'][k]), \
            float(z['meta_p'][k])
        rs = np.random.RandomState(seed)
        apply = rs.rand() < p
        ratio = rs.uniform(max(0, 1 - m), 1 + m)
        got = _device_program(z[f'in_{k}'][None], (kind,), [[int(apply)]], [[ratio]], lead=k % 16)
        assert np.array_equal(got[0], z[f'out_{k}']), (k, kind)
        applied += bool(apply)
    assert applied >= 60


def test_device_draws_equal_host_draws():
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 2 ** 40, 4096).astype(np.uint64)
    ids[:16] = np.arange(16)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for kind in KINDS:
        for seed, epoch, p, m in ((0, 0, 0.5, 0.4), (2 ** 63 + 5, 7, 0.25, 1.5), (12345, 400, 1.0, 0.0)):
            apply = ch.full((4096,), 9, dtype=ch.uint8, device=DEV)
            ratio = ch.zeros((4096,), dtype=ch.float64, device=DEV)
            status = ch.full((4096,), -1, dtype=ch.int32, device=DEV)
            L.color_jitter_draw_batch(d_ids, seed, epoch, OP_ID[kind], p, m, apply, ratio, status)
            ha, hr = L.color_jitter_draw_batch_host(ids, seed, epoch, OP_ID[kind], p, m)
            assert (status == 0).all()
            assert np.array_equal(apply.cpu().numpy(), ha)
            assert np.array_equal(ratio.cpu().numpy().view(np.uint64), hr.view(np.uint64))
            if p == 0.5:
                assert 1500 < int(ha.sum()) < 2600 and hr.min() >= 0.6 and hr.max() <= 1.4


def test_abi_rejects_bad_arguments():
    import ctypes
    lib = L.lib()
    img = ch.full((2, 80, 80, 3), 77, dtype=ch.uint8, device=DEV)   # beyond the one-workgroup regime
    apply = ch.ones((3, 2), dtype=ch.uint8, device=DEV)
    ratio = ch.full((3, 2), 0.5, dtype=ch.float64, device=DEV)
    ws = ch.zeros((2,), dtype=ch.int64, device=DEV)
    ch.cuda.synchronize()

    def call(p, ws_ptr=ws.data_ptr(), ws_bytes=16, h=80):
        return lib.ffcv_color_jitter_batch(None, img.data_ptr(), 2, h, 80, ctypes.byref(p), apply.data_ptr(),
                                           ratio.data_ptr(), ws_ptr, ws_bytes)
    for steps, msg in (([], b'1 to 3 steps'), ([2, 2], b'repeated'), ([1, 7], b'unknown step')):
        assert call(L.color_jitter_params(steps)) == -1 and msg in lib.ffcv_last_error()
    p = L.color_jitter_params([1, 2])
    for kw in (dict(ws_ptr=None), dict(ws_bytes=8), dict(ws_ptr=ws.data_ptr() + 4), dict(h=0)):
        assert call(p, **kw) == -1 and b'ffcv_color_jitter_batch' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert (img == 77).all()                                        # nothing was launched
    assert call(L.color_jitter_params([1, 3]), ws_ptr=None, ws_bytes=0) == 0   # no contrast: no workspace
    with pytest.raises(TypeError):
        L.color_jitter_batch(img.permute(0, 2, 1, 3), [1], apply, ratio)


# ------------------------------------------------------------- Loaders --
def _jitter_ops():
    return [RandomBrightness(0.5, 0.6), RandomContrast(0.7), RandomSaturation(1.2, p=0.5)]


def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


def _cpu_epochs(fn, decoder, seed, cut, epochs=2):
    """uint8 HWC outputs of the CPU Loader, per epoch, in sequential order."""
    loader = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5)] + _jitter_ops() + [Cutout(cut, CFILL), ToTensor()]})
    return [np.concatenate([im.numpy() for im, _ in loader]) for _ in range(epochs)]


def _dev_loader(fn, decoder, seed, cut, **kw):
    return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5)] + _jitter_ops() +
                 [Cutout(cut, CFILL), ToTensor(), ToDevice(DEV), ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)],
        'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)


LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49


def _check_device_loader(loader, want_epochs, n):
    ops = loader.pipeline_specs['image'].transforms
    jit = [o for o in ops if isinstance(o, (RandomBrightness, RandomContrast, RandomSaturation))]
    assert [o._absorbed for o in jit] == [False, True, True] and jit[0]._program == jit
    for want_u8 in want_epochs:
        got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in loader])
        assert got.dtype == np.float16 and got.shape == want_u8.shape and len(got) == n
        want = np.stack([LUT[want_u8[..., c], c] for c in range(3)], -1)
        bad = [k for k in range(n) if not np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16))]
        assert not bad, bad[:8]


@pytest.mark.parametrize('case', ['raw32', 'jpeg64', 'jpeg80x72'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case):
    """[decoder, flip, brightness, contrast, saturation, Cutout, ToTensor,
    ToDevice, ToTorchImage, NormalizeImage fp16] on the device-cache Loader,
    the PCIe Loader and with launch groups of 3, against the CPU Loader under
    the same seed.  32 x 32 raw and 64 x 64 crops run the one-workgroup
    regime, 80 x 72 crops (17,280 bytes) the tiled two-pass one."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'cj_raw.beton', 'raw', 40, (32, 32), 4)
        decoder, cut = SimpleRGBImageDecoder, 8
    else:
        fn = _beton(tmpdir_m, 'cj_jpg.beton', 'jpg', 40, (96, 120), 5)
        size = (64, 64) if case == 'jpeg64' else (80, 72)
        decoder, cut = (lambda: RandomResizedCropRGBImageDecoder(size)), 16
    seed = 17
    want = _cpu_epochs(fn, decoder, seed, cut)
    assert not np.array_equal(want[0], want[1])
    _check_device_loader(_dev_loader(fn, decoder, seed, cut, device_cache=True), want, 40)
    _check_device_loader(_dev_loader(fn, decoder, seed, cut, device_cache=False), want[:1], 40)
    _check_device_loader(_dev_loader(fn, decoder, seed, cut, batches_per_launch=3), want, 40)
