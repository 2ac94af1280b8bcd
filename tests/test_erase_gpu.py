"""RandomErasing on the MI355X: ffcv_erase_batch bit for bit against the numpy
statement (tests/erase_ref.py) and against the host twin, with the images at
every byte alignment inside guarded buffers; the draw launch; the ABI's
rejections; the layouts the tensor wrapper takes and rejects; the operation
on device tensors outside a Loader; and device Loaders (device cache, PCIe
staging, launch groups of 3, the default grouping) against the CPU Loader and
the statement under one seed, with RandomErasing before ToTensor on uint8 and
after NormalizeImage(float16) with per-pixel noise, once in front of
ImageCutMix."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomHorizontalFlip, ImageCutMix,
                                 RandomErasing)
from ffcv_amd.transforms.erase import noise_table
from tests.helpers import NaturalDS, write
from tests import cutmix_ref as C
from tests import erase_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49
TORCH_DTYPES = {1: ch.uint8, 2: ch.int16, 4: ch.int32}


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a):
    return ch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


def _device_fill(x, boxes, layout, value, tab, keys, lead):
    """ffcv_erase_batch on a copy of x placed lead bytes into a guarded device
    buffer filled with 0xA5; checks the guards and returns the images."""
    nb = x.nbytes
    buf = ch.full((lead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    buf[lead:lead + nb].copy_(_dev(x))
    view = buf[lead:lead + nb].view(TORCH_DTYPES[x.itemsize]).view(x.shape)
    d_boxes = ch.from_numpy(np.ascontiguousarray(boxes, np.int32).reshape(-1)).to(DEV)
    if tab is not None:
        d_tab = _dev(tab).view(TORCH_DTYPES[x.itemsize])
        d_keys = ch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(DEV)
        L.erase_batch(view, d_boxes, d_tab, d_keys, layout)
    else:
        channels = x.shape[3] if layout == 'hwc' else x.shape[1]
        L.erase_batch(view, d_boxes, _dev(np.broadcast_to(value, (channels,))), None, layout)
    got = buf.cpu().numpy()
    assert (got[:lead] == 0xA5).all() and (got[lead + nb:] == 0xA5).all()
    return got[lead:lead + nb].view(x.dtype).reshape(x.shape)


def _host_fill(x, boxes, layout, value, tab, keys):
    got = x.copy()
    channels = x.shape[3] if layout == 'hwc' else x.shape[1]
    fill = tab if tab is not None else np.broadcast_to(value, (channels,)).copy()
    return L.erase_batch_host(got, boxes, fill, keys, layout, nthreads=4)


def _random_boxes(rng, n, H, W):
    y, x = rng.integers(-2, H + 1, n), rng.integers(-2, W + 1, n)
    h, w = rng.integers(0, H + 3, n), rng.integers(0, W + 3, n)
    b = np.stack([y, x, h, w], 1)
    special = [(0, 0, 0, 0), (0, 0, H, W), (-3, -2, H + 5, W + 4), (H, W, 2, 2)]
    for j in range(0, n, 4):
        b[j] = special[(j // 4) % len(special)]
    return b.astype(np.int32)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('itemsize', [1, 2, 4])
def test_fill_shapes_and_forms(itemsize, mode):
    """The CPU test's matrix through the kernel: sizes whose row bytes lie
    around and off multiples of 16, NHWC with 1 and 3 channels and planar,
    batches of 1, 3 and 67 samples; leads cycle through all 16 alignments."""
    rng = np.random.default_rng(31 + itemsize)
    case = 0
    for H, W in C.SIZES:
        for layout, channels in C.FORMS:
            for n in (1, 3, 67):
                if n == 67 and H * W > 64:
                    continue
                x = C.random_images(rng, n, H, W, layout, channels, itemsize)
                boxes = _random_boxes(rng, n, H, W)
                value, tab, noisy = R.fill_case(rng, mode, itemsize, channels)
                keys = rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + 1 if noisy else None
                lead = (case * itemsize) % 16
                case += 1
                got = _device_fill(x, boxes, layout, value, tab, keys, lead)
                assert _same_bytes(got, R.erase(x, boxes, layout, value, tab, keys)), (H, W, layout, channels, n, lead)
                assert _same_bytes(got, _host_fill(x, boxes, layout, value, tab, keys))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('layout,channels', C.FORMS)
def test_fill_hand_made_boxes(layout, channels, mode):
    """Empty, one element, a row minus a column, a column minus a row, boxes
    out of range on every side, and x swept over 0..W-1 at W = 47, so that row
    starts fall at every byte phase; at every alignment of the images."""
    rng = np.random.default_rng(37)
    H, W = 33, 47
    boxes = R.hand_boxes(H, W)
    n = len(boxes)
    for itemsize in (1, 2, 4):
        x = C.random_images(rng, n, H, W, layout, channels, itemsize)
        value, tab, noisy = R.fill_case(rng, mode, itemsize, channels)
        keys = rng.integers(0, 2**63, n, dtype=np.uint64) if noisy else None
        want = R.erase(x, boxes, layout, value, tab, keys)
        assert _same_bytes(_host_fill(x, boxes, layout, value, tab, keys), want)
        for lead in range(0, 16, itemsize):
            assert _same_bytes(_device_fill(x, boxes, layout, value, tab, keys, lead), want), (itemsize, lead)
        if not noisy and itemsize > 1:
            # a constant fill moves bytes: the same images as uint8 pixels of itemsize bytes, at odd leads too
            xb = x.view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * itemsize,)) if layout == 'hwc' else None
            if xb is not None:
                vb = np.broadcast_to(value, (channels,)).copy().view(np.uint8)
                for lead in range(1, 16, 2):
                    got = _device_fill(xb, boxes, 'hwc', vb, None, None, lead)
                    assert _same_bytes(got.view(x.dtype).reshape(x.shape), want), (itemsize, lead)


def test_fill_forms_and_large_launch():
    """The launch takes 8 workgroups per (sample, plane) up to 2048 such pairs
    and 4 beyond: both sides of the threshold through the product entry, and
    the forms tools/erase_bench.py measures (1..16 workgroups, the table staged
    in LDS or read through the cache) on the hand-made boxes."""
    rng = np.random.default_rng(41)
    for n, layout, channels in ((2048, 'hwc', 3), (2049, 'hwc', 3), (683, 'chw', 3)):
        x = C.random_images(rng, n, 5, 6, layout, channels, 2)
        boxes = _random_boxes(rng, n, 5, 6)
        for mode in ('channel', 'noise'):
            value, tab, noisy = R.fill_case(rng, mode, 2, channels)
            keys = rng.integers(0, 2**63, n, dtype=np.uint64) if noisy else None
            got = _device_fill(x, boxes, layout, value, tab, keys, 6)
            assert _same_bytes(got, R.erase(x, boxes, layout, value, tab, keys)), (n, layout, mode)
    H, W = 33, 47
    boxes = R.hand_boxes(H, W)
    n = len(boxes)
    d_boxes = ch.from_numpy(boxes).to(DEV)
    for itemsize in (1, 2, 4):
        x = C.random_images(rng, n, H, W, 'hwc', 3, itemsize)
        _, tab, _ = R.fill_case(rng, 'noise', itemsize, 3)
        keys = rng.integers(0, 2**63, n, dtype=np.uint64)
        want = R.erase(x, boxes, 'hwc', None, tab, keys)
        d_tab = _dev(tab).view(TORCH_DTYPES[itemsize])
        d_keys = ch.from_numpy(keys.view(np.int64)).to(DEV)
        for form in ((1, 1), (2, 1), (4, 1), (16, 1), (100, 1), (1, 0), (4, 0), (8, 0), (16, 0)):
            t = _dev(x).view(TORCH_DTYPES[itemsize]).view(x.shape)
            L.erase_batch(t, d_boxes, d_tab, d_keys, form=form)
            assert _same_bytes(t.cpu().numpy().view(x.dtype), want), (itemsize, form)
        value = np.array([1, 2, 3]).astype(x.dtype)
        for bands in (1, 2, 4, 16, 100):
            t = _dev(x).view(TORCH_DTYPES[itemsize]).view(x.shape)
            L.erase_batch(t, d_boxes, _dev(value), form=(bands, 0))
            assert _same_bytes(t.cpu().numpy().view(x.dtype), R.erase(x, boxes, 'hwc', value)), (itemsize, bands)


@pytest.fixture(scope='module')
def ref_draws():
    return {case: R.draws(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, case[2], R.DEFAULT_RATIO, case[0], case[1])
            for case in R.DRAW_CASES}


@pytest.mark.parametrize('case', R.DRAW_CASES)
def test_draw_launch_equals_reference(ref_draws, case):
    H, W, scale = case
    boxes, keys, _, _ = ref_draws[case]
    n = len(R.DRAW_IDS)
    ids = ch.from_numpy(R.DRAW_IDS.view(np.int64)).to(DEV)
    d_boxes = ch.full((n, 4), -1, dtype=ch.int32, device=DEV)
    d_keys = ch.zeros(n, dtype=ch.int64, device=DEV)
    status = ch.full((n,), -1, dtype=ch.int32, device=DEV)
    L.erase_draw_batch(ids, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, scale, R.DEFAULT_RATIO, H, W, d_boxes, d_keys, status)
    assert np.array_equal(d_boxes.cpu().numpy(), boxes)
    assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), keys)
    assert (status == 0).all()
    host_boxes, host_keys = L.erase_draw_batch_host(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, scale,
                                                    R.DEFAULT_RATIO, H, W)
    assert np.array_equal(host_boxes, boxes) and np.array_equal(host_keys, keys)
    d_boxes.fill_(-1)
    L.erase_draw_batch(ids, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, scale, R.DEFAULT_RATIO, H, W, d_boxes)   # no keys
    assert np.array_equal(d_boxes.cpu().numpy(), boxes)


def test_abi_rejects_bad_arguments():
    lib = L.lib()
    a = ch.full((4, 4, 8, 2), 7, dtype=ch.uint8, device=DEV)
    bx = ch.tensor([[0, 0, 4, 8]] * 4, dtype=ch.int32, device=DEV)
    pat = ch.tensor([1, 1], dtype=ch.uint8, device=DEV)
    tab = ch.from_numpy(noise_table(128, 64, np.uint8)).to(DEV)
    keys = ch.arange(4, dtype=ch.int64, device=DEV)
    ch.cuda.synchronize()

    def call(im=a.data_ptr(), n=4, p=1, h=4, w=8, pb=2, b=bx.data_ptr(), mode=0, isz=1, fill=pat.data_ptr(), k=None):
        return lib.ffcv_erase_batch(None, im, n, p, h, w, pb, b, mode, isz, fill, k)
    noise = dict(mode=1, fill=tab.data_ptr(), k=keys.data_ptr())
    for kw in (dict(im=None), dict(b=None), dict(fill=None), dict(n=0), dict(n=-4), dict(p=0), dict(p=-1), dict(h=0),
               dict(w=0), dict(w=-8), dict(pb=0), dict(pb=65), dict(pb=-2), dict(mode=2), dict(mode=-1),
               dict(h=2**31 - 1, w=2**31 - 1, pb=64), dict(p=2**31 - 1, h=2**31 - 1), dict(n=2**62, h=1024, w=1024),
               dict(n=2**31, h=1, w=1, pb=1), dict(p=65536, h=1, w=1, pb=1),
               dict(noise, k=None), dict(noise, isz=3), dict(noise, isz=8), dict(noise, isz=0),
               dict(noise, isz=4, pb=2), dict(noise, isz=2, pb=3), dict(noise, isz=2, im=a.data_ptr() + 1),
               dict(noise, fill=tab.data_ptr() + 4)):
        assert call(**kw) == -1 and b'ffcv_erase_batch' in lib.ffcv_last_error(), kw
    ids = ch.arange(4, dtype=ch.int64, device=DEV)
    s, r = np.array([0.02, 0.33]), np.array([0.3, 3.3])

    def draw(i=ids.data_ptr(), n=4, p=0.5, sc=s, ra=r, h=32, w=32, b=bx.data_ptr()):
        return lib.ffcv_erase_draw_batch(None, i, n, 7, 1, p, sc.ctypes.data, ra.ctypes.data, h, w, b, None, None)
    for kw in (dict(i=None), dict(b=None), dict(n=-1), dict(p=1.5), dict(p=float('nan')), dict(sc=np.array([0.5, 0.2])),
               dict(sc=np.array([0.1, 1.5])), dict(ra=np.array([0.0, 1.0])), dict(ra=np.array([2.0, 1.0])), dict(h=0),
               dict(w=32768)):
        assert draw(**kw) == -1 and b'ffcv_erase_draw_batch' in lib.ffcv_last_error(), kw
    ch.cuda.synchronize()
    assert (a == 7).all() and (bx.cpu() == ch.tensor([0, 0, 4, 8], dtype=ch.int32)).all()   # nothing was launched
    assert call() == 0
    ch.cuda.synchronize()
    assert (a == 1).all()
    assert call(**noise) == 0
    ch.cuda.synchronize()
    want = R.erase(np.zeros((4, 4, 8, 2), np.uint8), bx.cpu().numpy(), 'hwc', None, noise_table(128, 64, np.uint8),
                   np.arange(4, dtype=np.uint64))
    assert np.array_equal(a.cpu().numpy(), want)


def test_layouts_accepted_and_rejected():
    """The NCHW view of channels-last float16 storage (one plane), contiguous
    CHW float32 with layout='chw' and uint8 HWC are accepted; tensors that are
    not dense or whose samples are not outermost are rejected."""
    rng = np.random.default_rng(3)
    boxes = _random_boxes(rng, 6, 9, 7)
    boxes[1] = (2, 1, 5, 4)
    d_boxes = ch.from_numpy(boxes).to(DEV)
    keys = rng.integers(0, 2**63, 6, dtype=np.uint64)
    d_keys = ch.from_numpy(keys.view(np.int64)).to(DEV)
    f16 = rng.standard_normal((6, 9, 7, 3)).astype(np.float16)
    tab16 = noise_table(0, 1, np.float16)
    nchw = ch.from_numpy(f16).to(DEV).permute(0, 3, 1, 2)
    L.erase_batch(nchw, d_boxes, ch.from_numpy(tab16).to(DEV), d_keys)
    assert _same_bytes(nchw.permute(0, 2, 3, 1).cpu().numpy(), R.erase(f16, boxes, 'hwc', None, tab16, keys))
    f32 = rng.standard_normal((6, 3, 9, 7)).astype(np.float32)
    tab32 = noise_table(0, 1, np.float32)
    planar = ch.from_numpy(f32).to(DEV)
    L.erase_batch(planar, d_boxes, ch.from_numpy(tab32).to(DEV), d_keys, layout='chw')
    assert _same_bytes(planar.cpu().numpy(), R.erase(f32, boxes, 'chw', None, tab32, keys))
    u8 = rng.integers(0, 256, (6, 9, 7, 3), dtype=np.uint8)
    value = np.array([9, 200, 31], np.uint8)
    hwc = ch.from_numpy(u8).to(DEV)
    L.erase_batch(hwc, d_boxes, ch.from_numpy(value).to(DEV))
    assert np.array_equal(hwc.cpu().numpy(), R.erase(u8, boxes, 'hwc', value))
    pat = ch.from_numpy(value).to(DEV)
    for bad in (hwc[:, :, ::2], hwc.permute(1, 0, 2, 3), hwc[:, 1:]):          # not dense, samples not outermost
        with pytest.raises(TypeError):
            L.erase_batch(bad, d_boxes, pat)
    with pytest.raises(TypeError):
        L.erase_batch(nchw, d_boxes, ch.from_numpy(tab16).to(DEV), d_keys, layout='hwc')       # not contiguous
    with pytest.raises(TypeError):
        L.erase_batch(hwc, d_boxes[:5], pat)                                                    # a box short
    with pytest.raises(TypeError):
        L.erase_batch(hwc, d_boxes.long(), pat)
    with pytest.raises(TypeError):
        L.erase_batch(hwc, d_boxes, pat[:2])                                                    # not one pixel
    with pytest.raises(TypeError):
        L.erase_batch(hwc, d_boxes, ch.from_numpy(tab16).to(DEV), d_keys)                       # another itemsize
    with pytest.raises(TypeError):
        L.erase_batch(hwc, d_boxes, pat.cpu())
    assert np.array_equal(hwc.cpu().numpy(), R.erase(u8, boxes, 'hwc', value))


def test_operation_on_device_tensors_outside_a_loader():
    """No context: seed 0, epoch 0, the passed indices.  uint8 NHWC, float16 as
    the NCHW view ToTorchImage hands on, float32 as a contiguous (B, C, H, W)
    with layout='chw'; constants and noise."""
    rng = np.random.default_rng(9)
    idx = np.array([9, 4, 77, 1, 30, 12, 5, 200], np.uint64)
    boxes, keys, _, _ = R.draws(idx, 0, 0, 0.7, R.DEFAULT_SCALE, R.DEFAULT_RATIO, 20, 24)
    assert 0 < (boxes[:, 2] > 0).sum() < 8
    u8 = rng.integers(0, 256, (8, 20, 24, 3), dtype=np.uint8)
    for value, kw in (((3, 250, 17), dict(value=np.array([3, 250, 17], np.uint8))), (9, dict(value=np.uint8(9))),
                      ('pixel', dict(tab=R.table(128, 64, np.uint8), keys=keys))):
        t = ch.from_numpy(u8).to(DEV)
        got = RandomErasing(0.7, value=value, noise=(128, 64)).generate_code()(t, None, idx)
        assert got is t and np.array_equal(t.cpu().numpy(), R.erase(u8, boxes, 'hwc', **kw)), value
    f16 = rng.standard_normal((8, 20, 24, 3)).astype(np.float16)
    for value, kw in (('pixel', dict(tab=R.table(0.0, 1.0, np.float16), keys=keys)),
                      ((0.5, -1.0, 2.0), dict(value=np.array([0.5, -1.0, 2.0], np.float16)))):
        nchw = ch.from_numpy(f16).to(DEV).permute(0, 3, 1, 2)
        got = RandomErasing(0.7, value=value).generate_code()(nchw, None, idx)
        assert tuple(got.shape) == (8, 3, 20, 24) and got.is_contiguous(memory_format=ch.channels_last)
        assert _same_bytes(got.permute(0, 2, 3, 1).cpu().numpy(), R.erase(f16, boxes, 'hwc', **kw)), value
    f32 = rng.standard_normal((8, 3, 20, 24)).astype(np.float32)
    for value, kw in (('pixel', dict(tab=R.table(0.5, 2.0, np.float32), keys=keys)),
                      (-3.25, dict(value=np.float32(-3.25)))):
        planar = ch.from_numpy(f32).to(DEV)
        RandomErasing(0.7, value=value, noise=(0.5, 2.0), layout='chw').generate_code()(planar, None, idx)
        assert _same_bytes(planar.cpu().numpy(), R.erase(f32, boxes, 'chw', **kw)), value
    with pytest.raises(TypeError):
        RandomErasing(0.7, value=(1, 2)).generate_code()(ch.from_numpy(u8).to(DEV), None, idx)
    with pytest.raises(TypeError):
        RandomErasing(0.7).generate_code()(ch.zeros((8, 20, 24, 3), dtype=ch.float64, device=DEV), None, idx)


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


def _case(tmpdir_m, case):
    if case == 'raw32':
        return _beton(tmpdir_m, 'erase_raw.beton', 'raw', 40, (32, 32), 4), SimpleRGBImageDecoder, (32, 32)
    return (_beton(tmpdir_m, 'erase_jpg.beton', 'jpg', 40, (96, 120), 5),
            (lambda: RandomResizedCropRGBImageDecoder((64, 64))), (64, 64))


SEED, P, VALUE, ALPHA = 29, 0.6, (7, 130, 255), 0.5
CONFIGS = ((dict(device_cache=True, batches_per_launch=1), 1, 2), (dict(device_cache=False), 3, 1),
           (dict(batches_per_launch=3), 3, 2), (dict(), 3, 2))           # (Loader arguments, it.G, epochs)


def _cpu_epochs(fn, decoder, epochs=2):
    loader = Loader(fn, batch_size=16, device='cpu', seed=SEED, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5), RandomErasing(P, value=VALUE)], 'label': [IntDecoder()]})
    return [np.concatenate([np.array(im) for im, _ in loader]) for _ in range(epochs)]


def _dev_loader(fn, decoder, before=(), after=(), **kw):
    tail = [ToTensor(), ToDevice(DEV), ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)]
    return Loader(fn, batch_size=16, seed=SEED, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5)] + list(before) + tail + list(after),
        'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)


def _dev_epoch(loader, want_g):
    it = iter(loader)
    assert it.G == want_g
    got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in it])
    assert got.dtype == np.float16 and len(got) == 40
    return got


@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_constant_before_totensor_matches_cpu_loader(tmpdir_m, case):
    """40 samples in batches of 16 (the last one partial), two epochs, a
    per-channel value on uint8 in front of ToTensor: the normalized batch is
    LUT[erased u8] of the CPU Loader."""
    fn, decoder, _ = _case(tmpdir_m, case)
    want = _cpu_epochs(fn, decoder)
    assert not np.array_equal(want[0], want[1])
    for kw, want_g, epochs in CONFIGS:
        loader = _dev_loader(fn, decoder, before=[RandomErasing(P, value=VALUE)], **kw)
        for e in range(epochs):
            got = _dev_epoch(loader, want_g)
            lut = np.stack([LUT[want[e][..., c], c] for c in range(3)], -1)
            bad = [k for k in range(40) if not _same_bytes(got[k], lut[k])]
            assert not bad, (kw, e, bad[:8])


@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_noise_after_normalize_matches_reference(tmpdir_m, case):
    """value='pixel' behind NormalizeImage(float16): the statement applied to
    the float16 batch of the same Loader without the operation."""
    fn, decoder, (H, W) = _case(tmpdir_m, case)
    tab = R.table(0.0, 1.0, np.float16)
    idx = np.arange(40)
    for kw, want_g, epochs in CONFIGS:
        base = _dev_loader(fn, decoder, **kw)
        loader = _dev_loader(fn, decoder, after=[RandomErasing(P, value='pixel')], **kw)
        for e in range(epochs):
            plain, got = _dev_epoch(base, want_g), _dev_epoch(loader, want_g)
            boxes, keys, _, _ = R.draws(idx, SEED, e, P, R.DEFAULT_SCALE, R.DEFAULT_RATIO, H, W)
            assert 5 < (boxes[:, 2] > 0).sum() < 35
            want = R.erase(plain, boxes, 'hwc', None, tab, keys)
            bad = [k for k in range(40) if not _same_bytes(got[k], want[k])]
            assert not bad, (kw, e, bad[:8])


def test_erasing_composes_with_cutmix(tmpdir_m):
    """RandomErasing then ImageCutMix behind NormalizeImage, in the default
    grouping: cutmix of the erased batch, batch by batch."""
    fn, decoder, (H, W) = _case(tmpdir_m, 'raw32')
    tab = R.table(0.0, 1.0, np.float16)
    idx = np.arange(40)
    base = _dev_loader(fn, decoder)
    loader = _dev_loader(fn, decoder, after=[RandomErasing(P, value='pixel'), ImageCutMix(ALPHA, False)])
    for e in range(2):
        plain, got = _dev_epoch(base, 3), _dev_epoch(loader, 3)
        boxes, keys, _, _ = R.draws(idx, SEED, e, P, R.DEFAULT_SCALE, R.DEFAULT_RATIO, H, W)
        want = C.image_cutmix(R.erase(plain, boxes, 'hwc', None, tab, keys), idx, ALPHA, False, batch_size=16)
        assert _same_bytes(got, want), e
