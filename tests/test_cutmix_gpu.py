"""ImageCutMix and the Mixup/CutMix switch on the MI355X: ffcv_cutmix_batch bit
for bit against the numpy statement (tests/cutmix_ref.py) and against the
host twin, with input and output at every byte alignment inside guarded
buffers; the layouts the tensor wrapper takes and rejects; the ABI's
rejections; the operations on device tensors outside a Loader; and device
Loaders (device cache, PCIe staging, launch groups of 3, the default
grouping) against the CPU Loader under one seed, with ImageCutMix before
ToTensor and after NormalizeImage(float16)."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomHorizontalFlip,
                                 MixupToOneHot, ImageCutMix, LabelCutMix, ImageMixupCutMix, LabelMixupCutMix)
from tests.helpers import NaturalDS, write
from tests import cutmix_ref as R
from tests.mixup_ref import SEGMENT_CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49
ALPHA = 0.5
TORCH_DTYPES = {1: ch.uint8, 2: ch.int16, 4: ch.int32, 8: ch.int64}


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_cut(x, boxes, batch_size, same, layout, lead_in, lead_out):
    """ffcv_cutmix_batch on a copy of x placed lead_in bytes into one guarded
    device buffer, into a second one (filled with 0xA5) at lead_out bytes;
    checks the guards of both, that the input is unchanged, and returns the
    output."""
    nb = x.nbytes
    raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    src = ch.full((lead_in + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    dst = ch.full((lead_out + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    tdt = TORCH_DTYPES[x.itemsize]
    sview = src[lead_in:lead_in + nb].view(tdt).view(x.shape)
    dview = dst[lead_out:lead_out + nb].view(tdt).view(x.shape)
    src[lead_in:lead_in + nb].copy_(ch.from_numpy(raw))
    L.cutmix_batch(sview, dview, ch.from_numpy(np.ascontiguousarray(boxes, np.int32).reshape(-1)).to(DEV),
                   batch_size, same, layout)
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    assert (s[:lead_in] == 0xA5).all() and (s[lead_in + nb:] == 0xA5).all()
    assert np.array_equal(s[lead_in:lead_in + nb], raw)                              # the input is not written
    assert (d[:lead_out] == 0xA5).all() and (d[lead_out + nb:] == 0xA5).all()
    return d[lead_out:lead_out + nb].view(x.dtype).reshape(x.shape)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('itemsize', R.ITEMSIZES)
def test_shapes_segments_and_forms(itemsize):
    """The CPU test's matrix through the kernel: sizes whose row bytes lie
    around and off multiples of 16, NHWC with 1 and 3 channels and planar,
    batches of 1, 2, 3, 67 and 10 samples in batches of 4, 10, 16 and 1 (short
    last runs), both box modes; leads cycle through all 16 alignments."""
    rng = np.random.default_rng(17 + itemsize)
    case = 0
    for H, W in R.SIZES:
        for layout, C in R.FORMS:
            for n, bs in SEGMENT_CASES:
                if n == 67 and H * W > 64:
                    continue
                for same in (False, True):
                    x = R.random_images(rng, n, H, W, layout, C, itemsize)
                    boxes = R.random_boxes(rng, -(-n // bs) if same else n, H, W)
                    lead_in, lead_out = (case * itemsize) % 16, ((case * 7 + 5) * itemsize) % 16
                    case += 1
                    got = _device_cut(x, boxes, bs, same, layout, lead_in, lead_out)
                    want = R.from_hwc(R.cut_segments(R.as_hwc(x, layout), boxes, bs, same), layout)
                    assert _same_bytes(got, want), (H, W, layout, C, n, bs, same, lead_in, lead_out)
                    host = L.cutmix_batch_host(x, np.zeros_like(x), boxes, bs, same, layout)
                    assert _same_bytes(got, host)


@pytest.mark.parametrize('layout,C', R.FORMS)
def test_hand_made_boxes(layout, C):
    """Empty, full, corner pixels, a full row and column, boxes out of range
    on every side, and x1 swept over 0..W at W = 47, so that box edges fall at
    every byte phase of a 16-byte piece; at all 16 alignments."""
    rng = np.random.default_rng(23)
    H, W = 33, 47
    boxes = R.hand_boxes(H, W)
    n = len(boxes)
    for itemsize in (1, 2):
        x = R.random_images(rng, n, H, W, layout, C, itemsize)
        want = R.from_hwc(R.cut_segments(R.as_hwc(x, layout), boxes, 5, False), layout)
        host = L.cutmix_batch_host(x, np.zeros_like(x), boxes, 5, False, layout, nthreads=4)
        assert _same_bytes(host, want)
        for lead in range(0, 16, itemsize):
            got = _device_cut(x, boxes, 5, False, layout, lead, (5 * lead + 3 * itemsize) % 16)
            assert _same_bytes(got, want), (itemsize, lead)
    x = R.random_images(rng, 6, H, W, layout, C, 1)
    for b in boxes[:12]:
        got = _device_cut(x, np.stack([b, b]), 4, True, layout, 3, 9)
        assert _same_bytes(got, R.from_hwc(R.cut_segments(R.as_hwc(x, layout), np.stack([b, b]), 4, True), layout))


def test_layouts_accepted_and_rejected():
    """An NCHW view of channels-last storage is accepted (one plane), as are
    float16 and bfloat16; the layouts test_mixup_gpu rejects are rejected."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (6, 9, 7, 3), dtype=np.uint8)
    boxes = R.random_boxes(rng, 6, 9, 7)
    boxes[1] = (2, 1, 7, 5)
    d_boxes = ch.from_numpy(boxes).to(DEV)
    want = R.cut_segments(x, boxes, 6, False)
    nchw = ch.from_numpy(x).to(DEV).permute(0, 3, 1, 2)
    out = ch.zeros((6, 9, 7, 3), dtype=ch.uint8, device=DEV).permute(0, 3, 1, 2)
    L.cutmix_batch(nchw, out, d_boxes, 6, False)
    assert np.array_equal(out.permute(0, 2, 3, 1).cpu().numpy(), want)
    for dt in (ch.float16, ch.bfloat16, ch.float32):
        f = ch.from_numpy(x.astype(np.float32)).to(DEV).to(dt).permute(0, 3, 1, 2)
        o = ch.zeros((6, 9, 7, 3), dtype=dt, device=DEV).permute(0, 3, 1, 2)
        L.cutmix_batch(f, o, d_boxes, 6, False)
        assert np.array_equal(o.permute(0, 2, 3, 1).float().cpu().numpy(), want.astype(np.float32)), dt
    planar = nchw.contiguous()
    o = ch.zeros_like(planar)
    L.cutmix_batch(planar, o, d_boxes, 6, False, layout='chw')
    assert np.array_equal(o.permute(0, 2, 3, 1).cpu().numpy(), want)
    for bad_in, bad_out in ((nchw, ch.zeros((6, 3, 9, 7), dtype=ch.uint8, device=DEV)),      # laid out differently
                            (nchw[:, :, ::2], out[:, :, ::2]),                                # not dense
                            (nchw.permute(1, 0, 2, 3), out.permute(1, 0, 2, 3)),              # samples not outermost
                            (nchw, out.half())):                                              # two dtypes
        with pytest.raises(TypeError):
            L.cutmix_batch(bad_in, bad_out, d_boxes, 6, False)
    with pytest.raises(TypeError):
        L.cutmix_batch(nchw, out, d_boxes, 6, False, layout='hwc')                            # not contiguous
    with pytest.raises(TypeError):
        L.cutmix_batch(nchw, out, d_boxes[:5], 6, False)                                      # a box short
    with pytest.raises(TypeError):
        L.cutmix_batch(nchw, out, d_boxes.long(), 6, False)


def test_abi_rejects_bad_arguments():
    lib = L.lib()
    a = ch.full((4, 4, 8, 2), 1, dtype=ch.uint8, device=DEV)
    o = ch.full((4, 4, 8, 2), 77, dtype=ch.uint8, device=DEV)
    bx = ch.tensor([[0, 0, 4, 8]] * 4, dtype=ch.int32, device=DEV)
    ch.cuda.synchronize()

    def call(inp=a.data_ptr(), out=o.data_ptr(), n=4, p=1, h=4, w=8, pb=2, bs=4, b=bx.data_ptr()):
        return lib.ffcv_cutmix_batch(None, inp, out, n, p, h, w, pb, bs, b, 0)
    for kw in (dict(inp=None), dict(out=None), dict(b=None), dict(n=0), dict(n=-4), dict(p=0), dict(p=-1), dict(h=0),
               dict(w=0), dict(w=-8), dict(bs=0), dict(bs=-2), dict(pb=0), dict(pb=65), dict(pb=-2),
               dict(h=2**31 - 1, w=2**31 - 1, pb=64), dict(p=2**31 - 1, h=2**31 - 1), dict(n=2**62, h=1024, w=1024),
               dict(inp=o.data_ptr()), dict(inp=o.data_ptr() + 255), dict(inp=o.data_ptr() - 255)):
        assert call(**kw) == -1 and b'ffcv_cutmix_batch' in lib.ffcv_last_error(), kw
    ch.cuda.synchronize()
    assert (o == 77).all() and (a == 1).all()                       # nothing was launched
    assert call() == 0
    ch.cuda.synchronize()
    assert (o == 1).all()


def test_image_ops_on_device_tensors_outside_a_loader():
    """No context: the whole input is one batch drawn from its last index.
    uint8 NHWC, float16 as the NCHW view ToTorchImage hands on, float32 as a
    contiguous (B, C, H, W) with layout='chw'; and the switch on uint8 and
    float32."""
    rng = np.random.default_rng(9)
    idx = np.array([9, 4, 77, 1, 30, 12, 5], np.uint64)
    for same in (False, True):
        u8 = rng.integers(0, 256, (7, 9, 11, 3), dtype=np.uint8)
        got = ImageCutMix(0.2, same).generate_code()(ch.from_numpy(u8).to(DEV),
                                                     ch.zeros((9, 9, 11, 3), dtype=ch.uint8, device=DEV), idx)
        assert np.array_equal(got.cpu().numpy(), R.image_cutmix(u8, idx, 0.2, same))
        f16 = (rng.standard_normal((7, 9, 11, 3)) * 50).astype(np.float16)
        nchw = ch.from_numpy(f16).to(DEV).permute(0, 3, 1, 2)
        got = ImageCutMix(2.0, same).generate_code()(nchw, ch.zeros((9, 3, 9, 11), dtype=ch.float16, device=DEV), idx)
        assert tuple(got.shape) == (7, 3, 9, 11) and got.is_contiguous(memory_format=ch.channels_last)
        want = R.image_cutmix(f16, idx, 2.0, same)
        assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy().view(np.uint16), want.view(np.uint16))
        f32 = (rng.standard_normal((7, 9, 11, 3)) * 50).astype(np.float32)
        planar = ch.from_numpy(f32).to(DEV).permute(0, 3, 1, 2).contiguous()
        got = ImageCutMix(1.0, same, layout='chw').generate_code()(planar, ch.zeros((9, 3, 9, 11), device=DEV), idx)
        assert got.is_contiguous()
        want = R.image_cutmix(f32, idx, 1.0, same)
        assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), want.view(np.uint32))
        picks = []
        for last in range(100, 108):
            sidx = np.arange(last - 6, last + 1, dtype=np.uint64)
            for x in (u8, f32):
                want, _, cut = R.switch_batch(x, np.zeros(7), last, 0.4, 1.0, 0.5, same)
                got = ImageMixupCutMix(0.4, 1.0, 0.5, same).generate_code()(
                    ch.from_numpy(x).to(DEV), ch.zeros((9, 9, 11, 3), dtype=ch.from_numpy(x[:0]).dtype, device=DEV),
                    sidx)
                assert _same_bytes(got.cpu().numpy(), want), (last, x.dtype)
            picks.append(cut)
        assert any(picks) and not all(picks)


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


def _ops(kind, same, size):
    if kind == 'cutmix':
        return ImageCutMix(ALPHA, same), LabelCutMix(ALPHA, same, size)
    return ImageMixupCutMix(ALPHA, 1.0, 0.5, same), LabelMixupCutMix(ALPHA, 1.0, 0.5, same, size)


def _cpu_epochs(fn, decoder, seed, kind, same, size, epochs=2):
    image_op, label_op = _ops(kind, same, size)
    loader = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5), image_op],
        'label': [IntDecoder(), label_op, ToTensor(), MixupToOneHot(10)]})
    out = []
    for _ in range(epochs):
        batches = [(np.array(im), lab.numpy().copy()) for im, lab in loader]
        out.append((np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])))
    return out


def _dev_loader(fn, decoder, seed, kind, same, size, after_normalize, **kw):
    image_op, label_op = _ops(kind, same, size)
    tail = [ToTensor(), ToDevice(DEV), ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)]
    image = [decoder(), RandomHorizontalFlip(0.5)] + (tail + [image_op] if after_normalize else [image_op] + tail)
    return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
        'image': image, 'label': [IntDecoder(), label_op, ToTensor(), ToDevice(DEV), MixupToOneHot(10)]}, **kw)


def _check_device_loader(loader, want_epochs, n, want_g):
    for want_u8, want_lab in want_epochs:
        it = iter(loader)
        assert it.G == want_g
        batches = [(im.permute(0, 2, 3, 1).cpu().numpy(), lab.cpu().numpy()) for im, lab in it]
        got = np.concatenate([b[0] for b in batches])
        lab = np.concatenate([b[1] for b in batches])
        assert got.dtype == np.float16 and got.shape == want_u8.shape and len(got) == n
        want = np.stack([LUT[want_u8[..., c], c] for c in range(3)], -1)
        bad = [k for k in range(n) if not np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16))]
        assert not bad, bad[:8]
        assert lab.dtype == np.float32 and np.array_equal(lab, want_lab)


def _case(tmpdir_m, case):
    if case == 'raw32':
        return _beton(tmpdir_m, 'cut_raw.beton', 'raw', 40, (32, 32), 4), SimpleRGBImageDecoder, (32, 32)
    return (_beton(tmpdir_m, 'cut_jpg.beton', 'jpg', 40, (96, 120), 5),
            (lambda: RandomResizedCropRGBImageDecoder((64, 64))), (64, 64))


def _loader_matrix(fn, decoder, seed, kind, same, size, after_normalize, want):
    args = (fn, decoder, seed, kind, same, size, after_normalize)
    _check_device_loader(_dev_loader(*args, device_cache=True, batches_per_launch=1), want, 40, 1)
    _check_device_loader(_dev_loader(*args, device_cache=False), want[:1], 40, 3)
    _check_device_loader(_dev_loader(*args, batches_per_launch=3), want, 40, 3)
    _check_device_loader(_dev_loader(*args), want, 40, 3)                      # the default keeps the group


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_cutmix_device_loader_matches_cpu_loader(tmpdir_m, case, same):
    """40 samples in batches of 16 (the last one partial), two epochs, with
    ImageCutMix before ToTensor and AFTER NormalizeImage(float16): both equal
    LUT[cutmix(u8)] bit for bit, CutMix being a select."""
    fn, decoder, size = _case(tmpdir_m, case)
    seed = 29
    want = _cpu_epochs(fn, decoder, seed, 'cutmix', same, size)
    assert not np.array_equal(want[0][0], want[1][0])
    for after_normalize in (False, True):
        _loader_matrix(fn, decoder, seed, 'cutmix', same, size, after_normalize, want)


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_switch_device_loader_matches_cpu_loader(tmpdir_m, case, same):
    """The same Loader matrix for the switch pair at switch_prob 0.5, with
    soft labels through MixupToOneHot(10)."""
    fn, decoder, size = _case(tmpdir_m, case)
    seed = 29
    want = _cpu_epochs(fn, decoder, seed, 'switch', same, size)
    _loader_matrix(fn, decoder, seed, 'switch', same, size, False, want)
