"""ImageMixup / MixupToOneHot on the MI355X: ffcv_mixup_batch bit for bit
against numpy's float64 statement (tests/mixup_ref.py) and against the host
twin, with the images at every byte alignment inside guarded buffers; the
ABI's rejections; ffcv_mixup_onehot_batch against the host operation; and
device Loaders (device cache, PCIe staging, launch groups of 3, the default
grouping) against the CPU Loader under one seed."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import DecodeError
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomHorizontalFlip,
                                 ImageMixup, LabelMixup, MixupToOneHot)
from tests.helpers import NaturalDS, write
from tests import mixup_ref as R

SEGMENT_CASES, ELEMS, _inputs, _lams = R.SEGMENT_CASES, R.ELEMS, R.random_inputs, R.random_lambdas

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49
ALPHA = 0.5


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_mix(imgs, lam, batch_size, same, lead_in, lead_out):
    """ffcv_mixup_batch on a copy of imgs placed lead_in bytes into one guarded
    device buffer, into a second one (filled with 0xA5) at lead_out bytes;
    checks the guards of both and returns the output."""
    nb = imgs.nbytes
    src = ch.full((lead_in + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    dst = ch.full((lead_out + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    tdt = ch.from_numpy(imgs[:0]).dtype
    sview = src[lead_in:lead_in + nb].view(tdt).view(imgs.shape)
    dview = dst[lead_out:lead_out + nb].view(tdt).view(imgs.shape)
    sview.copy_(ch.from_numpy(imgs))
    L.mixup_batch(sview, dview, ch.from_numpy(np.ascontiguousarray(lam, np.float64)).to(DEV), batch_size, same)
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    assert (s[:lead_in] == 0xA5).all() and (s[lead_in + nb:] == 0xA5).all()
    assert np.array_equal(s[lead_in:lead_in + nb], imgs.reshape(-1).view(np.uint8))      # the input is not written
    assert (d[:lead_out] == 0xA5).all() and (d[lead_out + nb:] == 0xA5).all()
    return d[lead_out:lead_out + nb].view(imgs.dtype).reshape(imgs.shape)


def test_all_pairs_at_every_alignment():
    """Every (a, b) byte pair under the fixed lambdas and 16 beta draws (25
    batches of the two all-pairs samples, one lambda per batch), with the
    input at each of the 16 byte alignments and the output at another."""
    pairs = R.all_pairs()
    lams = R.all_pairs_lambdas()
    imgs = np.concatenate([pairs] * len(lams))
    want = R.mix_segments(imgs, lams, 2, True)
    host = L.mixup_batch_host(imgs, np.zeros_like(imgs), lams, 2, True, nthreads=4)
    assert np.array_equal(host, want)
    for lead in range(16):
        got = _device_mix(imgs, lams, 2, True, lead, (5 * lead + 3) % 16)
        assert np.array_equal(got, want), lead


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_shapes_and_segments(dtype):
    """Batches of 1, 2, 3, 67; 10 samples in batches of 4 (4, 4, 2), 10, 16
    and 1; sample sizes around one workgroup's 4,096 bytes and tiny ones; both
    same_lambda values; float32 by bit pattern.  Runs of 8 samples: 67 and 10
    leave short last runs."""
    rng = np.random.default_rng(11)
    step = 1 if dtype == np.uint8 else 4
    case = 0
    for elems in ELEMS:
        for n, bs in SEGMENT_CASES:
            if n == 67 and elems > 3072:
                continue
            for same in (False, True):
                imgs = _inputs(rng, n, elems, dtype)
                lam = _lams(rng, n, bs, same)
                lead_in, lead_out = (case * step) % 16, ((case * 7 + 5) * step) % 16
                case += 1
                got = _device_mix(imgs, lam, bs, same, lead_in, lead_out)
                with np.errstate(over='ignore', invalid='ignore'):
                    want = R.mix_segments(imgs, lam, bs, same)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (elems, n, bs, same, lead_in)
                host = L.mixup_batch_host(imgs, np.zeros_like(imgs), lam, bs, same)
                assert np.array_equal(got.view(np.uint8), host.view(np.uint8))


def test_every_run_length_and_channels_last():
    """The diagnostic run lengths compute the same bytes; an NCHW view of
    channels-last storage is accepted, other layouts are not."""
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (21, 5000), dtype=np.uint8)
    lam = rng.beta(0.5, 0.5, 21)
    want = R.mix_segments(imgs, lam, 8, False)
    d_in, d_lam = ch.from_numpy(imgs).to(DEV), ch.from_numpy(lam).to(DEV)
    for run in (1, 2, 4, 8):
        out = ch.zeros_like(d_in)
        L.mixup_batch(d_in, out, d_lam, 8, False, run=run)
        assert np.array_equal(out.cpu().numpy(), want), run
    with pytest.raises(L.FFCVError, match='run length'):
        L.mixup_batch(d_in, ch.zeros_like(d_in), d_lam, 8, False, run=3)
    x = rng.integers(0, 256, (6, 9, 7, 3), dtype=np.uint8)
    lam6 = rng.beta(0.5, 0.5, 6)
    nchw = ch.from_numpy(x).to(DEV).permute(0, 3, 1, 2)
    out = ch.zeros((6, 9, 7, 3), dtype=ch.uint8, device=DEV).permute(0, 3, 1, 2)
    L.mixup_batch(nchw, out, ch.from_numpy(lam6).to(DEV), 6, False)
    assert np.array_equal(out.permute(0, 2, 3, 1).cpu().numpy(), R.mix_segments(x, lam6, 6, False))
    for bad_in, bad_out in ((nchw, ch.zeros((6, 3, 9, 7), dtype=ch.uint8, device=DEV)),      # laid out differently
                            (nchw[:, :, ::2], out[:, :, ::2]),                                # not dense
                            (nchw.permute(1, 0, 2, 3), out.permute(1, 0, 2, 3)),              # samples not outermost
                            (nchw.half(), out.half())):
        with pytest.raises(TypeError):
            L.mixup_batch(bad_in, bad_out, ch.from_numpy(lam6).to(DEV), 6, False)


def test_abi_rejects_bad_arguments():
    lib = L.lib()
    a = ch.full((4, 64), 1, dtype=ch.uint8, device=DEV)
    o = ch.full((4, 64), 77, dtype=ch.uint8, device=DEV)
    lam = ch.full((4,), 0.5, dtype=ch.float64, device=DEV)
    ch.cuda.synchronize()

    def call(inp=a.data_ptr(), out=o.data_ptr(), n=4, e=64, dt=L.MIXUP_U8, bs=4, lm=lam.data_ptr()):
        return lib.ffcv_mixup_batch(None, inp, out, n, e, dt, bs, lm, 0)
    for kw in (dict(inp=None), dict(out=None), dict(lm=None), dict(n=0), dict(n=-4), dict(e=0), dict(e=-1), dict(bs=0),
               dict(bs=-2), dict(dt=0), dict(dt=3), dict(inp=o.data_ptr()), dict(inp=o.data_ptr() + 255),
               dict(inp=o.data_ptr() - 255), dict(dt=L.MIXUP_F32, e=16, inp=a.data_ptr() + 2)):
        assert call(**kw) == -1 and b'ffcv_mixup_batch' in lib.ffcv_last_error(), kw
    ch.cuda.synchronize()
    assert (o == 77).all() and (a == 1).all()                       # nothing was launched
    assert call() == 0
    ch.cuda.synchronize()
    assert (o == 1).all()
    st = ch.zeros((4,), dtype=ch.int32, device=DEV)
    l3 = ch.zeros((4, 3), dtype=ch.float32, device=DEV)
    oh = ch.full((4, 10), 5.0, dtype=ch.float32, device=DEV)
    for args in ((None, oh.data_ptr(), 4, 10, st.data_ptr()), (l3.data_ptr(), None, 4, 10, st.data_ptr()),
                 (l3.data_ptr(), oh.data_ptr(), 4, 10, None), (l3.data_ptr(), oh.data_ptr(), 0, 10, st.data_ptr()),
                 (l3.data_ptr(), oh.data_ptr(), 4, 0, st.data_ptr())):
        assert lib.ffcv_mixup_onehot_batch(None, *args) == -1 and b'ffcv_mixup_onehot_batch' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert (oh == 5.0).all()


@pytest.mark.parametrize('n', [1, 67])
@pytest.mark.parametrize('classes', [2, 10, 1000])
def test_onehot_matches_host_op(n, classes):
    rng = np.random.default_rng(n * classes)
    l3 = np.empty((n, 3), np.float32)
    l3[:, 0] = rng.integers(0, classes, n)
    l3[:, 1] = rng.integers(0, classes, n)
    l3[:, 2] = rng.beta(0.5, 0.5, n)
    l3[::5, 1] = l3[::5, 0]                                          # a == b: the row sums to 1 - lam
    l3[-1, :2] = classes - 1
    host = MixupToOneHot(classes).generate_code()(ch.from_numpy(l3.copy()), ch.zeros((n, classes)))
    assert np.array_equal(host.numpy(), R.one_hot(l3, classes))
    bad_row = n // 2
    d3 = l3.copy()
    d3[bad_row, rng.integers(0, 2)] = (classes, -1, classes + 7)[n % 3]
    d_l3 = ch.from_numpy(d3).to(DEV)
    out = ch.full((n, classes), 9.0, dtype=ch.float32, device=DEV)
    status = ch.full((n,), -1, dtype=ch.int32, device=DEV)
    L.mixup_onehot_batch(d_l3, out, status)
    want = host.numpy().copy()
    want[bad_row] = 0
    want_status = np.zeros(n, np.int32)
    want_status[bad_row] = 7
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(status.cpu().numpy(), want_status)
    assert np.array_equal(d_l3.cpu().numpy(), d3)                    # the input is not changed
    # the operation outside a Loader reports it at once
    with pytest.raises(IndexError, match=f'row {bad_row}'):
        MixupToOneHot(classes).generate_code()(d_l3, ch.zeros((n, classes), device=DEV))


def test_image_op_on_device_tensors_outside_a_loader():
    """No context: the whole input is one batch drawn from its last index.
    uint8 NHWC, and float32 as the NCHW view ToTorchImage hands on."""
    rng = np.random.default_rng(9)
    idx = np.array([9, 4, 77, 1, 30, 12, 5], np.uint64)
    for same in (False, True):
        u8 = rng.integers(0, 256, (7, 5, 6, 3), dtype=np.uint8)
        got = ImageMixup(0.2, same).generate_code()(ch.from_numpy(u8).to(DEV), ch.zeros((9, 5, 6, 3), dtype=ch.uint8,
                                                                                         device=DEV), idx)
        assert np.array_equal(got.cpu().numpy(), R.image_mixup(u8, idx, 0.2, same))
        f32 = (rng.standard_normal((7, 5, 6, 3)) * 50).astype(np.float32)
        nchw = ch.from_numpy(f32).to(DEV).permute(0, 3, 1, 2)
        got = ImageMixup(2.0, same).generate_code()(nchw, ch.zeros((9, 3, 5, 6), device=DEV), idx)
        assert tuple(got.shape) == (7, 3, 5, 6) and got.is_contiguous(memory_format=ch.channels_last)
        want = R.image_mixup(f32, idx, 2.0, same)
        assert np.array_equal(got.permute(0, 2, 3, 1).cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


def _cpu_epochs(fn, decoder, seed, same, epochs=2):
    loader = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5), ImageMixup(ALPHA, same)],
        'label': [IntDecoder(), LabelMixup(ALPHA, same), ToTensor(), MixupToOneHot(10)]})
    out = []
    for _ in range(epochs):
        batches = [(np.array(im), lab.numpy().copy()) for im, lab in loader]
        out.append((np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])))
    return out


def _dev_loader(fn, decoder, seed, same, **kw):
    return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomHorizontalFlip(0.5), ImageMixup(ALPHA, same), ToTensor(), ToDevice(DEV),
                  ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)],
        'label': [IntDecoder(), LabelMixup(ALPHA, same), ToTensor(), ToDevice(DEV), MixupToOneHot(10)]}, **kw)


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


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case, same):
    """40 samples in batches of 16 (the last one partial), two epochs: the
    lambdas repeat per batch index, the images differ through the flips."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'mix_raw.beton', 'raw', 40, (32, 32), 4)
        decoder = SimpleRGBImageDecoder
    else:
        fn = _beton(tmpdir_m, 'mix_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = (lambda: RandomResizedCropRGBImageDecoder((64, 64)))
    seed = 29
    want = _cpu_epochs(fn, decoder, seed, same)
    assert not np.array_equal(want[0][0], want[1][0])
    _check_device_loader(_dev_loader(fn, decoder, seed, same, device_cache=True, batches_per_launch=1), want, 40, 1)
    _check_device_loader(_dev_loader(fn, decoder, seed, same, device_cache=False), want[:1], 40, 3)
    _check_device_loader(_dev_loader(fn, decoder, seed, same, batches_per_launch=3), want, 40, 3)
    _check_device_loader(_dev_loader(fn, decoder, seed, same), want, 40, 3)    # the default keeps the group


def test_device_loader_reports_out_of_range_label(tmpdir_m):
    fn = _beton(tmpdir_m, 'mix_raw.beton', 'raw', 40, (32, 32), 4)            # labels 0..9
    loader = Loader(fn, batch_size=16, seed=1, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder(), ToTensor(), ToDevice(DEV)],
        'label': [IntDecoder(), LabelMixup(ALPHA, True), ToTensor(), ToDevice(DEV), MixupToOneHot(9)]})
    with pytest.raises(DecodeError, match=r'MixupToOneHot: sample 9 .*label outside'):
        for _ in loader:
            pass
