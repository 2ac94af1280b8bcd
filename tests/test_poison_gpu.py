"""Poison / ReplaceLabel on the MI355X: ffcv_poison_batch bit for bit against
numpy's statements on a float32 temp (tests/poison_ref.py) and against the
host twin, with the images at every byte alignment inside guarded buffers;
every diagnostic kernel form; the layouts and ABI arguments it rejects;
ffcv_replace_label_batch against the host operation; and device Loaders
(device cache, PCIe staging, launch groups of 3, the default grouping) against
the CPU Loader under one seed."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, RandomHorizontalFlip, Poison,
                                 ReplaceLabel)
from tests.helpers import NaturalDS, write
from tests import poison_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
LUT = ((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)   # normalize.py:42-49
SPAN = 256 * 8            # bytes of a sample one workgroup covers
FORMS = [(b, r, o) for b in (4, 8, 16) for r in (1, 3, 8, 16, 64) for o in (0, 1)]


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _tables(mask, alpha):
    a3 = R.alpha3_of(alpha)
    return np.asarray(1 - a3, np.float64), np.asarray(mask.astype(float) * a3, np.float64)


def _dev(a):
    return ch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _device_poison(images, sample_ids, indices, d_keep, d_add, clamp=(0, 255), lead=0, form=None):
    """ffcv_poison_batch on a copy of images placed `lead` bytes into a device
    buffer filled with 0xA5; checks the guards and returns the result."""
    nb = images.nbytes
    buf = ch.full((lead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    view = buf[lead:lead + nb].view(images.shape)
    view.copy_(ch.from_numpy(images))
    ids = _dev(np.unique(np.asarray(indices, np.uint64)).astype(np.int64))
    L.poison_batch(view, _dev(np.asarray(sample_ids).astype(np.int64)), ids, d_keep, d_add, clamp, form=form)
    out = buf.cpu().numpy()
    assert (out[:lead] == 0xA5).all() and (out[lead + nb:] == 0xA5).all()
    return out[lead:lead + nb].reshape(images.shape)


@pytest.mark.parametrize('alpha_dtype', [np.float64, np.float32])
def test_all_pairs_at_every_alignment(alpha_dtype):
    """Every (v, m) byte pair under every opacity, with the images at each of
    the 16 byte alignments.  Three samples, the middle one not poisoned."""
    image, mask, alpha = R.all_pairs(alpha_dtype)
    images = np.concatenate([image, image, image])
    sids, indices = [4, 9, 6], [6, 4]
    want = R.poison_np(images, mask, alpha, sids, indices)
    keep, add = _tables(mask, alpha)
    host = L.poison_batch_host(images.copy(), sids, np.array([4, 6], np.uint64), keep, add, nthreads=4)
    assert np.array_equal(host, want) and np.array_equal(want[1], images[1]) and not np.array_equal(want[0], images[0])
    d_keep, d_add = _dev(keep), _dev(add)
    for lead in range(16):
        got = _device_poison(images, sids, indices, d_keep, d_add, lead=lead)
        assert np.array_equal(got, want), lead


# sample sizes just below and just above one workgroup's span, and past two
GPU_SHAPES = R.SHAPES + [(2, 341, 3), (1, 683, 3), (3, 455, 3)]
assert 2 * 341 * 3 == SPAN - 2 and 683 * 3 == SPAN + 1 and 3 * 455 * 3 == 2 * SPAN - 1


@pytest.mark.parametrize('alpha_dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', GPU_SHAPES)
def test_shapes_batches_index_sets(shape, alpha_dtype):
    """The CPU list's shapes, batch sizes (launches this small go in runs of 8,
    so 67 leaves a short last run of 3), index sets and clamps; guards
    checked, unpoisoned samples untouched."""
    rng = np.random.default_rng(sum(shape) + 1)
    case = 0
    for n in R.BATCHES:
        images, mask, alpha, sids = R.random_case(rng, shape, n, alpha_dtype)
        keep, add = _tables(mask, alpha)
        d_keep, d_add = _dev(keep), _dev(add)
        for kind in R.INDEX_SETS:
            indices = R.index_set(kind, sids)
            clamp = R.CLAMPS[case % len(R.CLAMPS)]
            lead = (5 * case + 1) % 16
            case += 1
            want = R.poison_np(images, mask, alpha, sids, indices, clamp)
            got = _device_poison(images, sids, indices, d_keep, d_add, clamp, lead)
            assert np.array_equal(got, want), (shape, n, kind, clamp, lead)
            ids = np.unique(np.asarray(indices, np.uint64))
            assert np.array_equal(got, L.poison_batch_host(images.copy(), sids, ids, keep, add, clamp))
            hit = R.chosen(sids, indices)
            assert all(np.array_equal(got[k], images[k]) for k in range(n) if k not in hit)


def test_every_form_and_layouts():
    """Every diagnostic (bytes per thread, run length, workgroup order)
    computes the same bytes; an NCHW view and other non-dense layouts are rejected."""
    rng = np.random.default_rng(3)
    images, mask, alpha, sids = R.random_case(rng, (29, 47, 3), 71, np.float32)       # 4,089 B: two spans, a tail
    indices = R.index_set('every_other', sids)
    want = R.poison_np(images, mask, alpha, sids, indices, (2, 251))
    keep, add = _tables(mask, alpha)
    d_keep, d_add = _dev(keep), _dev(add)
    for form in FORMS:
        got = _device_poison(images, sids, indices, d_keep, d_add, (2, 251), lead=(form[0] + form[1]) % 16, form=form)
        assert np.array_equal(got, want), form
    d_im = _dev(images)
    d_sid, d_ids = _dev(sids.astype(np.int64)), _dev(np.array(sorted(indices), np.int64))
    for form in ((3, 4, 0), (12, 8, 1), (8, 0, 0), (8, 65, 0), (8, -1, 1)):
        with pytest.raises(L.FFCVError, match='ffcv_poison_batch_form'):
            L.poison_batch(d_im, d_sid, d_ids, d_keep, d_add, form=form)
    for bad in (d_im.permute(0, 3, 1, 2), d_im[:, :, ::2], d_im.permute(1, 0, 2, 3), d_im.half(), d_im.cpu()):
        with pytest.raises(TypeError):
            L.poison_batch(bad, d_sid, d_ids, d_keep, d_add)
    for args in ((d_sid[:-1], d_ids, d_keep, d_add), (d_sid.int(), d_ids, d_keep, d_add),
                 (d_sid, d_ids.double(), d_keep, d_add), (d_sid, d_ids, d_keep.float(), d_add),
                 (d_sid, d_ids, d_keep, d_add.reshape(-1)[:-1]), (d_sid.cpu(), d_ids, d_keep, d_add)):
        with pytest.raises(TypeError):
            L.poison_batch(d_im, *args)
    ch.cuda.synchronize()
    assert np.array_equal(d_im.cpu().numpy(), images)                 # nothing was launched


def test_abi_rejects_bad_arguments():
    lib = L.lib()
    a = ch.full((4, 24), 7, dtype=ch.uint8, device=DEV)
    lab = ch.full((4, 1), 5, dtype=ch.int64, device=DEV)
    sid = ch.arange(4, dtype=ch.int64, device=DEV)
    pid = ch.tensor([1, 2], dtype=ch.int64, device=DEV)
    keep = ch.full((24,), 0.5, dtype=ch.float64, device=DEV)
    add = ch.full((24,), 3.0, dtype=ch.float64, device=DEV)
    ch.cuda.synchronize()

    def call(im=a.data_ptr(), n=4, e=24, s=sid.data_ptr(), p=pid.data_ptr(), npo=2, k=keep.data_ptr(),
             ad=add.data_ptr(), lo=0.0, hi=255.0):
        return lib.ffcv_poison_batch(None, im, n, e, s, p, npo, k, ad, lo, hi)
    for kw in (dict(im=None), dict(s=None), dict(p=None), dict(k=None), dict(ad=None), dict(n=0), dict(n=-1),
               dict(e=0), dict(e=-3), dict(npo=-1), dict(n=1 << 40, e=1 << 40), dict(n=1 << 40, e=1),
               dict(k=keep.data_ptr() + 4), dict(ad=add.data_ptr() + 1), dict(s=sid.data_ptr() + 4),
               dict(p=pid.data_ptr() + 2), dict(lo=-1.0), dict(hi=256.0), dict(lo=9.0, hi=8.0), dict(lo=float('nan'))):
        assert call(**kw) == -1 and b'ffcv_poison_batch' in lib.ffcv_last_error(), kw

    def relabel(lb=lab.data_ptr(), n=4, row=1, s=sid.data_ptr(), p=pid.data_ptr(), npo=2):
        return lib.ffcv_replace_label_batch(None, lb, n, row, s, p, npo, 9)
    for kw in (dict(lb=None), dict(s=None), dict(p=None), dict(n=0), dict(row=0), dict(npo=-2), dict(lb=lab.data_ptr() + 4),
               dict(s=sid.data_ptr() + 1), dict(n=1 << 61, row=8)):
        assert relabel(**kw) == -1 and b'ffcv_replace_label_batch' in lib.ffcv_last_error(), kw
    assert call(npo=0) == 0 and call(npo=0, p=None) == 0 and relabel(npo=0) == 0      # an empty set: no launch
    ch.cuda.synchronize()
    assert (a == 7).all() and (lab == 5).all()                          # nothing was launched
    assert call() == 0 and relabel() == 0
    ch.cuda.synchronize()
    assert (a[[1, 2]] == 6).all() and (a[[0, 3]] == 7).all()            # float32(7 * 0.5) + 3 = 6.5 -> 6
    assert lab.reshape(-1).tolist() == [5, 9, 9, 5]


@pytest.mark.parametrize('column', [False, True])
@pytest.mark.parametrize('n', [1, 67, 300])
def test_replace_label_matches_host_op(n, column):
    rng = np.random.default_rng(n)
    sids = rng.permutation(4 * n + 8)[:n].astype(np.uint64) + np.uint64(3)
    labels = rng.integers(0, 10, (n, 1) if column else (n,)).astype(np.int64)
    for kind in R.INDEX_SETS:
        indices = R.index_set(kind, sids)
        want = ReplaceLabel(indices, 42).generate_code()(labels.copy(), None, sids)
        assert np.array_equal(want, R.replace_label_np(labels, sids, indices, 42))
        buf = ch.full((n + 2,) + labels.shape[1:], -7, dtype=ch.int64, device=DEV)
        buf[1:n + 1].copy_(ch.from_numpy(labels))
        # the operation outside a Loader uploads the passed indices itself
        got = ReplaceLabel(indices, 42).generate_code()(buf[1:n + 1], None, sids)
        out = buf.cpu().numpy()
        assert got.data_ptr() == buf[1:].data_ptr() and np.array_equal(out[1:n + 1], want), (n, kind)
        assert (out[0] == -7).all() and (out[-1] == -7).all()


def test_poison_op_on_device_tensors_outside_a_loader():
    rng = np.random.default_rng(9)
    images, mask, alpha, sids = R.random_case(rng, (9, 11, 3), 7, np.float64)
    indices = R.index_set('every_other', sids)
    op = Poison(mask, alpha, indices, clamp=(1, 254))
    d = _dev(images)
    got = op.generate_code()(d, None, sids)
    assert got is d and np.array_equal(d.cpu().numpy(), R.poison_np(images, mask, alpha, sids, indices, (1, 254)))
    assert len(op._device._dev) == 1                                    # tables and ids uploaded once, kept
    first = op._device._dev[ch.device(DEV)]
    op.generate_code()(_dev(images), None, sids)
    assert op._device._dev[ch.device(DEV)] is first
    with pytest.raises(TypeError):
        op.generate_code()(d.permute(0, 3, 1, 2), None, sids)


# ------------------------------------------------------------- Loaders --
N = 40
CHOSEN = [0, 3, 6, 7, 16, 31, 39, 39, 500]


def _beton(tmpdir_m, name, mode, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(N, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


def _stamp(hw):
    rng = np.random.default_rng(hw)
    alpha = rng.random((hw, hw)).astype(np.float32)
    alpha[:hw // 4, :hw // 4] = 1.0
    return rng.integers(0, 256, (hw, hw, 3), dtype=np.uint8), alpha


def _cpu_epochs(fn, decoder, hw, seed, epochs=2):
    mask, alpha = _stamp(hw)
    kw = dict(batch_size=16, device='cpu', seed=seed, drop_last=False)
    plain = Loader(fn, pipelines={'image': [decoder(), RandomHorizontalFlip(0.5)], 'label': [IntDecoder()]}, **kw)
    loader = Loader(fn, pipelines={'image': [decoder(), Poison(mask, alpha, CHOSEN), RandomHorizontalFlip(0.5)],
                                   'label': [IntDecoder(), ReplaceLabel(CHOSEN, 11)]}, **kw)
    out = []
    for _ in range(epochs):
        batches = [(np.array(im), np.array(lab)) for im, lab in loader]
        ims, labs = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
        base = np.concatenate([np.array(im) for im, _ in plain])
        changed = [k for k in range(N) if not np.array_equal(ims[k], base[k])]
        assert changed == sorted(set(CHOSEN) - {500}) == np.nonzero(labs.reshape(-1) == 11)[0].tolist()
        out.append((ims, labs))
    return out


def _dev_loader(fn, decoder, hw, seed, label_on_device, **kw):
    mask, alpha = _stamp(hw)
    label = [IntDecoder(), ToTensor(), ToDevice(DEV), ReplaceLabel(CHOSEN, 11)] if label_on_device else \
        [IntDecoder(), ReplaceLabel(CHOSEN, 11), ToTensor(), ToDevice(DEV)]
    return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
        'image': [decoder(), Poison(mask, alpha, CHOSEN), RandomHorizontalFlip(0.5), ToTensor(), ToDevice(DEV),
                  ToTorchImage(), NormalizeImage(MEAN, STD, np.float16)],
        'label': label}, **kw)


def _check_device_loader(loader, want_epochs, want_g):
    assert loader.graph.groupable()
    for want_u8, want_lab in want_epochs:
        it = iter(loader)
        assert it.G == want_g                                           # the iterator actually grouped
        batches = [(im.permute(0, 2, 3, 1).cpu().numpy(), lab.cpu().numpy()) for im, lab in it]
        got = np.concatenate([b[0] for b in batches])
        lab = np.concatenate([b[1] for b in batches])
        assert got.dtype == np.float16 and got.shape == want_u8.shape and len(got) == N
        want = np.stack([LUT[want_u8[..., c], c] for c in range(3)], -1)
        bad = [k for k in range(N) if not np.array_equal(got[k].view(np.uint16), want[k].view(np.uint16))]
        assert not bad, bad[:8]
        assert lab.dtype == np.int64 and np.array_equal(lab, want_lab)


@pytest.mark.parametrize('label_on_device', [False, True])
@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case, label_on_device):
    """40 samples in batches of 16 (the last one partial), two epochs (the
    flips differ, the stamped samples do not)."""
    if case == 'raw32':
        fn, hw = _beton(tmpdir_m, 'psn_raw.beton', 'raw', (32, 32), 4), 32
        decoder = SimpleRGBImageDecoder
    else:
        fn, hw = _beton(tmpdir_m, 'psn_jpg.beton', 'jpg', (96, 120), 5), 64
        decoder = (lambda: RandomResizedCropRGBImageDecoder((64, 64)))
    seed = 29
    want = _cpu_epochs(fn, decoder, hw, seed)
    assert not np.array_equal(want[0][0], want[1][0])
    args = (fn, decoder, hw, seed, label_on_device)
    _check_device_loader(_dev_loader(*args, device_cache=True, batches_per_launch=1), want, 1)
    _check_device_loader(_dev_loader(*args, device_cache=False), want[:1], 3)
    _check_device_loader(_dev_loader(*args, batches_per_launch=3), want, 3)
    _check_device_loader(_dev_loader(*args), want, 3)                   # the default keeps the group
