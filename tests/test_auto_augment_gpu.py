"""TrivialAugmentWide on the MI355X: the device draws against the host twin in
every output array (compared as bits), ffcv_tone_batch_bits against its host
twin in both regimes, the launch sequence against the host twins' on images
beyond every kernel's whole-image regime, and device Loaders against the CPU
Loader under the same seed."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, TrivialAugmentWide
from ffcv_amd.transforms.auto_augment import value_table
from tests import auto_augment_ref as R
from tests import tone_ref as TR
from tests.helpers import NaturalDS, write
from tests.test_auto_augment import SEED

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _torch_dtype(dt):
    return getattr(ch, np.dtype(dt).name)


def _device_draws(ids, seed, epoch, nbins, H, W):
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    out = {name: ch.full(shape(len(ids)), 77, dtype=_torch_dtype(dt), device=DEV)
           for name, dt, shape in L.POLICY_ARRAYS}
    status = ch.full((len(ids),), -1, dtype=ch.int32, device=DEV)
    L.policy_draw_batch(d_ids, seed, epoch, nbins, ch.from_numpy(value_table(nbins)).to(DEV), H, W, out, status)
    assert (status == 0).all()
    return out


@pytest.mark.parametrize('nbins,hw', ((31, (32, 32)), (10, (33, 47))))
def test_device_draws_equal_host_draws(nbins, hw):
    ids = np.arange(2048, dtype=np.uint64)
    for seed, epoch in ((SEED, 0), (2 ** 63 + 5, 7)):
        dev = _device_draws(ids, seed, epoch, nbins, *hw)
        host = L.policy_draw_batch_host(ids, seed, epoch, nbins, value_table(nbins), *hw)
        for name, dt, _ in L.POLICY_ARRAYS:
            got = dev[name].cpu().numpy()
            assert got.dtype == np.dtype(dt) and got.shape == host[name].shape
            assert np.array_equal(got.view(np.uint8), host[name].view(np.uint8)), (name, seed, epoch)
        assert len(set(host['op'])) == R.NUM_OPS
    op, b, neg = R.draw(SEED, 0, 5, nbins)
    assert L.policy_draw_batch_host(ids[:8], SEED, 0, nbins, value_table(nbins), *hw)['op'][5] == op


@pytest.mark.parametrize('hw', ((32, 32), (80, 80), (7, 5)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_tone_bits_matches_host_twin(hw):
    """[posterize, autocontrast, equalize] with per-sample bits 1 .. 8: one
    workgroup per image at 32 x 32, tiles with the two-pass statistics at
    80 x 80; images at an odd byte offset inside a guarded buffer."""
    h, w = hw
    assert (h * w * 3 > L.tone_lds_bytes()) == (hw == (80, 80))
    rng = np.random.default_rng(3)
    B = 16
    imgs = np.stack([TR.family(rng, TR.FAMILIES[k % 5], h, w) for k in range(B)])
    bits = (np.arange(B) % 8 + 1).astype(np.uint8)
    ws = ch.empty((768 * B,), dtype=ch.int32, device=DEV)
    for n, apply in enumerate((np.tile([[1], [0], [0]], (1, B)), rng.integers(0, 2, (3, B)), np.ones((3, B)))):
        apply = apply.astype(np.uint8)
        want = imgs.copy()
        L.tone_batch_bits_host(want, TONE_STEPS, apply, bits)
        buf = ch.full((imgs.size + 40,), 0xA5, dtype=ch.uint8, device=DEV)
        lead = 3 + 4 * n
        view = buf[lead:lead + imgs.size].view(imgs.shape)
        view.copy_(ch.from_numpy(imgs))
        L.tone_batch_bits(view, TONE_STEPS, ch.from_numpy(apply).to(DEV), ch.from_numpy(bits).to(DEV), ws)
        out = buf.cpu().numpy()
        assert (out[:lead] == 0xA5).all() and (out[lead + imgs.size:] == 0xA5).all()
        got = out[lead:lead + imgs.size].reshape(imgs.shape)
        bad = [k for k in range(B) if not np.array_equal(got[k], want[k])]
        assert not bad, (hw, n, bad)
        assert not np.array_equal(got, imgs)
    # NULL bits is ffcv_tone_batch
    a = ch.from_numpy(imgs).to(DEV)
    b = a.clone()
    ones = ch.ones((3, B), dtype=ch.uint8, device=DEV)
    L.tone_batch(a, TONE_STEPS, 3, ones, ws)
    params = L.tone_params(TONE_STEPS, 3)
    L.tone_batch_bits(b, params, ones, None, ws)
    assert ch.equal(a, b)


@pytest.mark.parametrize('hw,mode', (((80, 80), 1), ((97, 131), 0)), ids=('80x80-nearest', '97x131-bilinear'))
def test_launch_sequence_matches_host_twins(hw, mode):
    """The op's launches on 56 images beyond every kernel's whole-image
    regime (every operation occurs), against the host twins of the same
    entries; the output starts as 0xA5 and every image of it is written."""
    H, W = hw
    B = 56
    ids = np.arange(B, dtype=np.uint64) + 100
    table = value_table(31)
    host = L.policy_draw_batch_host(ids, SEED, 1, 31, table, H, W)
    assert len(set(host['op'])) == R.NUM_OPS
    rng = np.random.default_rng(5)
    imgs = np.stack([TR.family(rng, TR.FAMILIES[k % 5], H, W) for k in range(B)])
    fill = (9, 200, 31)
    src = imgs.copy()
    want = np.full_like(imgs, 0xA5)
    L.color_jitter_batch_host(src, CJ_STEPS, host['cj_apply'][:3], host['cj_ratio'][:3])
    L.color_jitter_batch_host(src, SOLARIZE_STEPS, host['cj_apply'][3:], host['cj_ratio'][3:])
    L.tone_batch_bits_host(src, TONE_STEPS, host['tone_apply'], host['tone_bits'])
    L.affine_batch_host(src, want, mode, fill, host['aff_apply'], host['aff_coef'], nthreads=4)
    L.sharpness_batch_host(src, want, host['sharp_apply'], host['sharp_factor'], nthreads=4)
    changed = sum(not np.array_equal(want[k], imgs[k]) for k in range(B))
    assert B // 2 < changed and not (want == 0xA5).all(axis=(1, 2, 3)).any()

    d = _device_draws(ids, SEED, 1, 31, H, W)
    x = ch.from_numpy(imgs).to(DEV)
    out = ch.full_like(x, 0xA5)
    assert H * W * 3 > max(L.color_jitter_lds_bytes(), L.tone_lds_bytes())
    L.color_jitter_batch(x, CJ_STEPS, d['cj_apply'][:3], d['cj_ratio'][:3], ch.empty((B,), dtype=ch.int64, device=DEV))
    L.color_jitter_batch(x, SOLARIZE_STEPS, d['cj_apply'][3:], d['cj_ratio'][3:])
    L.tone_batch_bits(x, TONE_STEPS, d['tone_apply'], d['tone_bits'], ch.empty((768 * B,), dtype=ch.int32, device=DEV))
    L.affine_batch(x, out, mode, fill, d['aff_apply'], d['aff_coef'])
    L.sharpness_batch(x, out, d['sharp_apply'], d['sharp_factor'])
    got = out.cpu().numpy()
    bad = [(k, int(host['op'][k])) for k in range(B) if not np.array_equal(got[k], want[k])]
    assert not bad, (hw, bad)
    assert np.array_equal(x.cpu().numpy(), src)


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case):
    """[decoder, TrivialAugmentWide(), flip] on the device Loader, one batch
    per launch, with the Loader's own launch groups and with groups of 3,
    against the CPU Loader under the same seed, over two epochs."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'taw_raw.beton', 'raw', 40, (32, 32), 4)
        decoder = SimpleRGBImageDecoder
    else:
        fn = _beton(tmpdir_m, 'taw_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = lambda: RandomResizedCropRGBImageDecoder((64, 64))  # noqa: E731
    seed = 17
    chain = lambda: [decoder(), TrivialAugmentWide(), RandomHorizontalFlip()]  # noqa: E731
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': chain() + [ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]
    assert not np.array_equal(want[0], want[1])
    ops = {R.draw(seed, e, k)[0] for e in range(2) for k in range(40)}
    assert len(ops) >= 12          # the two epochs of 40 samples draw nearly every operation

    def dev(**kw):
        return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
            'image': chain() + [ToTensor(), ToDevice(DEV)],
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict(), dict(batches_per_launch=3)):
        loader = dev(**kw)
        assert loader.graph.groupable()                     # launch groups are kept
        assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
        assert launch_group(loader, len(loader)) == (kw.get('batches_per_launch') or len(loader))
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            assert got.dtype == np.uint8 and got.shape == want_u8.shape
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (case, kw, bad[:8])
