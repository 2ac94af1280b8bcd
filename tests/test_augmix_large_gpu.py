"""AugMix's launch for images beyond 64 x 64 (ffcv_augmix_large_batch) on the
MI355X, to the bit: the kernel on hand-written arrays against the statement of
test_augmix_gpu.py; rounding and cap; the dispatch's bounds; a Loader."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields.decoders import IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, AugMix
from tests import affine_ref as AR
from tests import auto_augment_ref as R
from tests.test_augmix import SEED
from tests.test_augmix_gpu import hand_chains, statement, operation_expected
from tests.test_randaugment_gpu import FILL, hand_arrays, images, run_device_op, _beton, _to_device, tmpdir_m  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def large_in_guards(imgs, d, width, mode, fill, slabs):
    """ffcv_augmix_large_batch with src and dst at odd byte offsets inside
    0xA5-guarded buffers and a workspace of exactly `slabs` slabs."""
    n = imgs.size
    src_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    dst_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    ws = ch.empty(slabs * L.augmix_large_slab_bytes(*imgs.shape[1:3], width), dtype=ch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    sl, dl = 3, 21
    src = src_buf[sl:sl + n].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    L.augmix_large_batch(src, dst_buf[dl:dl + n].view(imgs.shape), width, mode, fill, _to_device(d), ws)
    o = dst_buf.cpu().numpy()
    assert np.array_equal(src_buf.cpu().numpy()[sl:sl + n], imgs.ravel())
    assert (o[:dl] == 0xA5).all() and (o[dl + n:] == 0xA5).all()
    return o[dl:dl + n].reshape(imgs.shape)


SHAPES = ((1, 1), (7, 5), (117, 117), (150, 333), (224, 224))
CASES = [(hw, w, m, 5) for hw in SHAPES for w, m in ((1, AR.NEAREST), (3, AR.BILINEAR), (4, AR.NEAREST))]
CASES.append(((117, 117), 3, AR.BILINEAR, 64))


@pytest.mark.parametrize('hw,width,mode,slabs', CASES, ids=lambda v: f'{v[0]}x{v[1]}' if isinstance(v, tuple) else str(v))
def test_large_kernel_matches_the_statement(hw, width, mode, slabs):
    """39 images over 5 workgroups: every slab is reused and the tail is
    uneven; over 64 slabs: more slabs than images."""
    H, W = hw
    assert L.augmix_large_fits(H, W) and (3 * H * W >= L.randaugment_large_min_bytes()) == (H >= 117)
    B = 39
    d, seqs = hand_chains(B, width, H, W)
    imgs = images(B, H, W, 7 + H)
    want = statement(imgs, d, width, mode, FILL)
    got = large_in_guards(imgs, d, width, mode, FILL, slabs)
    bad = [(k, tuple(seqs[k])) for k in range(B) if not np.array_equal(got[k], want[k])]
    assert not bad, (hw, width, bad[:6])


def test_large_kernel_rounds_half_to_even_and_caps():
    """The construction of test_fused_kernel_rounds_half_to_even_and_caps
    (halves down and up to even, an Identity-only chain, the cap), two slabs."""
    H, W = 4, 3
    seqs = np.array([[R.POSTERIZE, 0, 0], [R.SOLARIZE, 0, 0], [R.IDENTITY, 0, 0], [R.POSTERIZE, 0, 0],
                     [R.SOLARIZE, 0, 0]])
    d = hand_arrays(seqs, np.zeros(seqs.shape, bool), H, W)
    d['tone_bits'][0, [0, 3]] = 7
    d['cj_ratio'][0, 3, [1, 4]] = 0.0
    d['depth'] = np.ones((1, 5), np.uint8)
    d['weights'] = np.array([[0.5, 0.5, 0.75, 1.0, 0.0], [0.5, 0.5, 0.75, 0.0, 1.0]], np.float32)
    imgs = np.tile(np.arange(36, dtype=np.uint8).reshape(1, H, W, 3), (5, 1, 1, 1))
    imgs[2] = 255
    got = large_in_guards(imgs, d, 1, AR.NEAREST, FILL, 2)
    assert np.array_equal(got[0], imgs[0] & 254)
    assert (got[1] == 128).all() and (got[2] == 255).all()
    assert np.array_equal(got[3], imgs[3]) and np.array_equal(got[4], 255 - imgs[4])
    assert np.array_equal(got, statement(imgs, d, 1, AR.NEAREST, FILL))


def test_dispatch_bounds_of_the_large_launch(monkeypatch):
    """From randaugment_large_min_bytes() on, while the shape fits: 117 x 117
    is the one launch; 116 x 117 (below) and 224 x 225 (beyond) are the rounds."""
    assert 3 * 116 * 117 < L.randaugment_large_min_bytes() <= 3 * 117 * 117
    assert L.augmix_large_fits(224, 224) and not L.augmix_large_fits(224, 225)
    ids = np.arange(20, dtype=np.uint64) + 300
    calls = []
    for name in ('augmix_batch', 'augmix_mix_batch', 'augmix_large_batch'):
        monkeypatch.setattr(L, name, lambda *a, _f=getattr(L, name), _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    for H, W in ((117, 117), (116, 117), (224, 225)):
        del calls[:]
        imgs = images(len(ids), H, W, 19)
        op = AugMix(severity=6, chain_depth=2, interpolation='bilinear', fill=FILL)
        got, _ = run_device_op(op, imgs, ids, SEED, 2, monkeypatch)
        assert np.array_equal(got, operation_expected(imgs, ids, SEED, 2, op, AR.BILINEAR)), (H, W)
        if (H, W) == (117, 117):
            assert calls == ['augmix_large_batch']
        else:
            assert calls[-1] == 'augmix_mix_batch' and 'augmix_large_batch' not in calls


def test_device_loader_matches_cpu_loader_at_128(tmpdir_m):  # noqa: F811
    """The large launch at 128 x 128 behind the JPEG decoder; the launch group is the plain pipeline's."""
    fn = _beton(tmpdir_m, 'aml_jpg.beton', 'jpg', 40, (144, 160), 6)
    decoder = lambda: RandomResizedCropRGBImageDecoder((128, 128))  # noqa: E731
    chain = lambda: [decoder(), AugMix(), RandomHorizontalFlip()]  # noqa: E731
    cpu = Loader(fn, batch_size=16, device='cpu', seed=17, drop_last=False, pipelines={'image': chain() + [ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]

    def dev(ops, **kw):
        return Loader(fn, batch_size=16, seed=17, drop_last=False, pipelines={
            'image': ops + [ToTensor(), ToDevice(DEV)], 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict()):
        loader, plain = dev(chain(), **kw), dev([decoder(), RandomHorizontalFlip()], **kw)
        assert loader.graph.groupable()
        assert launch_group(loader, len(loader)) == launch_group(plain, len(plain))
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (kw, bad[:8])
