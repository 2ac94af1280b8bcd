"""RandAugment's fused kernel for images up to 224 x 224
(ffcv_randaugment_large_batch) on the MI355X: hand-written arrays -- all 196
ordered pairs of operations, triples across two register-to-LDS hand-overs --
against the rounds of host twins, at odd byte offsets inside guarded buffers,
every byte equal; the dispatch at both edges of its regime and the entry's
guards; a device Loader at 128 x 128 against the CPU Loader under one seed."""
import math

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields.decoders import IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, RandAugment
from tests import affine_ref as AR
from tests import randaugment_ref as RA
from tests.test_randaugment import SEED
from tests.test_randaugment_gpu import (DEV, FILL, PAIRS, TRIPLES, _beton, _to_device, assert_images_equal, hand_arrays,
                                        host_expected, host_rounds, images, run_device_op, tmpdir_m)  # noqa: F401

pytestmark = pytest.mark.gpu
ROUND = ['color_jitter_batch', 'color_jitter_batch', 'tone_batch_bits', 'affine_batch', 'sharpness_batch']


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def large_in_guards(imgs, d, mode, fill):
    """ffcv_randaugment_large_batch with src and dst at odd byte offsets inside
    0xA5-guarded buffers: the result, after checking the guards and src."""
    n, sl, dl = imgs.size, 3, 21
    src_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    dst_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    src = src_buf[sl:sl + n].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    L.randaugment_large_batch(src, dst_buf[dl:dl + n].view(imgs.shape), d['op'].shape[0], mode, fill, _to_device(d))
    s, o = src_buf.cpu().numpy(), dst_buf.cpu().numpy()
    assert (s[:sl] == 0xA5).all() and (s[sl + n:] == 0xA5).all() and np.array_equal(s[sl:sl + n], imgs.ravel())
    assert (o[:dl] == 0xA5).all() and (o[dl + n:] == 0xA5).all()
    return o[dl:dl + n].reshape(imgs.shape)


@pytest.mark.parametrize('mode', (AR.NEAREST, AR.BILINEAR), ids=('nearest', 'bilinear'))
@pytest.mark.parametrize('hw', ((1, 1), (7, 5), (97, 131), (223, 225), (224, 224)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_large_pairs_match_host_rounds(hw, mode):
    """One image per ordered pair of operations, strengths of both signs.
    97 x 131 has rows of 393 bytes (the stencil's byte-store tail); 223 x 225
    is three bytes under the edge with odd rows; 224 x 224 is the edge."""
    H, W = hw
    assert L.randaugment_large_fits(H, W)
    seqs = np.array(PAIRS)
    negs = np.array([[(a + b) % 2, (a // 2 + b) % 2] for a, b in PAIRS], bool)
    imgs = images(196, H, W, 7 + H)
    d = hand_arrays(seqs, negs, H, W)
    want = host_rounds(imgs, d, mode, FILL)
    got = large_in_guards(imgs, d, mode, FILL)
    assert_images_equal(got, want, seqs, (hw, mode))
    if H * W >= 35:
        assert sum(not np.array_equal(want[k], imgs[k]) for k in range(196)) > 150


def test_large_triples_match_host_rounds():
    """num_ops = 3 on the 48 triples of the small kernel's test at 113 x 127:
    two hand-overs from registers to the one buffer in a row, and table steps
    on the staged and on the dense image."""
    H, W = 113, 127
    rng = np.random.default_rng(23)
    seqs = np.array(TRIPLES + [tuple(rng.integers(0, RA.NUM_OPS, 3)) for _ in range(48 - len(TRIPLES))])
    negs = rng.integers(0, 2, seqs.shape).astype(bool)
    imgs = images(len(seqs), H, W, 13)
    d = hand_arrays(seqs, negs, H, W)
    for mode in (AR.BILINEAR, AR.NEAREST):
        got = large_in_guards(imgs, d, mode, FILL)
        assert_images_equal(got, host_rounds(imgs, d, mode, FILL), seqs, mode)


def test_dispatch_and_guards(monkeypatch):
    """Below large_min_bytes the rounds; from the first shape at or above it
    to 224 x 224 one large launch; 224 x 225 the rounds again.  The entry
    refuses 224 x 225 and overlapping src / dst."""
    edge = L.randaugment_large_min_bytes()
    H = math.isqrt(-(-edge // 3))
    below, first = (H, (edge - 1) // (3 * H)), (H, -(-edge // (3 * H)))
    assert 6 * below[0] * below[1] > L.randaugment_lds_bytes() and 3 * below[0] * below[1] < edge
    assert 3 * first[0] * first[1] >= edge and L.randaugment_large_fits(*first)
    assert L.randaugment_large_fits(224, 224) and not L.randaugment_large_fits(224, 225)
    calls = []
    monkeypatch.setattr(L, 'randaugment_large_batch',
                        lambda *a, _f=L.randaugment_large_batch, **kw: (calls.append('randaugment_large_batch'),
                                                                        _f(*a, **kw))[1])
    ids = np.arange(28, dtype=np.uint64) + 300
    for (H, W), large in ((below, False), (first, True), ((224, 224), True), ((224, 225), False)):
        imgs = images(len(ids), H, W, 19)
        op = RandAugment(num_ops=2, interpolation='bilinear', fill=FILL)
        del calls[:]
        got, rounds = run_device_op(op, imgs, ids, SEED, 2, monkeypatch)
        want, d = host_expected(imgs, ids, SEED, 2, 2, 31, 9, AR.BILINEAR, FILL)
        assert_images_equal(got, want, d['op'].T, (H, W))
        assert (calls, rounds) == ((['randaugment_large_batch'], []) if large else ([], ROUND * 2)), (H, W)

    d = _to_device(hand_arrays(np.array([[1, 2]]), np.zeros((1, 2), bool), 224, 225))
    x = ch.zeros((2, 224, 225, 3), dtype=ch.uint8, device=DEV)
    with pytest.raises(L.FFCVError, match=r'ffcv_randaugment_large_batch failed \(-1\)'):
        L.randaugment_large_batch(x[:1], x[1:], 2, AR.NEAREST, FILL, d)
    d = _to_device(hand_arrays(np.array([[1, 2]]), np.zeros((1, 2), bool), 224, 224))
    x = ch.zeros((1, 224, 224, 3), dtype=ch.uint8, device=DEV)
    with pytest.raises(L.FFCVError, match=r'failed \(-1\).*overlap'):
        L.randaugment_large_batch(x, x, 2, AR.NEAREST, FILL, d)


def test_device_loader_matches_cpu_loader(tmpdir_m):  # noqa: F811
    """[crop decoder to 128 x 128, RandAugment(), flip] on the device Loader
    (the large launch), one batch per launch and groups of 3, against the CPU
    Loader under the same seed, over two epochs of 40 samples."""
    if not (L.randaugment_large_fits(128, 128) and 3 * 128 * 128 >= L.randaugment_large_min_bytes()):
        pytest.skip('the measured dispatch bounds ended above 128 x 128')
    fn = _beton(tmpdir_m, 'ral_jpg.beton', 'jpg', 40, (150, 170), 6)
    seed = 17
    chain = lambda: [RandomResizedCropRGBImageDecoder((128, 128)), RandAugment(), RandomHorizontalFlip()]  # noqa: E731
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': chain() + [ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]
    assert not np.array_equal(want[0], want[1])
    for bpl in (1, 3):
        loader = Loader(fn, batch_size=16, seed=seed, drop_last=False, batches_per_launch=bpl, pipelines={
            'image': chain() + [ToTensor(), ToDevice(DEV)], 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]})
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            assert got.shape == want_u8.shape
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (bpl, bad[:8])
