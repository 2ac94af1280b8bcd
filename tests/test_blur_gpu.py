"""GaussianBlur on the MI355X, bit for bit against numpy (tests/blur_ref.py):
ffcv_gaussian_blur_batch with numpy's weights in both regimes (a workgroup
per image; bands of rows, column strips) with src and dst at every byte
alignment inside guarded buffers, the order fixture, the device draws and
weights against the host twin under the weight guard, and device Loaders
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
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, GaussianBlur
from tests import blur_ref as R
from tests.helpers import NaturalDS, write
from tests.test_blur import GOLDEN, SEED, SHAPES, SIGMAS, chain_ops, make_inputs, mixed_apply

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LDS, BAND = 32768, 32      # asserted against the library below
# beyond the CPU list: the largest whole image (15 * 46 * 47 = 32,430) and the first beyond it (46 x 48: two
# bands), a one-row last band whose halo reflects, an image shorter than a band under k = 31, two and seven
# column strips, and 97 x 131 at k = 23
EDGE_SHAPES = (((46, 47), (3, 31)), ((46, 48), (3, 31)), ((BAND + 1, 67), (5, 31)), ((20, 120), (31,)),
               ((40, 70), (31,)), ((64, 224), (23,)), ((97, 131), (23,)))


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_blur(imgs, ksize, apply, weights, slead=0, dlead=0):
    """ffcv_gaussian_blur_batch with imgs `slead` bytes into a device buffer
    and the output `dlead` bytes into a 0xA5-guarded one; returns the output
    and checks the guards and the source."""
    nb = imgs.size
    sbuf = ch.full((slead + nb + 33,), 0x3C, dtype=ch.uint8, device=DEV)
    dbuf = ch.full((dlead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    src = sbuf[slead:slead + nb].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    dst = dbuf[dlead:dlead + nb].view(imgs.shape)
    L.gaussian_blur_batch(src, dst, ksize, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                          ch.from_numpy(np.ascontiguousarray(weights, np.float32)).to(DEV))
    out, back = dbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (out[:dlead] == 0xA5).all() and (out[dlead + nb:] == 0xA5).all()
    assert np.array_equal(back[slead:slead + nb].reshape(imgs.shape), imgs)
    return out[dlead:dlead + nb].reshape(imgs.shape)


def test_regime_constants():
    assert L.gaussian_blur_lds_bytes() == LDS and L.gaussian_blur_band_rows() == BAND
    assert 15 * 46 * 47 <= LDS < 15 * 46 * 48 and LDS // (15 * 46) == 47
    assert L.gaussian_blur_strip_cols(46, 47, 31) == 47 and L.gaussian_blur_strip_cols(46, 48, 3) == 48
    assert L.gaussian_blur_strip_cols(20, 120, 31) == 120                  # one strip
    assert 70 / 2 <= L.gaussian_blur_strip_cols(40, 70, 31) < 70           # two strips
    assert 1 <= L.gaussian_blur_strip_cols(64, 224, 23) < 224 / 2          # more than two


@pytest.mark.parametrize('shape,ksizes', SHAPES + EDGE_SHAPES, ids=[f'{s[0]}x{s[1]}' for s, _ in SHAPES + EDGE_SHAPES])
def test_kernel_matches_numpy(shape, ksizes):
    """Batches of 7 images (random, all-0, all-255, checkerboard) with mixed
    apply flags: unapplied images come out equal to the input.  Every kernel
    size at sigma 0.5 runs all 16 alignments of src, with dst's alignment
    running against it; sigma 0.1 and 2.0 run one alignment each."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    imgs = make_inputs(rng, shape)
    apply = mixed_apply()
    for ksize in ksizes:
        assert (ksize - 1) // 2 < min(shape)
        for sigma in SIGMAS:
            weights = np.stack([R.weights_f32(ksize, sigma)] * len(imgs))
            want = R.blur_batch(imgs, ksize, apply, weights)
            for a in (range(16) if sigma == 0.5 else (3,)):
                got = _device_blur(imgs, ksize, apply, weights, slead=a, dlead=(11 * a + 5) & 15)
                bad = [k for k in range(len(imgs)) if not np.array_equal(got[k], want[k])]
                assert not bad, (shape, ksize, sigma, a, bad)
            assert np.array_equal(want[1], imgs[1]) and np.array_equal(want[4], imgs[4])


def test_padded_dst_stride_and_weights_of_the_callers_own():
    rng = np.random.default_rng(2)
    imgs = make_inputs(rng, (33, 31))
    B, img = len(imgs), imgs[0].size
    w = np.zeros((B, R.WROW), np.float32)
    w[:, :5] = 0.31                                     # not normalised: clips at 255
    stride = img + 7
    dbuf = ch.full((B * stride + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    src = ch.from_numpy(imgs).to(DEV)
    apply = ch.from_numpy(mixed_apply()).to(DEV)
    L.gaussian_blur_batch(src, dbuf[1:], 5, apply, ch.from_numpy(w).to(DEV), dst_stride=stride)
    out = dbuf.cpu().numpy()
    want = R.blur_batch(imgs, 5, mixed_apply(), w)
    for k in range(B):
        o = 1 + k * stride
        assert np.array_equal(out[o:o + img].reshape(imgs[k].shape), want[k]), k
        assert (out[o + img:o + stride] == 0xA5).all()
    assert out[0] == 0xA5 and want.max() == 255


def test_order_fixture():
    z = np.load(GOLDEN)
    for ksize in (3, 5, 23):
        r = (ksize - 1) // 2
        tiles, weights, want = z[f'tiles_{ksize}'], z[f'weights_{ksize}'], z[f'want_{ksize}']
        got = _device_blur(tiles, ksize, np.ones(len(tiles), np.uint8), weights, slead=1, dlead=2)
        assert np.array_equal(got[:, r, r], want), ksize
        assert ((want != z[f'fma_{ksize}']) | (want != z[f'reversed_{ksize}'])).any(1).all()
    # whole images too: the tiles of k = 5 set into a 46 x 47 image and a 97 x 131 one
    for shape in ((46, 47), (97, 131)):
        rng = np.random.default_rng(9)
        imgs = rng.integers(0, 256, (16,) + shape + (3,), dtype=np.uint8)
        imgs[:, 20:25, 30:35] = z['tiles_5']
        got = _device_blur(imgs, 5, np.ones(16, np.uint8), z['weights_5'], slead=7, dlead=9)
        assert np.array_equal(got[:, 22, 32], z['want_5']), shape
        assert np.array_equal(got, R.blur_batch(imgs, 5, np.ones(16), z['weights_5']))


@pytest.mark.parametrize('ksize', (1, 3, 5, 9, 23, 31))
def test_device_draws_equal_host_draws_under_the_guard(ksize):
    ids = np.arange(256, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    apply = ch.full((256,), 9, dtype=ch.uint8, device=DEV)
    sigma = ch.zeros((256,), dtype=ch.float64, device=DEV)
    weights = ch.full((256, R.WROW), 7.0, dtype=ch.float32, device=DEV)
    status = ch.full((256,), -1, dtype=ch.int32, device=DEV)
    L.blur_draw_batch(d_ids, SEED, 0, 0.5, 0.1, 2.0, ksize, apply, sigma, weights, status)
    ha, hs, hw = L.blur_draw_batch_host(ids, SEED, 0, 0.5, 0.1, 2.0, ksize)
    assert (status == 0).all()
    assert np.array_equal(apply.cpu().numpy(), ha)
    assert np.array_equal(sigma.cpu().numpy().view(np.uint64), hs.view(np.uint64))
    assert all(R.guard_holds(ksize, s) for s in hs)
    dw = weights.cpu().numpy()
    assert np.array_equal(dw.view(np.uint32), hw.view(np.uint32))
    assert np.array_equal(dw[5].view(np.uint32), R.weights_f32(ksize, hs[5]).view(np.uint32))
    # the draws of grayscale and solarization
    for op_id, p, lo, hi in ((9, 0.1, 0.0, 0.0), (10, 0.5, 128.0, 128.0), (11, 0.5, 0.1, 2.0)):
        value = ch.zeros((256,), dtype=ch.float64, device=DEV)
        L.uniform_draw_batch(d_ids, 2 ** 63 + 5, 7, op_id, p, lo, hi, apply, value, status)
        ua, uv = L.uniform_draw_batch_host(ids, 2 ** 63 + 5, 7, op_id, p, lo, hi)
        assert (status == 0).all() and np.array_equal(apply.cpu().numpy(), ua)
        assert np.array_equal(value.cpu().numpy().view(np.uint64), uv.view(np.uint64))


def test_in_place_is_rejected_before_any_launch():
    lib = L.lib()
    img = ch.full((2, 40, 40, 3), 77, dtype=ch.uint8, device=DEV)
    apply = ch.ones((2,), dtype=ch.uint8, device=DEV)
    w = ch.zeros((2, R.WROW), dtype=ch.float32, device=DEV)
    ch.cuda.synchronize()
    for off in (0, 1, 4799, 9599):
        assert lib.ffcv_gaussian_blur_batch(None, img.data_ptr(), img.data_ptr() + off, 2, 40, 40, 3,
                                            apply.data_ptr(), w.data_ptr(), 0) == -1
        assert b'overlap' in lib.ffcv_last_error()
    with pytest.raises(L.FFCVError, match='overlap'):
        L.gaussian_blur_batch(img, img, 3, apply, w)
    ch.cuda.synchronize()
    assert (img == 77).all()


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


@pytest.mark.parametrize('case', ['raw32', 'jpeg64'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case):
    """[decoder, brightness, grayscale, GaussianBlur(5), solarization] on the
    device Loader, one batch per launch, with the Loader's own launch groups
    and with groups of 3, against the CPU Loader under the same seed; 32 x 32
    images blur whole, 64 x 64 crops in two bands."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'blur_raw.beton', 'raw', 40, (32, 32), 4)
        decoder = SimpleRGBImageDecoder
    else:
        fn = _beton(tmpdir_m, 'blur_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = lambda: RandomResizedCropRGBImageDecoder((64, 64))  # noqa: E731
    seed = 17
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [decoder()] + chain_ops() + [ToTensor()]})
    want = [np.concatenate([im.numpy() for im, _ in cpu]) for _ in range(2)]
    assert not np.array_equal(want[0], want[1])

    def dev(**kw):
        return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
            'image': [decoder()] + chain_ops() + [ToTensor(), ToDevice(DEV)],
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict(), dict(batches_per_launch=3)):
        loader = dev(**kw)
        ops = loader.pipeline_specs['image'].transforms
        assert loader.graph.groupable()                     # launch groups are kept
        assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
        assert launch_group(loader, len(loader)) == (kw.get('batches_per_launch') or len(loader))
        assert ops[0]._program == ops[0:2] and ops[1]._absorbed and isinstance(ops[2], GaussianBlur)
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            assert got.dtype == np.uint8 and got.shape == want_u8.shape
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (case, kw, bad[:8])
