"""RandomAdjustSharpness on the MI355X, bit for bit against the numpy statement
(tests/sharpness_ref.py): ffcv_sharpness_batch in both regimes (a workgroup
per image; bands of rows, column strips) with apply codes 0 / 1 / 2 mixed and
src and dst at every byte alignment inside guarded buffers, a padded
dst_stride, the order fixture, the device draws against the host twin, and
device Loaders against the CPU Loader under the same seed."""
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
from ffcv_amd.transforms import ToTensor, ToDevice, RandomAdjustSharpness
from tests import sharpness_ref as R
from tests.helpers import NaturalDS, write
from tests.test_sharpness import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LDS, BAND = 24576, 16      # asserted against the library below
FACTORS = (0, 0.3, 1, 1.7, 2, 16)
# below 3 x 3 (a copy through the stencil's path), the smallest stencils, 32 x 32, the largest whole image
# (6 * 64 * 64 = 24,576) and the first beyond it (four bands), a last band of one row, an image shorter than a band,
# two column strips and three
SHAPES = ((1, 1), (2, 5), (3, 3), (3, 4), (32, 32), (64, 64), (64, 65), (2 * BAND + 1, 125), (10, 412), (20, 300),
          (17, 600))


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _device_sharpness(imgs, apply, factor, slead=0, dlead=0):
    """ffcv_sharpness_batch with imgs `slead` bytes into a 0x3C-guarded device
    buffer and the output `dlead` bytes into a 0xA5-filled one; returns the
    output and checks the guards and the source."""
    nb = imgs.size
    sbuf = ch.full((slead + nb + 33,), 0x3C, dtype=ch.uint8, device=DEV)
    dbuf = ch.full((dlead + nb + 33,), 0xA5, dtype=ch.uint8, device=DEV)
    src = sbuf[slead:slead + nb].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    dst = dbuf[dlead:dlead + nb].view(imgs.shape)
    L.sharpness_batch(src, dst, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                      ch.from_numpy(np.ascontiguousarray(factor, np.float32)).to(DEV))
    out, back = dbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert (out[:dlead] == 0xA5).all() and (out[dlead + nb:] == 0xA5).all()
    assert (back[:slead] == 0x3C).all() and (back[slead + nb:] == 0x3C).all()
    assert np.array_equal(back[slead:slead + nb].reshape(imgs.shape), imgs)
    return out[dlead:dlead + nb].reshape(imgs.shape)


def test_regime_constants():
    assert L.sharpness_lds_bytes() == LDS and L.sharpness_band_rows() == BAND
    assert 6 * 64 * 64 <= LDS < 6 * 64 * 65
    for h, w in SHAPES[:9]:
        assert L.sharpness_strip_cols(h, w) == w                 # one strip
    assert 300 / 2 <= L.sharpness_strip_cols(20, 300) < 300      # two strips
    assert 600 / 3 <= L.sharpness_strip_cols(17, 600) < 600 / 2  # three


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_kernel_matches_numpy(shape):
    """Batches of 7 images (random, all-0, all-255, checkerboard, random) with
    codes 2, 0, 7, 1, 1, 1, 1: every factor at one alignment, then all 16
    alignments of src, dst's running against it, with a factor per image.
    Code-2 images stay 0xA5, copies equal the input."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    imgs = R.make_inputs(rng, shape)
    B = len(imgs)
    apply = R.mixed_apply()
    filled = np.full_like(imgs, 0xA5)
    want = {f: R.sharpen_batch(imgs, apply, np.full(B, f, np.float32), filled) for f in FACTORS}
    assert (want[2][0] == 0xA5).all() and np.array_equal(want[2][1], imgs[1]) and np.array_equal(want[2][2], imgs[2])

    def check(got, exp, what):
        bad = [k for k in range(B) if not np.array_equal(got[k], exp[k])]
        assert not bad, (shape, what, bad)
    for n, f in enumerate(FACTORS):
        check(_device_sharpness(imgs, apply, np.full(B, f, np.float32), slead=3 + n, dlead=14 - n), want[f], f)
    mixed = np.array([FACTORS[(k + 1) % len(FACTORS)] for k in range(B)], np.float32)
    want_mixed = np.stack([want[FACTORS[(k + 1) % len(FACTORS)]][k] for k in range(B)])
    for a in range(16):
        check(_device_sharpness(imgs, apply, mixed, slead=a, dlead=(11 * a + 5) & 15), want_mixed, a)
    # every image sharpened
    ones = np.ones(B, np.uint8)
    check(_device_sharpness(imgs, ones, mixed, slead=1, dlead=2), R.sharpen_batch(imgs, ones, mixed, filled), 'all')


def test_padded_dst_stride():
    rng = np.random.default_rng(2)
    imgs = R.make_inputs(rng, (33, 31))
    B, img = len(imgs), imgs[0].size
    stride = img + 7
    dbuf = ch.full((B * stride + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    apply = R.mixed_apply()
    factor = np.full(B, 1.7, np.float32)
    L.sharpness_batch(ch.from_numpy(imgs).to(DEV), dbuf[1:], ch.from_numpy(apply).to(DEV),
                      ch.from_numpy(factor).to(DEV), dst_stride=stride)
    out = dbuf.cpu().numpy()
    want = R.sharpen_batch(imgs, apply, factor, np.full_like(imgs, 0xA5))
    for k in range(B):
        o = 1 + k * stride
        assert np.array_equal(out[o:o + img].reshape(imgs[k].shape), want[k]), k
        assert (out[o + img:o + stride] == 0xA5).all()
    assert out[0] == 0xA5 and (want[0] == 0xA5).all() and want.max() == 255


def test_order_fixture():
    z = np.load(GOLDEN)
    tiles, factor, want = z['tiles'], z['factor'], z['want']
    assert (want != z['fma']).all()
    ones = np.ones(len(tiles), np.uint8)
    got = _device_sharpness(tiles, ones, factor, slead=1, dlead=2)
    assert np.array_equal(got[:, 1, 1], want)
    # whole images too: the tiles set into a 64 x 64 image and a 33 x 125 one
    for shape in ((64, 64), (33, 125)):
        rng = np.random.default_rng(9)
        imgs = rng.integers(0, 256, (len(tiles),) + shape + (3,), dtype=np.uint8)
        imgs[:, 15:18, 30:33] = tiles
        got = _device_sharpness(imgs, ones, factor, slead=7, dlead=9)
        assert np.array_equal(got[:, 16, 31], want), shape
        assert np.array_equal(got, R.sharpen_batch(imgs, ones, factor, imgs))


def test_device_draws_equal_host_draws():
    ids = np.arange(256, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for seed, epoch, p, f in ((5, 0, 0.5, 2.0), (2 ** 63 + 5, 7, 0.1, 0.3), (1, 1, 1.0, 16)):
        apply = ch.full((256,), 9, dtype=ch.uint8, device=DEV)
        factor = ch.full((256,), 7.0, dtype=ch.float32, device=DEV)
        status = ch.full((256,), -1, dtype=ch.int32, device=DEV)
        L.sharpness_draw_batch(d_ids, seed, epoch, p, f, apply, factor, status)
        ha, hf = L.sharpness_draw_batch_host(ids, seed, epoch, p, f)
        assert (status == 0).all()
        assert np.array_equal(apply.cpu().numpy(), ha)
        assert np.array_equal(factor.cpu().numpy().view(np.uint32), hf.view(np.uint32))
        assert bool(ha[3]) == R.draw(seed, epoch, 3, p)


def test_in_place_is_rejected_before_any_launch():
    lib = L.lib()
    img = ch.full((2, 40, 40, 3), 77, dtype=ch.uint8, device=DEV)
    apply = ch.ones((2,), dtype=ch.uint8, device=DEV)
    factor = ch.ones((2,), dtype=ch.float32, device=DEV)
    ch.cuda.synchronize()
    for off in (0, 1, 4799, 9599):
        assert lib.ffcv_sharpness_batch(None, img.data_ptr(), img.data_ptr() + off, 2, 40, 40, apply.data_ptr(),
                                        factor.data_ptr(), 0) == -1
        assert b'overlap' in lib.ffcv_last_error()
    with pytest.raises(L.FFCVError, match='overlap'):
        L.sharpness_batch(img, img, apply, factor)
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
    """[decoder, RandomAdjustSharpness(2, p=0.5)] on the device Loader, one
    batch per launch, with the Loader's own launch groups and with groups of 3,
    against the CPU Loader under the same seed, over two epochs."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'sharp_raw.beton', 'raw', 40, (32, 32), 4)
        decoder = SimpleRGBImageDecoder
    else:
        fn = _beton(tmpdir_m, 'sharp_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = lambda: RandomResizedCropRGBImageDecoder((64, 64))  # noqa: E731
    seed = 17
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [decoder(), RandomAdjustSharpness(2, p=0.5), ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]
    assert not np.array_equal(want[0], want[1])

    def dev(**kw):
        return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
            'image': [decoder(), RandomAdjustSharpness(2, p=0.5), ToTensor(), ToDevice(DEV)],
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
