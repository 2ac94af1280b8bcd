"""RandomPerspective on the MI355X, byte for byte against the numpy statement
(tests/perspective_ref.py): ffcv_perspective_batch in every regime (a
workgroup per image; tiles that stage their footprint, read global memory
directly, or read nothing) inside guarded buffers, the device draws against
the host twin as bits, and a device Loader against the CPU Loader."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, RandomPerspective
from tests import perspective_ref as R
from tests.helpers import NaturalDS, write
from tests.test_blur import make_inputs, mixed_apply
from tests.test_perspective import FILL, MODES, SEED, SHAPES, coef_sets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def _device_warp(imgs, mode, apply, coef, slead=3, pad=7):
    """ffcv_perspective_batch with imgs at an odd byte offset of a device
    buffer into a 0xA5-guarded one with a padded stride; checks the guards."""
    B, img = len(imgs), imgs[0].size
    sbuf = ch.full((slead + imgs.size + 33,), 0x3C, dtype=ch.uint8, device=DEV)
    src = sbuf[slead:slead + imgs.size].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    stride = img + pad
    dbuf = ch.full((5 + B * stride + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    L.perspective_batch(src, dbuf[5:], mode, FILL, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV),
                        ch.from_numpy(np.ascontiguousarray(coef, np.float64)).to(DEV), dst_stride=stride)
    out = dbuf.cpu().numpy()
    body = out[5:5 + B * stride].reshape(B, stride)
    assert (out[:5] == 0xA5).all() and (out[5 + B * stride:] == 0xA5).all() and (body[:, img:] == 0xA5).all()
    return body[:, :img].reshape(imgs.shape)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_kernel_matches_numpy(shape, mode):
    """Mixed apply flags under every coefficient set; the strong quadrilateral
    must land tiles in all three regimes; the identity reproduces the input."""
    H, W = shape
    imgs = make_inputs(np.random.default_rng(H * 100 + W), shape)
    sets = coef_sets(H, W)
    whole = L.perspective_whole_bytes()
    assert 3 * 43 * 127 <= whole < 3 * 43 * 128
    if 3 * H * W > whole and min(shape) > 64:
        th, tw = L.perspective_tile_shape()
        sizes = [L.perspective_tile_bytes(H, W, mode, sets['strong'], r, c)
                 for r in range(-(-H // th)) for c in range(-(-W // tw))]
        lds = L.perspective_tile_lds()
        assert any(0 < s <= lds for s in sizes) and any(s > lds for s in sizes) and any(s == 0 for s in sizes), sizes
    for name, q in sets.items():
        coef = np.stack([q] * len(imgs))
        got = _device_warp(imgs, mode, mixed_apply(), coef)
        want = R.warp_batch(imgs, coef, mode, mixed_apply(), FILL)
        bad = [k for k in range(len(imgs)) if not np.array_equal(got[k], want[k])]
        assert not bad, (shape, mode, name, bad)
        if name == 'identity':
            assert np.array_equal(got, imgs)
        if name == 'horizon':
            assert (got[0, int(0.6 * H) + 1:] == np.array(FILL, np.uint8)).all()   # the far side


@pytest.mark.parametrize('d', (0.0, 0.5, 1.0))
def test_device_draws_equal_host_draws_as_bits(d):
    ids = np.arange(256, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for H, W in ((2, 2), (2, 9), (32, 32), (97, 131)):
        apply = ch.full((256,), 9, dtype=ch.uint8, device=DEV)
        coef = ch.full((256, 9), -7, dtype=ch.float64, device=DEV)
        status = ch.full((256,), -1, dtype=ch.int32, device=DEV)
        L.perspective_draw_batch(d_ids, SEED, 1, 0.6, d, H, W, apply, coef, status)
        ha, hq = L.perspective_draw_batch_host(ids, SEED, 1, 0.6, d, H, W)
        assert (status == 0).all() and np.array_equal(apply.cpu().numpy(), ha)
        assert np.array_equal(coef.cpu().numpy().view(np.uint64), hq.view(np.uint64)), (H, W)


@pytest.mark.parametrize('interpolation', ('bilinear', 'nearest'))
def test_device_loader_matches_cpu_loader(tmp_path, interpolation):
    """32 x 32 raw, 64 samples, two epochs, launch groups of two."""
    fn = write(str(tmp_path / 'persp.beton'), NaturalDS(64, hw=(32, 32), seed=4),
               {'image': RGBImageField(write_mode='raw'), 'label': IntField()})

    def ops():
        return [SimpleRGBImageDecoder(), RandomPerspective(0.6, 0.7, interpolation, FILL), ToTensor()]
    cpu = Loader(fn, batch_size=16, device='cpu', seed=SEED, drop_last=False, pipelines={'image': ops()})
    loader = Loader(fn, batch_size=16, seed=SEED, drop_last=False, batches_per_launch=2, pipelines={
        'image': ops() + [ToDevice(DEV)], 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]})
    assert loader.graph.groupable() and launch_group(loader, len(loader)) == 2
    assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
    epochs = []
    for _ in range(2):
        want = np.concatenate([im.numpy() for im, _ in cpu])
        got = np.concatenate([im.cpu().numpy() for im, _ in loader])
        bad = [k for k in range(len(got)) if not np.array_equal(got[k], want[k])]
        assert got.shape == want.shape and not bad, (interpolation, bad[:8])
        epochs.append(got)
    assert not np.array_equal(epochs[0], epochs[1])
