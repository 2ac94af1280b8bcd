"""ffcv_resample_images_batch on the MI355X against the numpy statement
(tests/resample_ref.py), every byte, `inp` and `out` at odd byte offsets inside
0xA5-guarded allocations; a batch past 2^31 bytes; device against CPU Loaders."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from tests import large_batch as LB
from tests import resample_ref as R
from tests.helpers import NaturalDS, write

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (H, W), window (i, j, h, w), (out_h, out_w): what it breaks
CASES = [
    ((1, 1), (0, 0, 1, 1), (1, 1)),                # a single tap
    ((1, 1), (0, 0, 1, 1), (5, 3)),                # ... and a non-square output
    ((7, 5), (3, 1, 2, 3), (7, 7)),                # upscale; clamping at the window; rows of 15 bytes
    ((64, 48), (0, 0, 64, 48), (4, 4)),            # scale 16: the ring wraps, a record is longer than a chunk
    ((3, 3), (0, 0, 3, 3), (64, 64)),              # every record clipped at an edge
    ((33, 47), (0, 0, 33, 47), (32, 32)),          # odd pitches
    ((33, 47), (0, 0, 33, 47), (31, 31)),          # 93 bytes a row: the last dword holds one byte
    ((32, 32), (0, 0, 32, 32), (32, 32)),          # the identity
    ((224, 224), (40, 50, 97, 131), (224, 224)),   # every band boundary
    ((224, 224), (0, 0, 224, 224), (224, 224)),    # the largest staged rows of the 224 recipe
    ((128, 256), (0, 0, 128, 256), (64, 64)),      # the tallest source with chunks of 16 rows, the widest rows
    ((256, 256), (0, 0, 256, 256), (256, 256)),    # the corners of the predicate
    ((256, 256), (0, 0, 256, 256), (1, 1)),
]


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def run(imgs, crops, oh, ow, mode, pad=5):
    """One launch: (images, status); asserts that no byte outside them changed."""
    B, H, W = imgs.shape[:3]
    dense, stride = oh * ow * 3, oh * ow * 3 + pad
    src, dst = LB.DevBuf(imgs.size, 1), LB.DevBuf(B * stride, 3)
    src.flat.copy_(LB.dev(imgs).reshape(-1))
    status = ch.full((B,), -1, dtype=ch.int32, device=DEV)
    L.resample_images_batch(src.flat, H * W * 3, B, H, W, LB.dev(np.asarray(crops, np.int32)), mode, oh, ow,
                            dst.flat, stride, status)
    got = dst.flat.cpu().numpy().reshape(B, stride)
    assert src.guards_ok() and dst.guards_ok() and (got[:, dense:] == LB.FILL_BYTE).all()
    assert np.array_equal(src.flat.cpu().numpy(), imgs.reshape(-1))
    return got[:, :dense].reshape(B, oh, ow, 3), status.cpu().numpy()


@pytest.mark.parametrize('mode', ('bilinear', 'bicubic'))
@pytest.mark.parametrize('case', CASES, ids=[f'{c[0][0]}x{c[0][1]}-{c[1][2]}x{c[1][3]}-{c[2][0]}x{c[2][1]}'
                                             for c in CASES])
def test_entry_is_the_statement(case, mode):
    (H, W), window, (oh, ow) = case
    imgs = R.images(np.random.default_rng(H * 1000 + ow), H, W)
    got, status = run(imgs, [window] * 2, oh, ow, mode)
    assert (status == 0).all()
    for k in range(2):
        want = R.resample(imgs[k], window, oh, ow, mode)
        assert np.array_equal(got[k], want), (k, np.argwhere(got[k] != want)[:4])
    if (window[2], window[3]) == (oh, ow):
        i, j, h, w = window
        assert np.array_equal(got, imgs[:, i:i + h, j:j + w])


@pytest.mark.parametrize('shape', [((12, 10), 4), ((224, 224), 64)], ids=['one-band', 'bands'])
def test_invalid_window(shape):
    (H, W), size = shape
    imgs = R.images(np.random.default_rng(5), H, W)[[0, 0, 0]]
    crops = [(0, 0, H, W), (1, 0, H, W), (1, 1, H - 1, W - 1)]
    got, status = run(imgs, crops, size, size, 'bicubic')
    assert status.tolist() == [0, 8, 0] and (got[1] == 0).all()
    for k in (0, 2):
        assert np.array_equal(got[k], R.resample(imgs[k], crops[k], size, size, 'bicubic'))


def test_last_images_start_past_2g():
    """256 x 256 sources, a period of 251 tiled past 2^31 bytes, each resampled to 8 x 8."""
    LB.need_device()
    H = W = 256
    img, M = H * W * 3, LB.M
    assert LB.wrap_ok(img)
    base = np.random.default_rng(8).integers(0, 256, (M, H, W, 3), dtype=np.uint8)
    crops = np.stack([LB.cyc(3, 1), LB.cyc(3, 2, 1), np.full(M, H - 2), np.full(M, W - 2)], 1).astype(np.int32)
    want = np.stack([R.resample(base[k], crops[k], 8, 8, 'bilinear') for k in range(M)]).reshape(M, 192)
    batch = LB.batch_for(1 << 31, img)
    reps = batch // M
    src, dst = LB.DevBuf(batch * img, 5), LB.DevBuf(batch * 192, 11)
    LB.tile_bytes(src.flat, LB.dev(base).reshape(-1), reps)
    status = ch.full((batch,), -1, dtype=ch.int32, device=DEV)
    L.resample_images_batch(src.flat, img, batch, H, W, LB.tile_param(crops, 0, reps), 'bilinear', 8, 8, dst.flat, 0,
                            status)
    assert src.guards_ok() and dst.guards_ok() and bool((status == 0).all())
    for r in (0, reps - 1):
        assert np.array_equal(dst.flat.view(reps, M, 192)[r].cpu().numpy(), want), r
    assert LB.differing(dst.flat, LB.dev(want), reps)[0] == 0


def _loaders_agree(fn, decoder, size, interpolation, **kw):
    """Two epochs of the device Loader against the CPU Loader's."""
    cpu, dev = R.loader(fn, decoder, size, interpolation), R.loader(fn, decoder, size, interpolation, DEV, **kw)
    epochs = [[np.concatenate([np.asarray(im.cpu()) for im, *_ in ld]) for _ in range(2)] for ld in (cpu, dev)]
    assert not np.array_equal(epochs[0][0], epochs[0][1])
    for want, got in zip(*epochs):
        assert got.dtype == np.uint8 and got.shape[1:] == (size, size, 3) and np.array_equal(got, want)
    return dev


@pytest.mark.parametrize('kind,interpolation', [('raw', 'bicubic'), ('jpg', 'bilinear'), ('jpg', 'area')])
def test_loader_in_launch_groups_matches_cpu_loader(kind, interpolation):
    """raw 32 x 32 -> 32; JPEG through CenterCropRGBImageDecoder (96 x 96) -> 80."""
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import CenterCropRGBImageDecoder, SimpleRGBImageDecoder
    from ffcv_amd.loader.epoch_iterator import launch_group
    fn = os.path.join(tempfile.mkdtemp(), kind + '.beton')
    ds = NaturalDS(40, hw=(32, 32), seed=4) if kind == 'raw' else NaturalDS(40, hw=(100, 120), var=True, seed=6)
    write(fn, ds, {'image': RGBImageField(write_mode=kind), 'label': IntField()})
    decoder = SimpleRGBImageDecoder if kind == 'raw' else lambda: CenterCropRGBImageDecoder((96, 96), 0.875)
    dev = _loaders_agree(fn, decoder, 32 if kind == 'raw' else 80, interpolation, batches_per_launch=2)
    assert dev.graph.groupable() and launch_group(dev, len(dev)) == 2
