"""ElasticTransform on the MI355X, byte for byte against the numpy statement
(tests/elastic_ref.py): ffcv_elastic_batch at every case of tests/test_elastic.py
inside guarded buffers, and a device Loader against the CPU Loader."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, ElasticTransform
from tests.helpers import NaturalDS, write
from tests.test_elastic import CASES, CASE_IDS, EPOCH, FILL, IDS, MODES, SEED, expected, inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def _device_warp(imgs, mode, alpha, sigma, slead=3, pad=7):
    """ffcv_elastic_batch with imgs at an odd byte offset of a device buffer
    into a 0xA5-guarded one with a padded stride; checks the guards."""
    B, img = len(imgs), imgs[0].size
    sbuf = ch.full((slead + imgs.size + 33,), 0x3C, dtype=ch.uint8, device=DEV)
    src = sbuf[slead:slead + imgs.size].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    stride = img + pad
    dbuf = ch.full((5 + B * stride + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    L.elastic_batch(src, dbuf[5:], mode, FILL, ch.from_numpy(IDS.view(np.int64)).to(DEV), SEED, EPOCH, alpha, sigma,
                    dst_stride=stride)
    out = dbuf.cpu().numpy()
    body = out[5:5 + B * stride].reshape(B, stride)
    assert (out[:5] == 0xA5).all() and (out[5 + B * stride:] == 0xA5).all() and (body[:, img:] == 0xA5).all()
    return body[:, :img].reshape(imgs.shape)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_kernel_matches_numpy(case, mode):
    """Each case's tiles run staged, except at alpha 4096, where footprints
    exceed the budget and tiles read global memory; alpha = 0 is a copy."""
    shape, sigma, alpha = case
    H, W = shape
    th, tw = L.elastic_tile_shape()
    sizes = np.array([[L.elastic_tile_bytes(H, W, mode, int(i), SEED, EPOCH, alpha, sigma, r, c)
                       for r in range(-(-H // th)) for c in range(-(-W // tw))] for i in IDS[:2]])
    lds = L.elastic_tile_lds()
    assert (sizes > lds).any() == (alpha == 4096.0) and ((sizes > 0) & (sizes <= lds)).any(), sizes
    imgs = inputs(shape)
    got = _device_warp(imgs, mode, alpha, sigma)
    want = expected(case, mode)
    bad = [k for k in range(len(imgs)) if not np.array_equal(got[k], want[k])]
    assert not bad, (case, mode, bad)
    if alpha == 50.0:
        assert np.array_equal(_device_warp(imgs, mode, 0.0, sigma), imgs)


@pytest.mark.parametrize('interpolation', ('bilinear', 'nearest'))
def test_device_loader_matches_cpu_loader(tmp_path, interpolation):
    """32 x 32 raw, 64 samples, two epochs, launch groups of two."""
    fn = write(str(tmp_path / 'elastic.beton'), NaturalDS(64, hw=(32, 32), seed=4),
               {'image': RGBImageField(write_mode='raw'), 'label': IntField()})

    def ops():
        return [SimpleRGBImageDecoder(), ElasticTransform(50.0, 5.0, interpolation, FILL), ToTensor()]
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
