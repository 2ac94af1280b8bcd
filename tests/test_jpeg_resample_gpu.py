"""The crop decoders' 'bilinear' / 'bicubic' launches on the MI355X
(DESIGN.md s31), every byte against the statement: the CPU decode
(L.cpu_decode_batch, pinned to libjpeg-turbo) followed by
tests/resample_ref.py's resample.  Outputs land in 0xA5-guarded buffers with a
padded stride."""
import io
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.synthetic import encode_jpeg, natural_image, pack
from tests import large_batch as LB
from tests import resample_ref as R
from tests.helpers import NaturalDS, write

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = ('bilinear', 'bicubic')

# format, (H, W), window (i, j, h, w) or None for the whole image, (out_h, out_w): what it breaks
CASES = [
    ('4:2:0', (17, 23), (1, 1, 15, 21), (8, 8)),       # odd origin against the chroma quad; partial MCUs; image-edge replication
    ('4:2:0', (3, 3), None, (5, 5)),                   # the cw <= 2 upsampling branch; a single tap
    ('4:2:0', (16, 16), None, (16, 16)),               # the identity: output equals the decode
    ('4:2:2', (40, 33), (3, 5, 30, 25), (12, 12)),     # the general colour path
    ('4:4:4', (40, 33), (3, 5, 30, 25), (12, 12)),
    ('gray', (40, 33), (3, 5, 30, 25), (12, 12)),
    ('4:2:0', (24, 24), (10, 9, 3, 3), (32, 32)),      # upscale; every record clipped at the window, not the image
    ('4:2:0', (200, 168), (40, 50, 97, 111), (64, 64)),  # several bands, every band boundary; chunks starting on odd rows
    ('4:2:0', (256, 256), None, (4, 4)),               # scale 64: the ring wraps, a record is longer than a chunk
    ('4:2:0', (48, 512), None, (8, 224)),              # the widest staged rows and column records of the predicate
    ('4:2:0', (512, 512), None, (256, 256)),           # the corners of the predicate
    ('4:2:0', (512, 512), None, (1, 1)),
]
IDS = [f'{c[0]}-{c[1][0]}x{c[1][1]}-{c[3][0]}x{c[3][1]}' for c in CASES]


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


def blob_of(case):
    """(stream, its CPU decode, window) of a case."""
    fmt, (H, W), window, _ = case
    img = natural_image(np.random.default_rng(H * 1000 + W), H, W)
    blob = encode_jpeg(img[..., 1].copy() if fmt == 'gray' else img, 90, '4:2:0' if fmt == 'gray' else fmt)
    return blob, decode(blob, H, W, 0), window or (0, 0, H, W)


def decode(blob, h, w, mode):
    full = np.zeros((1, h, w, 3), np.uint8)
    assert L.cpu_decode_batch([blob], [h], [w], [mode], full)[0] == 0
    return full[0]


def table(blobs, shapes, modes):
    """(device bytes, device ffcv_sample[n]) of samples packed one after another."""
    buf, offs, sizes = pack(blobs)
    smp = np.zeros(len(blobs), L.SAMPLE_DTYPE)
    smp['offset'], smp['size'], smp['mode'] = offs, sizes, modes
    smp['height'], smp['width'] = [s[0] for s in shapes], [s[1] for s in shapes]
    return LB.dev(buf), LB.dev(smp.view(np.uint8))


def run(launch, B, oh, ow, pad=7):
    """launch(out, stride, status) into guarded memory: (images (B, oh, ow, 3), status)."""
    dense, stride = oh * ow * 3, oh * ow * 3 + pad
    dst = LB.DevBuf(B * stride, 3)
    status = ch.full((B,), -1, dtype=ch.int32, device=DEV)
    launch(dst.flat, stride, status)
    ch.cuda.synchronize()
    got = dst.flat.cpu().numpy().reshape(B, stride)
    assert dst.guards_ok() and (got[:, dense:] == LB.FILL_BYTE).all()
    return got[:, :dense].reshape(B, oh, ow, 3), status.cpu().numpy()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_entry_is_the_statement(case, mode):
    """Two windows of one image: the case's, and the same one row and column shorter."""
    (H, W), (oh, ow) = case[1], case[3]
    blob, full, (i, j, h, w) = blob_of(case)
    wins = [(i, j, h, w), (i, j, max(h - 1, 1), max(w - 1, 1))]
    d_buf, d_smp = table([blob] * 2, [(H, W)] * 2, 0)
    dec = L.JpegDecoder(2, H, W, len(blob))
    got, status = run(lambda o, s, st: dec.resample(d_buf, d_smp, 2, LB.dev(np.array(wins, np.int32)), mode, oh, ow,
                                                    o, s, st), 2, oh, ow)
    assert (status == 0).all()
    for k in range(2):
        want = R.resample(full, wins[k], oh, ow, mode)
        assert np.array_equal(got[k], want), (k, np.argwhere(got[k] != want)[:4])
    if (h, w) == (oh, ow):
        assert np.array_equal(got[0], full[i:i + h, j:j + w])


@pytest.mark.parametrize('mode', MODES)
def test_a_ragged_batch_keeps_each_image_its_own_geometry(mode):
    """Every case's image in ONE launch (context of 512 x 512), all to 24 x 40."""
    items = [blob_of(c) for c in CASES]
    d_buf, d_smp = table([it[0] for it in items], [c[1] for c in CASES], 0)
    dec = L.JpegDecoder(len(items), 512, 512, max(len(it[0]) for it in items))
    crops = LB.dev(np.array([it[2] for it in items], np.int32))
    got, status = run(lambda o, s, st: dec.resample(d_buf, d_smp, len(items), crops, mode, 24, 40, o, s, st),
                      len(items), 24, 40)
    assert (status == 0).all()
    for k, (_, full, win) in enumerate(items):
        assert np.array_equal(got[k], R.resample(full, win, 24, 40, mode)), IDS[k]


def test_failed_samples_are_zero_and_leave_their_neighbours_exact():
    from PIL import Image
    img = natural_image(np.random.default_rng(1), 64, 80)
    good = encode_jpeg(img)
    b = io.BytesIO()
    Image.fromarray(img).save(b, format='JPEG', progressive=True)
    blobs = [good, np.frombuffer(b.getvalue(), np.uint8), good, good[:len(good) // 2], good]
    d_buf, d_smp = table(blobs, [(64, 80)] * 5, 0)
    dec = L.JpegDecoder(5, 64, 80, max(len(x) for x in blobs))
    wins = np.array([(3, 5, 50, 60)] * 5, np.int32)
    got, status = run(lambda o, s, st: dec.resample(d_buf, d_smp, 5, LB.dev(wins), 'bicubic', 20, 20, o, s, st),
                      5, 20, 20)
    area = ch.full((5,), -1, dtype=ch.int32, device=DEV)   # today's codes: the area launch's
    p = L.RRCParams()
    p.out_h = p.out_w = 20
    dec.rrc(d_buf, d_smp, 5, LB.dev(wins), None, None, p, ch.empty(5 * 1200, dtype=ch.uint8, device=DEV), area)
    assert status.tolist() == area.cpu().tolist() and status[1] == 2 and status[3] != 0 and status[0] == 0
    want = R.resample(decode(good, 64, 80, 0), wins[0], 20, 20, 'bicubic')
    assert (got[1] == 0).all() and (got[3] == 0).all()
    assert all(np.array_equal(got[k], want) for k in (0, 2, 4))


def test_raw_entry_serves_the_raw_samples_and_skips_the_others():
    rng = np.random.default_rng(3)
    shapes = [(30, 21), (64, 80), (17, 100), (9, 9)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    blobs = [imgs[0].reshape(-1), encode_jpeg(imgs[1]), imgs[2].reshape(-1), imgs[3].reshape(-1)]
    d_buf, d_smp = table(blobs, shapes, [1, 0, 1, 1])
    wins = np.array([(2, 3, 27, 17), (0, 0, 64, 80), (1, 0, 16, 99), (0, 0, 9, 9)], np.int32)
    got, _ = run(lambda o, s, st: L.resample_raw_batch(d_buf, d_smp, 4, LB.dev(wins), 'bicubic', 40, 12, o, s, 64, 100),
                 4, 40, 12)
    assert (got[1] == LB.FILL_BYTE).all()
    for k in (0, 2, 3):
        assert np.array_equal(got[k], R.resample(imgs[k], wins[k], 40, 12, 'bicubic')), k


@pytest.mark.parametrize('device_cache', (True, False), ids=('hbm', 'staged'))
@pytest.mark.parametrize('decoder', ('rrc-bicubic', 'center-bilinear', 'rrc-bicubic-flip-norm'))
def test_device_loader_matches_cpu_loader(decoder, device_cache):
    """Two epochs over 40 samples of varying size, JPEG and raw mixed, in launch groups of two."""
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import CenterCropRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
    from ffcv_amd.loader import Loader
    from ffcv_amd.loader.epoch_iterator import launch_group
    from ffcv_amd.transforms import NormalizeImage, RandomHorizontalFlip, ToDevice, ToTensor, ToTorchImage
    np.random.seed(5)   # 'proportion' draws the write mode per sample
    fn = write(os.path.join(tempfile.mkdtemp(), 'p.beton'), NaturalDS(40, hw=(100, 120), var=True, seed=6),
               {'image': RGBImageField(write_mode='proportion'), 'label': IntField()})
    tail = decoder.endswith('flip-norm')

    def ops():
        dec = CenterCropRGBImageDecoder((48, 56), 0.875, interpolation='bilinear') if decoder.startswith('center') \
            else RandomResizedCropRGBImageDecoder((48, 56), interpolation='bicubic')
        post = [RandomHorizontalFlip(), NormalizeImage(np.array([120., 110., 100.]), np.array([60., 61., 62.]),
                                                       np.float16)] if tail else []
        return dec, post
    dec, post = ops()
    cpu = Loader(fn, batch_size=8, device='cpu', seed=12, drop_last=False, pipelines={'image': [dec] + post + [ToTensor()]})
    dec, post = ops()   # (on the device NormalizeImage takes the NCHW view; the host table works on HWC)
    dev = Loader(fn, batch_size=8, seed=12, drop_last=False, device_cache=device_cache, batches_per_launch=2,
                 pipelines={'image': [dec, ToTensor(), ToDevice(DEV)] + post[:1] + ([ToTorchImage()] if tail else [])
                            + post[1:], 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]})

    def hwc(im):
        a = np.asarray(im.cpu())
        return a.view(np.float16) if a.dtype == np.int16 else (a.transpose(0, 2, 3, 1) if tail else a)
    epochs = [[np.concatenate([hwc(im) for im, *_ in ld]) for _ in range(2)] for ld in (cpu, dev)]
    assert not np.array_equal(epochs[0][0], epochs[0][1]) or decoder.startswith('center')
    for want, got in zip(*epochs):
        assert got.shape[1:] == (48, 56, 3) and got.dtype == (np.float16 if tail else np.uint8)
        assert np.array_equal(got, want)
    assert dev.graph.groupable() and launch_group(dev, len(dev)) == 2
    assert not dec._epilogue and not any(getattr(o, '_absorbed', False) for o in post)   # they ran as their own launches
