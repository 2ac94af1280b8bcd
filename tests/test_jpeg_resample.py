"""The crop decoders' interpolation='bilinear' | 'bicubic' without a GPU
(DESIGN.md s31): the argument, the predicate, the host entry against the
statement (tests/resample_ref.py on the CPU decode) and CPU Loaders over a
file that mixes JPEG and raw samples of varying size."""
import os
import tempfile

import numpy as np
import pytest

from ffcv_amd import libffcv as L
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import CenterCropRGBImageDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.synthetic import encode_jpeg, natural_image
from tests import resample_ref as R
from tests.helpers import ConstDS, NaturalDS, samples_of, write

MODES = ('bilinear', 'bicubic')


def test_interpolation_is_validated_and_area_is_the_default():
    for make in (lambda **kw: RandomResizedCropRGBImageDecoder((8, 8), **kw),
                 lambda **kw: CenterCropRGBImageDecoder((8, 8), 0.9, **kw)):
        assert make().interpolation == make(interpolation='area').interpolation == 'area'
        assert [make(interpolation=m).interpolation for m in MODES] == list(MODES)
        for bad in ('lanczos', 'AREA', 1, None):
            with pytest.raises(ValueError, match='interpolation'):
                make(interpolation=bad)


def test_area_builds_the_same_pipeline(hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.transforms import ToTensor
    fn = write(os.path.join(tempfile.mkdtemp(), 'c.beton'), ConstDS(6, size_range=(20, 40)),
               {'index': IntField(), 'value': RGBImageField(write_mode='jpg')})
    sig = []
    for kw in ({}, {'interpolation': 'area'}):
        ld = Loader(fn, batch_size=3, device='cpu', seed=3, pipelines={
            'value': [RandomResizedCropRGBImageDecoder((16, 16), **kw), ToTensor()]})
        sig.append((ld.graph.allocation_signature(), [np.asarray(v) for v, *_ in ld]))
    assert sig[0][0] == sig[1][0] and all(np.array_equal(a, b) for a, b in zip(sig[0][1], sig[1][1]))


def test_predicate_holds_on_the_promised_range_and_not_beyond(hip_lib):
    sides = (1, 2, 127, 128, 129, 255, 256, 300, 511, 512)
    outs = sorted({1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 223, 224, 255, 256})
    bad = [(h, w, o, m) for m in MODES for h in sides for w in sides for o in outs
           if not L.jpeg_resample_fits(h, w, o, o, m)]
    bad += [(512, 512, o, m) for m in MODES for o in range(1, 257) if not L.jpeg_resample_fits(512, 512, o, o, m)]
    assert not bad, bad[:8]
    assert not L.jpeg_resample_fits(300, 4000, 224, 224, 'bilinear')
    assert not L.jpeg_resample_fits(0, 10, 8, 8, 'bicubic')


def test_a_source_outside_the_predicate_is_refused_at_declare_time(hip_lib):
    from ffcv_amd.loader import Loader
    fn = write(os.path.join(tempfile.mkdtemp(), 'w.beton'), ConstDS(2, hw=(8, 4000)),
               {'index': IntField(), 'value': RGBImageField(write_mode='raw')})
    with pytest.raises(ValueError, match='ffcv_jpeg_resample_fits'):
        Loader(fn, batch_size=2, device='cpu', pipelines={
            'value': [CenterCropRGBImageDecoder((224, 224), 1.0, interpolation='bicubic')]})


@pytest.mark.parametrize('mode', MODES)
def test_host_entry_is_the_statement(hip_lib, mode):
    rng = np.random.default_rng(7)
    cases = [((17, 23), '4:2:0', (1, 1, 15, 21)), ((40, 33), '4:2:2', (3, 5, 30, 25)), ((40, 33), '4:4:4', (3, 5, 30, 25)),
             ((40, 33), 'gray', (3, 5, 30, 25)), ((24, 24), '4:2:0', (10, 9, 3, 3)), ((30, 21), 'raw', (2, 3, 27, 17))]
    imgs = [natural_image(rng, h, w) for (h, w), _, _ in cases]
    blobs = [np.ascontiguousarray(im).reshape(-1) if s == 'raw' else
             encode_jpeg(im[..., 1].copy() if s == 'gray' else im, 90, '4:2:0' if s == 'gray' else s)
             for im, (_, s, _) in zip(imgs, cases)]
    hs, ws = [c[0][0] for c in cases], [c[0][1] for c in cases]
    modes = [int(c[1] == 'raw') for c in cases]
    full = np.zeros((len(cases), 40, 33, 3), np.uint8)
    for k, b in enumerate(blobs):   # the pinned full decode of each sample
        one = np.zeros((1, hs[k], ws[k], 3), np.uint8)
        assert L.cpu_decode_batch([b], hs[k:k + 1], ws[k:k + 1], modes[k:k + 1], one)[0] == 0
        full[k, :hs[k], :ws[k]] = one[0]
    crops = np.array([c[2] for c in cases], np.int32)
    out = np.full((len(cases), 12, 9, 3), 7, np.uint8)
    status = L.cpu_decode_resample_batch(blobs, hs, ws, modes, out, crops, mode, 40, 33, nthreads=3)
    assert (status == 0).all()
    for k in range(len(cases)):
        want = R.resample(full[k, :hs[k], :ws[k]], crops[k], 12, 9, mode)
        assert np.array_equal(out[k], want), (cases[k], np.argwhere(out[k] != want)[:4])


@pytest.mark.parametrize('decoder', ('rrc', 'center'))
def test_cpu_loader_over_a_mixed_file_is_the_statement(hip_lib, decoder):
    from ffcv_amd.loader import Loader
    from ffcv_amd.transforms import ToTensor
    np.random.seed(3)   # 'proportion' draws the write mode per sample
    fn = write(os.path.join(tempfile.mkdtemp(), 'p.beton'), NaturalDS(12, hw=(60, 72), var=True, seed=2),
               {'image': RGBImageField(write_mode='proportion', compress_probability=0.5), 'label': IntField()})
    smp = samples_of(fn)
    assert {s[3] for s in smp} == {0, 1} and len({s[1:3] for s in smp}) > 4
    mode = 'bicubic' if decoder == 'rrc' else 'bilinear'
    dec = RandomResizedCropRGBImageDecoder((20, 24), interpolation=mode) if decoder == 'rrc' else \
        CenterCropRGBImageDecoder((20, 24), 0.8, interpolation=mode)
    ld = Loader(fn, batch_size=5, device='cpu', seed=9, drop_last=False, pipelines={
        'image': [dec, ToTensor()]})
    got = np.concatenate([np.asarray(im) for im, *_ in ld])
    ids = np.arange(len(smp), dtype=np.uint64)
    dp = dec._draw_params(9, 0, 20, 24)
    crops = np.empty((len(smp), 4), np.int32)
    L.draw_batch_host(ids, [s[1] for s in smp], [s[2] for s in smp], dp, crops)
    for k, (b, h, w, m) in enumerate(smp):
        full = np.zeros((1, h, w, 3), np.uint8)
        L.cpu_decode_batch([b], [h], [w], [m], full)
        assert np.array_equal(got[k], R.resample(full[0], crops[k], 20, 24, mode)), k
