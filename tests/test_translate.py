"""RandomTranslate on the host (no GPU): the public names, argument checks,
the reference's own outputs (tests/golden/translate.npz, written by
tests/golden/make_translate.py from the reference's translate.py), the host
draw twin of the C ABI against numpy's legacy RandomState under the seeding
contract (op id 4), and a CPU Loader running flip -> translate -> cutout."""
import os

import numpy as np
import pytest

from tests.helpers import NaturalDS, write
from tests.translate_ref import apply_chain, translate_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'translate.npz')


def test_public_names_and_arguments():
    from ffcv_amd.transforms import RandomTranslate
    from ffcv.transforms import RandomTranslate as Aliased
    import ffcv_amd.transforms as T
    assert Aliased is RandomTranslate and 'RandomTranslate' in T.__all__
    op = RandomTranslate(2, (125, 123, 114))
    assert op.padding == 2 and op.fill_u8().tolist() == [125, 123, 114]
    assert RandomTranslate(0).fill_u8().tolist() == [0, 0, 0]
    assert RandomTranslate(np.int64(3), 7).fill_u8().tolist() == [7, 7, 7]  # broadcast like Cutout
    assert RandomTranslate(1000).padding == 1000                           # larger than any image: allowed
    for bad in (-1, 1.5, '2', None, True):
        with pytest.raises(ValueError):
            RandomTranslate(bad)
    assert RandomTranslate.per_sample and RandomTranslate.device_aware


def test_reference_offsets_are_legacy_randint():
    """Every recorded row: RandomState(seed) drawing randint(2p + 1) twice
    gives the reference's (y, x), y first."""
    rows = np.load(GOLDEN)['rows']
    assert len(rows) >= 2000
    assert rows[:, 1].min() == 1 and rows[:, 1].max() == 64 and rows[:, 2].max() == 64
    assert (rows[:, 3] == 0).any() and (rows[:, 3] > rows[:, 1]).any() and (rows[:, 3] > rows[:, 2]).any()
    for seed, h, w, p, y, x in rows.tolist():
        rs = np.random.RandomState(seed)
        assert (rs.randint(2 * p + 1), rs.randint(2 * p + 1)) == (y, x), (seed, h, w, p)


def test_host_translate_reproduces_reference_images():
    from ffcv_amd.transforms.translate import translate_window
    z = np.load(GOLDEN)
    meta = z['meta']
    assert len(meta) >= 24
    whole_fill = 0
    for k, (seed, p, f0, f1, f2) in enumerate(meta.tolist()):
        img, want = z[f'in_{k}'], z[f'out_{k}']
        assert img.shape[0] <= 16 and img.shape[1] <= 16 and (f0, f1, f2) != (0, 0, 0) and img.std() > 0
        rs = np.random.RandomState(seed)
        y, x = rs.randint(2 * p + 1), rs.randint(2 * p + 1)
        fill = np.array([f0, f1, f2], np.uint8)
        got = translate_window(img, np.empty_like(img), y, x, p, fill)
        assert np.array_equal(got, want), k
        assert np.array_equal(translate_np(img, y, x, p, fill), want), k  # the tests' own numpy statement
        whole_fill += bool((want == fill).all())
    assert whole_fill >= 1  # a window that misses the image entirely is among them


def test_host_draw_twin_matches_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.rng import contract_seed
    rng = np.random.default_rng(11)
    n = 5000
    seeds = rng.integers(0, 2 ** 63, n)
    epochs = rng.integers(0, 1000, n)
    ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    ids[:8] = np.arange(8)
    seeds[:4], epochs[:4] = 0, 0
    for p in (0, 1, 2, 7, 40):
        want = np.empty((n, 2), np.int32)
        got = np.empty((n, 2), np.int32)
        for k in range(n):
            rs = np.random.RandomState(contract_seed(int(seeds[k]), int(epochs[k]), int(ids[k]), 4))
            want[k, 0] = rs.randint(2 * p + 1)
            want[k, 1] = rs.randint(2 * p + 1)
            got[k] = L.translate_draw_batch_host(ids[k:k + 1], int(seeds[k]), int(epochs[k]), p)[0]
        assert np.array_equal(got, want), p
        assert want.min() == 0 and want.max() == 2 * p
    # one call over a batch (one seed / epoch) gives the per-sample values
    batch = L.translate_draw_batch_host(ids[:64], 5, 3, 7)
    for k in range(64):
        rs = np.random.RandomState(contract_seed(5, 3, int(ids[k]), 4))
        assert (rs.randint(15), rs.randint(15)) == tuple(batch[k].tolist())
    assert hip_lib.ffcv_translate_draw_batch_host(None, 1, 0, 0, 1, None) == -1
    assert b'ffcv_translate_draw_batch_host' in hip_lib.ffcv_last_error()


def test_graph_lowers_simple_chains_with_translate_only(tmp_path):
    """Lowering decisions (no kernel launched): a plain Simple decoder of raw
    samples is fused exactly when the chain holds a RandomTranslate; the
    absorbed operations run as identities and the decoder hands out fp16 when
    the LUT went in; JPEG samples, a chain without translate, a repeated
    operation and an operation behind the layout change stay staged."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, NormalizeImage, ToTensor, ToDevice, ToTorchImage,
                                     RandomHorizontalFlip, RandomTranslate)
    fields = lambda mode: {'image': RGBImageField(write_mode=mode), 'label': IntField()}  # noqa: E731
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)), fields('raw'))
    jpg = write(str(tmp_path / 'jpg.beton'), NaturalDS(6, hw=(32, 32)), fields('jpg'))
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])

    def graph(fn, ops):
        r = Reader(fn)
        g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                  r.metadata, OSCacheManager(r).compile_reader(), device='cuda:0')
        return g, g._chains['image'][0]

    def cifar():
        return [SimpleRGBImageDecoder(), RandomHorizontalFlip(), RandomTranslate(2, (125, 123, 114)),
                Cutout(4, (125, 123, 114)), ToTensor(), ToDevice(ch.device('cuda:0'), non_blocking=True),
                ToTorchImage(), NormalizeImage(mean, std, np.float16)]
    ops = cifar()
    g, dec = graph(raw, ops)
    assert dec.fused and list(dec._fused_steps) == ops[1:4] and dec._fused_normalize is ops[7]
    assert all(o._absorbed for o in ops[1:4] + [ops[7]]) and dec.output_dtype == ch.float16
    g.collect_requirements()
    last = g.states[g.outputs['image'].id]
    assert last.dtype == ch.float16 and tuple(last.shape) == (3, 32, 32) and last.device.type == 'cuda'
    assert g.groupable()
    names = [name for name, alloc in g.allocation_signature() if alloc is not None]
    assert names == ['SimpleRGBImageDecoder']  # the absorbed operations own no buffers

    ops = cifar()
    g, dec = graph(jpg, ops)                      # JPEG samples: nothing absorbed
    assert not dec.fused and not any(o._absorbed for o in ops[1:4] + [ops[7]])
    ops = cifar()
    del ops[2]
    g, dec = graph(raw, ops)                      # no translate: today's staged launches
    assert not dec.fused and not any(getattr(o, '_absorbed', False) for o in ops[1:])
    ops = [SimpleRGBImageDecoder(), RandomTranslate(1), RandomTranslate(2), Cutout(4)]
    g, dec = graph(raw, ops)                      # each operation at most once
    assert list(dec._fused_steps) == ops[1:2] and not ops[2]._absorbed and not ops[3]._absorbed
    ops = [SimpleRGBImageDecoder(), RandomTranslate(1), ToTensor(), ToTorchImage(), Cutout(4)]
    g, dec = graph(raw, ops)                      # not behind the layout change
    assert list(dec._fused_steps) == ops[1:2] and not ops[4]._absorbed


def test_cpu_loader_flip_translate_cutout(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, Cutout, RandomHorizontalFlip, RandomTranslate
    ds = NaturalDS(24, hw=(13, 10), seed=3)
    fn = write(str(tmp_path / 'tr.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed = 12
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), RandomTranslate(3, (9, 8, 7)),
                  Cutout(4, (200, 201, 202)), ToTensor()]})
    for epoch in range(2):
        flips = seen = 0
        for b, (images, labels) in enumerate(loader):
            got = images.numpy()
            assert got.shape == (8, 13, 10, 3) and got.dtype == np.uint8
            for k in range(8):
                sid = b * 8 + k
                want, f = apply_chain(ds.imgs[sid], 'ftc', seed, epoch, sid, pad=3, tfill=(9, 8, 7), cut=4,
                                      cfill=(200, 201, 202))
                assert np.array_equal(got[k], want), (epoch, sid)
                flips += f
                seen += 1
        assert seen == 24 and 0 < flips < 24
