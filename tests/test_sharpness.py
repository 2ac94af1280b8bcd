"""RandomAdjustSharpness on the host (no GPU): the numpy statement
(tests/sharpness_ref.py) against Pillow itself, the host twins of the C ABI
against the statement bit for bit (mixed apply codes 0 / 1 / 2, a pre-filled
dst), the order fixture (tests/golden/sharpness_order.npz, written by
tests/golden/make_sharpness_order.py), argument checks, the public name, and a
CPU Loader."""
import ctypes
import os

import numpy as np
import pytest

from tests import sharpness_ref as R
from tests.helpers import NaturalDS, write

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sharpness_order.npz')
FIXED_SHAPES = ((1, 1), (1, 7), (2, 5), (3, 3), (3, 4), (40, 40), (40, 1), (5, 2))


@pytest.fixture(scope='module')
def cases():
    """(image, per-factor statement results): 7 images (random, all-0,
    all-255, checkerboard, random) of each fixed shape and of 24 random shapes
    with H and W in 1 .. 40: 224 images, each at the eight factors."""
    rng = np.random.default_rng(1905)
    shapes = list(FIXED_SHAPES) + [tuple(int(v) for v in rng.integers(1, 41, 2)) for _ in range(24)]
    out = []
    for shape in shapes:
        for img in R.make_inputs(rng, shape):
            out.append((img, [R.sharpen(img, f) for f in R.FACTORS]))
    assert len(out) >= 200
    return out


def test_statement_matches_pillow(cases):
    """Every image at every factor, bit for bit; nothing skipped or tolerated."""
    n = 0
    for img, wants in cases:
        for f, want in zip(R.FACTORS, wants):
            assert np.array_equal(R.pillow_sharpen(img, f), want), (img.shape, f)
            n += 1
    assert n >= 1600
    # the statement is not the identity, smooths at 0, and keeps the outer ring
    img, wants = next(c for c in cases if c[0].shape == (40, 40, 3))
    assert np.array_equal(wants[R.FACTORS.index(1)], img)
    for want in (wants[0], wants[-1]):
        assert not np.array_equal(want, img)
        assert np.array_equal(want[0], img[0]) and np.array_equal(want[:, -1], img[:, -1])


def test_host_twin_matches_statement(hip_lib, cases):
    """The same images in batches of one shape, codes 0 / 1 / 2 / 7 mixed, into
    a dst pre-filled with 0x5A: code 2 leaves it alone."""
    from ffcv_amd import libffcv as L
    by_shape = {}
    for img, wants in cases:
        by_shape.setdefault(img.shape, []).append((img, wants))
    for shape, group in by_shape.items():
        imgs = np.stack([g[0] for g in group])
        B = len(imgs)
        apply = np.resize(R.mixed_apply(), B)
        for fi, f in enumerate(R.FACTORS + (16,)):
            factor = np.full(B, f, np.float32)
            got = np.full_like(imgs, 0x5A)
            L.sharpness_batch_host(imgs, got, apply, factor, nthreads=3)
            for k in range(B):
                if apply[k] == R.LEAVE:
                    assert (got[k] == 0x5A).all()
                elif apply[k] == R.SHARPEN:
                    want = group[k][1][fi] if f != 16 else R.sharpen(imgs[k], 16)
                    assert np.array_equal(got[k], want), (shape, f, k)
                else:
                    assert np.array_equal(got[k], imgs[k])
    # per-image factors
    imgs = np.stack([c[0] for c in cases if c[0].shape == (40, 40, 3)])
    factor = np.linspace(0, 2, len(imgs)).astype(np.float32)
    got = np.zeros_like(imgs)
    L.sharpness_batch_host(imgs, got, np.ones(len(imgs), np.uint8), factor)
    assert np.array_equal(got, R.sharpen_batch(imgs, np.ones(len(imgs)), factor, got))


def test_draw_twin_matches_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    ids = np.arange(256, dtype=np.uint64)
    for seed, epoch, p, f in ((5, 0, 0.5, 2.0), (2 ** 63 + 1, 3, 0.1, 0.3), (0, 1, 1.0, 16), (9, 9, 0.0, 0)):
        apply, factor = L.sharpness_draw_batch_host(ids, seed, epoch, p, f)
        assert apply.dtype == np.uint8 and factor.dtype == np.float32
        assert np.array_equal(apply, [R.draw(seed, epoch, i, p) for i in range(256)])
        assert (factor.view(np.uint32) == np.float32(f).view(np.uint32)).all()
        assert (0 < apply.sum() < 256) if 0 < p < 1 else (apply == p).all()


def test_entries_reject_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ptr = lambda x, off=0: ctypes.c_void_p(x.ctypes.data + off)  # noqa: E731
    ids = np.arange(2, dtype=np.uint64)
    a, f = np.full(2, 9, np.uint8), np.full(2, 9, np.float32)
    for p, fac in ((-0.1, 1.0), (1.5, 1.0), (float('nan'), 1.0), (0.5, -0.01), (0.5, 16.5), (0.5, float('nan')),
                   (0.5, float('inf'))):
        assert lib.ffcv_sharpness_draw_batch_host(ptr(ids), 2, 0, 0, p, fac, ptr(a), ptr(f)) == -1
        assert b'ffcv_sharpness_draw_batch_host' in lib.ffcv_last_error()
        assert lib.ffcv_sharpness_draw_batch(None, ptr(ids), 2, 0, 0, p, fac, ptr(a), ptr(f), None) == -1
    assert lib.ffcv_sharpness_draw_batch_host(None, 2, 0, 0, 0.5, 1.0, ptr(a), ptr(f)) == -1
    assert lib.ffcv_sharpness_draw_batch_host(ptr(ids), 2, 0, 0, 0.5, 1.0, ptr(a), None) == -1
    assert (a == 9).all() and (f == 9).all()

    src = np.full((2, 6, 5, 3), 77, np.uint8)
    dst = np.full((3, 6, 5, 3), 66, np.uint8)
    apply, factor = np.ones(2, np.uint8), np.ones(2, np.float32)

    def call(s=None, d=None, h=6, wd=5, stride=0, ap=apply, fa=factor, batch=2, entry='host'):
        s = ptr(src) if s is None else s
        d = ptr(dst) if d is None else d
        ap = None if ap is None else ptr(ap)
        fa = None if fa is None else ptr(fa)
        if entry == 'host':
            return lib.ffcv_sharpness_batch_host(s, d, batch, h, wd, ap, fa, stride, 1)
        return lib.ffcv_sharpness_batch(None, s, d, batch, h, wd, ap, fa, stride)
    for entry, name in (('host', b'ffcv_sharpness_batch_host'), ('device', b'ffcv_sharpness_batch')):
        for kw in (dict(h=0), dict(wd=-1), dict(wd=65536), dict(h=65536), dict(batch=-1), dict(ap=None),
                   dict(fa=None), dict(s=ctypes.c_void_p(0)), dict(d=ctypes.c_void_p(0)), dict(stride=89),
                   dict(d=ptr(src)), dict(d=ptr(src, 90)), dict(d=ptr(src, 179)), dict(s=ptr(dst, 90), stride=90)):
            assert call(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
        assert b'overlap' in lib.ffcv_last_error()
    assert (src == 77).all() and (dst == 66).all()
    assert call() == 0 and call(stride=135) == 0 and call(batch=0) == 0
    assert L.sharpness_lds_bytes() >= 6 * 32 * 32 and L.sharpness_band_rows() >= 1
    assert L.sharpness_strip_cols(32, 32) == 32 and L.sharpness_strip_cols(0, 5) == 0
    with pytest.raises(TypeError):
        L.sharpness_batch_host(src[:, :, :, :2], dst, apply, factor)
    with pytest.raises(TypeError):
        L.sharpness_batch_host(src, dst, apply[:1], factor)


def test_order_fixture(hip_lib):
    """Pillow's own centre bytes on 3 x 3 neighbourhoods where a blend
    contracted to a fused multiply-add gives another byte in every channel."""
    from ffcv_amd import libffcv as L
    z = np.load(GOLDEN)
    tiles, factor, want, fma = z['tiles'], z['factor'], z['want'], z['fma']
    assert tiles.shape[1:] == (3, 3, 3) and len(tiles) >= 32 and factor.dtype == np.float32
    assert (want != fma).all()
    got = np.empty_like(tiles)
    L.sharpness_batch_host(tiles, got, np.ones(len(tiles), np.uint8), factor)
    assert np.array_equal(got[:, 1, 1], want)
    for k in range(len(tiles)):
        assert np.array_equal(R.sharpen(tiles[k], factor[k])[1, 1], want[k])
        assert np.array_equal(R.sharpen(tiles[k], factor[k], fma=True)[1, 1], fma[k])
        assert np.array_equal(R.pillow_sharpen(tiles[k], float(factor[k]))[1, 1], want[k])


def test_public_name_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls = T.RandomAdjustSharpness
    assert FT.RandomAdjustSharpness is cls and 'RandomAdjustSharpness' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_SHARPNESS
    op = cls(2)
    assert op.sharpness_factor == 2.0 and op.p == 0.5
    assert cls(0, 1).sharpness_factor == 0 and cls(16, 0).sharpness_factor == 16 and cls(np.float32(1.5)).p == 0.5
    for bad in (-0.01, 16.01, float('nan'), float('inf'), None, 'x', True, (1, 2)):
        with pytest.raises(ValueError, match='RandomAdjustSharpness'):
            cls(bad)
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError, match='RandomAdjustSharpness'):
            cls(2, p=bad)


def test_state_is_out_of_place_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomAdjustSharpness
    op = RandomAdjustSharpness(2)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(2, 6, 3)))
    assert isinstance(alloc, AllocationQuery) and tuple(alloc.shape) == (2, 6, 3) and st.shape == (2, 6, 3)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
    assert alloc.device == ch.device('cuda:0') and alloc.dtype == ch.uint8 and st.device.type == 'cuda'
    for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('f4'), (8, 6, 3)),
                      (np.dtype('u1'), (8, 6)), (np.dtype('u1'), (8, 6, 4))):
        with pytest.raises(TypeError, match='RandomAdjustSharpness'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_graph_keeps_launch_groups(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, RandomAdjustSharpness
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    ops = [SimpleRGBImageDecoder(), RandomAdjustSharpness(2), RandomHorizontalFlip(), ToTensor(),
           ToDevice(ch.device('cuda:0'), non_blocking=True)]
    r = Reader(raw)
    g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
              r.metadata, OSCacheManager(r).compile_reader(), device='cuda:0')
    g.collect_requirements()
    assert g.groupable()
    assert not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes)
    assert not ops[1]._absorbed


def test_cpu_loader(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandomAdjustSharpness
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'sharp.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed = 12
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomAdjustSharpness(2, p=0.5), ToTensor()]})
    for epoch in range(2):
        applied = seen = 0
        for b, (images, labels) in enumerate(loader):
            got = images.numpy()
            assert got.shape == (8, 32, 32, 3) and got.dtype == np.uint8
            for k in range(8):
                sid = b * 8 + k
                on = R.draw(seed, epoch, sid, 0.5)
                want = R.sharpen(ds.imgs[sid], 2) if on else ds.imgs[sid]
                assert np.array_equal(got[k], want), (epoch, sid, on)
                assert not on or not np.array_equal(got[k], ds.imgs[sid])
                applied += on
                seen += 1
        assert seen == 24 and 0 < applied < 24
