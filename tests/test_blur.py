"""GaussianBlur on the host (no GPU): public name and argument checks, the
host twins of the C ABI (draws against numpy's legacy RandomState under the
seeding contract, op id 11; weights and pixels against tests/blur_ref.py, bit
for bit), the order fixture (tests/golden/blur_order.npz, written by
tests/golden/make_blur_order.py), the graph lowering, and a CPU Loader with
grayscale and solarization around the blur.

exp is the one function of the contract that is not pinned bit for bit, so
every comparison of weights first asserts, on numpy's float64 weights, that no
weight lies within a relative 2^-44 of a float32 rounding boundary
(blur_ref.guard_holds) and then demands equal float32 bits."""
import ctypes
import os

import numpy as np
import pytest

from tests import blur_ref as R
from tests.helpers import NaturalDS, write

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'blur_order.npz')
SEED = 7    # with this loader seed the guard holds for all six kernel sizes below (ids 0 .. 255, epoch 0)
# (shape, kernel sizes): every listed size has (k - 1) / 2 < min(H, W)
SHAPES = (((1, 1), (1,)), ((2, 2), (1, 3)), ((2, 9), (1, 3)), ((3, 5), (1, 3, 5)), ((16, 16), (1, 3, 5, 23, 31)),
          ((32, 32), (1, 3, 5, 23, 31)), ((33, 31), (1, 3, 5, 23, 31)))
SIGMAS = (0.1, 0.5, 2.0)


def make_inputs(rng, shape, batch=7):
    """Random images, then all-0, all-255 and a 0 / 255 checkerboard."""
    imgs = rng.integers(0, 256, (batch,) + tuple(shape) + (3,), dtype=np.uint8)
    imgs[batch - 3] = 0
    imgs[batch - 2] = 255
    yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing='ij')
    imgs[batch - 1] = (((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None]
    return imgs


def mixed_apply(batch=7):
    apply = np.ones(batch, np.uint8)
    apply[[1, 4]] = 0
    return apply


def test_public_name_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls = T.GaussianBlur
    assert FT.GaussianBlur is cls and 'GaussianBlur' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_BLUR
    op = cls(5)
    assert op.kernel_size == 5 and op.sigma == (0.1, 2.0) and op.p == 0.5
    assert cls(1, 1.5, 0).sigma == (1.5, 1.5) and cls(31, (0.5, 0.5), 1).kernel_size == 31
    for bad in (0, 2, 4, 33, -3, 3.0, None, True):
        with pytest.raises(ValueError):
            cls(bad)
    for bad in (0, -1.0, (0.0, 1.0), (2.0, 1.0), (0.1, float('inf')), float('nan'), (1.0,), 'x', None):
        with pytest.raises(ValueError):
            cls(3, bad)
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError):
            cls(3, p=bad)


def test_state_must_be_uint8_hwc_and_larger_than_the_reflection():
    import torch as ch
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import GaussianBlur
    op = GaussianBlur(5)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
    assert isinstance(alloc, AllocationQuery) and tuple(alloc.shape) == (8, 6, 3) and st.shape == (8, 6, 3)
    assert st.dtype == np.dtype('u1')
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
    assert alloc.device == ch.device('cuda:0') and alloc.dtype == ch.uint8 and st.device.type == 'cuda'
    for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('f4'), (8, 6, 3)),
                      (np.dtype('u1'), (8, 6)), (np.dtype('u1'), (8, 6, 4))):
        with pytest.raises(TypeError, match='GaussianBlur'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))
    for shape in ((2, 9, 3), (9, 2, 3)):      # (5 - 1) / 2 >= min(H, W)
        with pytest.raises(TypeError, match='GaussianBlur'):
            op.declare_state_and_memory(
                State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=shape))
    op.declare_state_and_memory(State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(3, 3, 3)))


def test_uniform_draw_twin_matches_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(12)
    n = 300
    seeds = rng.integers(0, 2 ** 63, n)
    epochs = rng.integers(0, 1000, n)
    ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    ids[:8] = np.arange(8)
    seeds[:4], epochs[:4] = 0, 0
    for op_id in (9, 10, 11):
        for p, lo, hi in ((0.5, 0.0, 0.0), (0.1, 128.0, 128.0), (0.5, 0.1, 2.0), (1.0, 256.0, 256.0), (0.0, 1.0, 3.0)):
            applies = 0
            for k in range(n):
                wa, wv = R.uniform_draw(int(seeds[k]), int(epochs[k]), int(ids[k]), op_id, p, lo, hi)
                ga, gv = L.uniform_draw_batch_host(ids[k:k + 1], int(seeds[k]), int(epochs[k]), op_id, p, lo, hi)
                assert bool(ga[0]) == wa and gv.view(np.uint64)[0] == wv.view(np.uint64), (op_id, k)
                applies += int(ga[0])
            assert applies == (n if p == 1.0 else 0) if p in (0.0, 1.0) else 0 < applies < n
        ga, gv = L.uniform_draw_batch_host(ids[:64], 5, 3, op_id, 0.5, 0.25, 0.75)
        for k in range(64):
            wa, wv = R.uniform_draw(5, 3, int(ids[k]), op_id, 0.5, 0.25, 0.75)
            assert bool(ga[k]) == wa and gv.view(np.uint64)[k] == wv.view(np.uint64)
    lib = L.lib()
    a, v = np.zeros(2, np.uint8), np.zeros(2)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    two = np.arange(2, dtype=np.uint64)
    for op_id, p, lo, hi in ((5, 0.5, 0.0, 1.0), (8, 0.5, 0.0, 1.0), (12, 0.5, 0.0, 1.0), (0, 0.5, 0.0, 1.0),
                             (9, -0.1, 0.0, 1.0), (9, 1.5, 0.0, 1.0), (9, 0.5, 1.0, 0.0), (9, 0.5, 0.0, float('inf')),
                             (9, float('nan'), 0.0, 1.0), (9, 0.5, float('nan'), 1.0)):
        assert lib.ffcv_uniform_draw_batch_host(ptr(two), 2, 0, 0, op_id, p, lo, hi, ptr(a), ptr(v)) == -1
        assert b'ffcv_uniform_draw_batch_host' in lib.ffcv_last_error()
        assert lib.ffcv_uniform_draw_batch(None, ptr(two), 2, 0, 0, op_id, p, lo, hi, ptr(a), ptr(v), None) == -1
    assert lib.ffcv_uniform_draw_batch_host(None, 2, 0, 0, 9, 0.5, 0.0, 1.0, ptr(a), ptr(v)) == -1


@pytest.mark.parametrize('ksize', (1, 3, 5, 9, 23, 31))
def test_weights_twin_matches_numpy_under_the_guard(hip_lib, ksize):
    """256 drawn sigma per kernel size: decision and sigma bit for bit against
    RandomState, then, under the guard, the float32 weights bit for bit."""
    from ffcv_amd import libffcv as L
    ids = np.arange(256, dtype=np.uint64)
    apply, sigma, weights = L.blur_draw_batch_host(ids, SEED, 0, 0.5, 0.1, 2.0, ksize)
    assert weights.shape == (256, R.WROW) and weights.dtype == np.float32
    flushed = 0
    for i in range(256):
        wa, ws = R.uniform_draw(SEED, 0, i, R.OP_BLUR, 0.5, 0.1, 2.0)
        assert bool(apply[i]) == wa and sigma.view(np.uint64)[i] == ws.view(np.uint64)
        assert R.guard_holds(ksize, ws), (ksize, i, float(ws))
        want = R.weights_f32(ksize, ws)
        assert np.array_equal(weights[i].view(np.uint32), want.view(np.uint32)), (ksize, i, float(ws))
        assert (weights[i, ksize:].view(np.uint32) == 0).all()
        flushed += bool((R.weights_f64(ksize, ws) < R.FLT_MIN).any())
        assert abs(float(weights[i].astype(np.float64).sum()) - 1) < 1e-5
    assert 0 < apply.sum() < 256 and 0.1 <= sigma.min() and sigma.max() < 2.0
    if ksize >= 23:
        assert flushed > 0      # the flush rule is exercised
    if ksize == 1:
        assert (weights[:, 0] == 1).all()


def test_blur_draw_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    ids = np.arange(2, dtype=np.uint64)
    a, s, w = np.zeros(2, np.uint8), np.zeros(2), np.full((2, 32), 9, np.float32)
    for p, lo, hi, k in ((0.5, 0.1, 2.0, 2), (0.5, 0.1, 2.0, 0), (0.5, 0.1, 2.0, 33), (0.5, 0.0, 2.0, 3),
                         (0.5, 2.0, 1.0, 3), (0.5, 0.1, float('inf'), 3), (1.5, 0.1, 2.0, 3),
                         (0.5, float('nan'), 2.0, 3)):
        assert lib.ffcv_blur_draw_batch_host(ptr(ids), 2, 0, 0, p, lo, hi, k, ptr(a), ptr(s), ptr(w)) == -1
        assert b'ffcv_blur_draw_batch_host' in lib.ffcv_last_error()
        assert lib.ffcv_blur_draw_batch(None, ptr(ids), 2, 0, 0, p, lo, hi, k, ptr(a), ptr(s), ptr(w), None) == -1
    assert lib.ffcv_blur_draw_batch_host(ptr(ids), 2, 0, 0, 0.5, 0.1, 2.0, 3, ptr(a), ptr(s), None) == -1
    assert (w == 9).all()


@pytest.mark.parametrize('shape,ksizes', SHAPES, ids=[f'{s[0]}x{s[1]}' for s, _ in SHAPES])
def test_host_twin_pixels_match_numpy(hip_lib, shape, ksizes):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    imgs = make_inputs(rng, shape)
    apply = mixed_apply()
    for ksize in ksizes:
        assert (ksize - 1) // 2 < min(shape)
        for sigma in SIGMAS:
            weights = np.stack([R.weights_f32(ksize, sigma)] * len(imgs))
            got = np.full_like(imgs, 0x5A)
            L.gaussian_blur_batch_host(imgs, got, ksize, apply, weights, nthreads=3)
            want = R.blur_batch(imgs, ksize, apply, weights)
            assert np.array_equal(got, want), (shape, ksize, sigma)
            assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[4], imgs[4])
            assert (got[-3] == 0).all()
    # weights of the caller's own: not normalised, so the result clips at 255
    w = np.zeros((len(imgs), R.WROW), np.float32)
    k = ksizes[-1]
    w[:, :k] = 0.75
    got = np.empty_like(imgs)
    L.gaussian_blur_batch_host(imgs, got, k, np.ones(len(imgs), np.uint8), w)
    assert np.array_equal(got, R.blur_batch(imgs, k, np.ones(len(imgs)), w))


def test_pixel_entry_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ptr = lambda x, off=0: ctypes.c_void_p(x.ctypes.data + off)  # noqa: E731
    src = np.full((2, 6, 5, 3), 77, np.uint8)
    dst = np.full((3, 6, 5, 3), 66, np.uint8)
    apply = np.ones(2, np.uint8)
    w = np.zeros((2, 32), np.float32)
    w[:, 0] = 1

    def call(s=None, d=None, h=6, wd=5, k=3, stride=0, entry='host'):
        s = ptr(src) if s is None else s
        d = ptr(dst) if d is None else d
        if entry == 'host':
            return lib.ffcv_gaussian_blur_batch_host(s, d, 2, h, wd, k, ptr(apply), ptr(w), stride, 1)
        return lib.ffcv_gaussian_blur_batch(None, s, d, 2, h, wd, k, ptr(apply), ptr(w), stride)
    for entry, name in (('host', b'ffcv_gaussian_blur_batch_host'), ('device', b'ffcv_gaussian_blur_batch')):
        for kw in (dict(k=2), dict(k=0), dict(k=33), dict(k=11), dict(h=0), dict(wd=-1), dict(wd=65536),
                   dict(stride=89), dict(d=ptr(src)), dict(d=ptr(src, 90)), dict(d=ptr(src, 179)),
                   dict(s=ptr(dst, 90), stride=90)):
            assert call(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
    assert b'overlap' in lib.ffcv_last_error()
    assert (src == 77).all() and (dst == 66).all()
    assert call(k=5) == 0 and call(stride=135) == 0          # r = 2 < 5; a padded stride
    assert L.gaussian_blur_lds_bytes() >= 15 * 32 * 32 and L.gaussian_blur_band_rows() >= 1
    with pytest.raises(TypeError):
        L.gaussian_blur_batch_host(src[:, :, :, :2], dst, 3, apply, w)


def test_order_fixture(hip_lib):
    """Each tile's centre must come out as the pinned arithmetic gives it; on
    every tile a fused multiply-add or the descending tap order gives another
    byte."""
    from ffcv_amd import libffcv as L
    z = np.load(GOLDEN)
    total = 0
    for ksize in (3, 5, 23):
        r = (ksize - 1) // 2
        tiles, weights, want = z[f'tiles_{ksize}'], z[f'weights_{ksize}'], z[f'want_{ksize}']
        assert tiles.shape[1:] == (ksize, ksize, 3) and weights.shape == (len(tiles), R.WROW)
        differs = (want != z[f'fma_{ksize}']).any(1) | (want != z[f'reversed_{ksize}']).any(1)
        assert differs.all()
        got = np.empty_like(tiles)
        L.gaussian_blur_batch_host(tiles, got, ksize, np.ones(len(tiles), np.uint8), weights)
        assert np.array_equal(got[:, r, r], want), ksize
        assert np.array_equal(got, R.blur_batch(tiles, ksize, np.ones(len(tiles)), weights))
        total += len(tiles)
    assert total >= 32


def test_blur_ends_a_decoders_fused_prefix(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, RandomResizedCropRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, NormalizeImage, ToTensor, ToDevice, ToTorchImage, RandomHorizontalFlip,
                                     RandomTranslate, RandomResizedCrop, GaussianBlur)
    fields = lambda mode: {'image': RGBImageField(write_mode=mode), 'label': IntField()}  # noqa: E731
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)), fields('raw'))
    jpg = write(str(tmp_path / 'jpg.beton'), NaturalDS(6, hw=(48, 40)), fields('jpg'))
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])

    def graph(fn, ops):
        r = Reader(fn)
        g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                  r.metadata, OSCacheManager(r).compile_reader(), device='cuda:0')
        return g, g._chains['image'][0]

    def absorbed(ops):
        return [i for i, o in enumerate(ops) if getattr(o, '_absorbed', False)]

    def tail():
        return [ToTensor(), ToDevice(ch.device('cuda:0'), non_blocking=True), ToTorchImage(),
                NormalizeImage(mean, std, np.float16)]

    ops = [RandomResizedCropRGBImageDecoder((32, 32)), RandomHorizontalFlip(), GaussianBlur(5), Cutout(8)] + tail()
    g, dec = graph(jpg, ops)
    assert absorbed(ops) == [1]
    g.collect_requirements()
    assert g.groupable() and tuple(g.states[g.outputs['image'].id].shape) == (3, 32, 32)
    assert not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes)
    ops = [SimpleRGBImageDecoder(), RandomTranslate(2), RandomHorizontalFlip(), GaussianBlur(3), Cutout(4)] + tail()
    g, dec = graph(raw, ops)
    assert dec.fused and list(dec._fused_steps) == ops[1:3] and dec._fused_normalize is None
    assert absorbed(ops) == [1, 2]
    # a RandomResizedCrop transform in front of the blur absorbs nothing past it
    ops = [SimpleRGBImageDecoder(), RandomResizedCrop((0.3, 1), (0.75, 4 / 3), 24), GaussianBlur(3),
           RandomHorizontalFlip()] + tail()
    g, dec = graph(raw, ops)
    assert absorbed(ops) == [] and not ops[1].fused
    g.collect_requirements()
    assert g.groupable()
    # a kernel too long for the image is refused when states are declared
    ops = [RandomResizedCropRGBImageDecoder((8, 8)), GaussianBlur(17), ToTensor()]
    g, dec = graph(jpg, ops)
    with pytest.raises(TypeError, match='GaussianBlur'):
        g.collect_requirements()


def expected_chain(img, seed, epoch, sid, ksize=5, threshold=100):
    """brightness(0.5, p 0.6) -> grayscale(p 0.4) -> GaussianBlur(ksize, p 0.7)
    -> solarization(threshold, p 0.5) on one image with the contract's draws;
    returns the image and the four decisions."""
    from tests import color_jitter_ref as CR
    a1, v1 = CR.jitter_draw(seed, epoch, sid, CR.BRIGHTNESS, 0.6, 0.5)
    a2, _ = R.uniform_draw(seed, epoch, sid, R.OP_GRAYSCALE, 0.4, 0.0, 0.0)
    a3, sigma = R.uniform_draw(seed, epoch, sid, R.OP_BLUR, 0.7, 0.1, 2.0)
    a4, thr = R.uniform_draw(seed, epoch, sid, R.OP_SOLARIZE, 0.5, threshold, threshold)
    assert thr == threshold
    assert R.guard_holds(ksize, sigma), (seed, epoch, sid, float(sigma))
    out = np.array(img, np.uint8)
    if a1:
        out = CR.jitter_np(out, CR.BRIGHTNESS, v1)
    if a2:
        out = R.step_np(out, R.GRAYSCALE, 0.0)
    if a3:
        out = R.blur(out, ksize, R.weights_f32(ksize, sigma))
    if a4:
        out = R.step_np(out, R.SOLARIZE, threshold)
    return out, (a1, a2, a3, a4)


def chain_ops(ksize=5, threshold=100):
    from ffcv_amd.transforms import RandomBrightness, RandomGrayscale, RandomSolarization, GaussianBlur
    return [RandomBrightness(0.5, 0.6), RandomGrayscale(0.4), GaussianBlur(ksize, p=0.7),
            RandomSolarization(threshold)]


def test_cpu_loader_brightness_grayscale_blur_solarization(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'blur.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed = 12
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder()] + chain_ops() + [ToTensor()]})
    for epoch in range(2):
        counts = np.zeros(4, int)
        seen = 0
        for b, (images, labels) in enumerate(loader):
            got = images.numpy()
            assert got.shape == (8, 32, 32, 3) and got.dtype == np.uint8
            for k in range(8):
                sid = b * 8 + k
                want, flags = expected_chain(ds.imgs[sid], seed, epoch, sid)
                assert np.array_equal(got[k], want), (epoch, sid, flags)
                counts += np.array(flags, int)
                seen += 1
        assert seen == 24 and all(0 < v < 24 for v in counts)
