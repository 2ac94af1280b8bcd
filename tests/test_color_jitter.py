"""RandomBrightness / RandomContrast / RandomSaturation on the host (no GPU):
public names and argument checks, the reference's own outputs
(tests/golden/color_jitter.npz, written by tests/golden/make_color_jitter.py
from the reference's color_jitter.py), the host twins of the C ABI (draws
against numpy's legacy RandomState under the seeding contract, op ids 5-7;
pixels against tests/color_jitter_ref.py, bit for bit, over all 2^24 RGB
triples), the graph lowering, and a CPU Loader."""
import ctypes
import inspect
import itertools
import os

import numpy as np
import pytest

from tests.helpers import NaturalDS, write
from tests.color_jitter_ref import (BRIGHTNESS, CONTRAST, SATURATION, OP_ID, apply_program, apply_program_batch,
                                    jitter_draw, jitter_np, near_integer_triples)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'color_jitter.npz')
KINDS = (BRIGHTNESS, CONTRAST, SATURATION)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def near_image():
    t = near_integer_triples()
    assert len(t) == 1704
    return t.reshape(24, 71, 3)


def _ops():
    from ffcv_amd.transforms import RandomBrightness, RandomContrast, RandomSaturation
    return {BRIGHTNESS: RandomBrightness, CONTRAST: RandomContrast, SATURATION: RandomSaturation}


def test_public_names_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    for kind, cls in _ops().items():
        name = cls.__name__
        assert getattr(FT, name) is cls and getattr(T, name) is cls and name in T.__all__
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert [p.name for p in params] == ['self', 'magnitude', 'p'] and params[2].default == 0.5
        op = cls(0.4)
        assert op.magnitude == 0.4 and op.p == 0.5 and cls.per_sample and cls.device_aware
        assert cls.op_id == OP_ID[kind] and cls.kind == kind
        assert cls(0, 0).p == 0 and cls(3.5, 1).magnitude == 3.5
        for bad in (-0.1, float('inf'), float('nan'), None, 'x'):
            with pytest.raises(ValueError):
                cls(bad)
        for bad in (-0.01, 1.01, float('nan'), None):
            with pytest.raises(ValueError):
                cls(0.5, bad)


def test_state_must_be_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.state import State
    for cls in _ops().values():
        op = cls(0.5)
        ok = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3))
        st, alloc = op.declare_state_and_memory(ok)
        assert alloc is None and st.shape == (8, 6, 3) and st.dtype == np.dtype('u1')
        op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
        for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('f4'), (8, 6, 3)),
                          (np.dtype('u1'), (8, 6)), (np.dtype('u1'), (8, 6, 4))):
            with pytest.raises(TypeError, match=cls.__name__):
                op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_host_numpy_path_reproduces_reference_images(golden, near_image):
    from ffcv_amd.transforms import color_jitter as CJ
    fns = {BRIGHTNESS: CJ.brightness_np, CONTRAST: CJ.contrast_np, SATURATION: CJ.saturation_np}
    meta = list(zip(golden['meta_op'].tolist(), golden['meta_seed'].tolist(), golden['meta_magnitude'].tolist(),
                    golden['meta_p'].tolist()))
    assert len(meta) >= 90
    applied = {k: 0 for k in KINDS}
    near_seen = 0
    for k, (kind, seed, m, p) in enumerate(meta):
        img, want = golden[f'in_{k}'], golden[f'out_{k}']
        assert img.std() > 0 and img.size <= 24 * 71 * 3
        rs = np.random.RandomState(seed)
        apply = rs.rand() < p
        ratio = rs.uniform(max(0, 1 - m), 1 + m)
        got = img.copy()
        if apply:
            fns[kind](got, ratio)
        assert np.array_equal(got, want), (k, kind)
        assert np.array_equal(jitter_np(img, kind, ratio) if apply else img, want), k  # the tests' own statement
        applied[kind] += bool(apply)
        near_seen += np.array_equal(img, near_image)
    assert all(v >= 20 for v in applied.values()) and near_seen >= 9


def test_host_draws_reproduce_reference_rows(golden, hip_lib):
    """The reference's recorded (rand(1) < p, uniform(lo, hi, 1)) per seed are
    RandomState(seed).rand() < p and .uniform(lo, hi), with equal float64 bits:
    the stream the contract gives every sample."""
    from ffcv_amd.transforms.color_jitter import jitter_range
    n = len(golden['rows_op'])
    assert n >= 300 and golden['rows_apply'].min() == 0 and golden['rows_apply'].max() == 1
    for op, seed, m, p, a, bits in zip(golden['rows_op'].tolist(), golden['rows_seed'].tolist(),
                                       golden['rows_magnitude'].tolist(), golden['rows_p'].tolist(),
                                       golden['rows_apply'].tolist(), golden['rows_ratio_bits'].tolist()):
        rs = np.random.RandomState(seed)
        lo, hi = jitter_range(m)
        assert bool(rs.rand() < p) == bool(a)
        assert int(np.float64(rs.uniform(lo, hi)).view(np.uint64)) == bits, (op, seed, m)


def test_host_draw_twin_matches_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.rng import contract_seed
    from ffcv_amd.transforms.color_jitter import jitter_draw as package_draw
    rng = np.random.default_rng(12)
    n = 500
    seeds = rng.integers(0, 2 ** 63, n)
    epochs = rng.integers(0, 1000, n)
    ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    ids[:8] = np.arange(8)
    seeds[:4], epochs[:4] = 0, 0
    for kind in KINDS:
        for m, p in ((0.0, 0.5), (0.4, 0.5), (1.0, 0.1), (2.5, 1.0), (0.7, 0.0)):
            applies = 0
            for k in range(n):
                rs = np.random.RandomState(contract_seed(int(seeds[k]), int(epochs[k]), int(ids[k]), OP_ID[kind]))
                wa, wr = rs.rand() < p, rs.uniform(max(0, 1 - m), 1 + m)
                ga, gr = L.color_jitter_draw_batch_host(ids[k:k + 1], int(seeds[k]), int(epochs[k]), OP_ID[kind], p, m)
                assert bool(ga[0]) == bool(wa) and gr.view(np.uint64)[0] == np.float64(wr).view(np.uint64), (kind, k)
                applies += int(ga[0])
            assert applies == (n if p == 1.0 else 0) if p in (0.0, 1.0) else 0 < applies < n
        # one call over a batch of 64 (one seed / epoch) gives the per-sample values
        ga, gr = L.color_jitter_draw_batch_host(ids[:64], 5, 3, OP_ID[kind], 0.5, 0.4)
        for k in range(64):
            wa, wr = jitter_draw(5, 3, int(ids[k]), kind, 0.5, 0.4)
            assert bool(ga[k]) == wa and gr.view(np.uint64)[k] == np.float64(wr).view(np.uint64)
            pa, pr = package_draw(5, 3, int(ids[k]), OP_ID[kind], 0.5, 0.4)
            assert pa == wa and np.float64(pr).view(np.uint64) == np.float64(wr).view(np.uint64)
        assert 0 < ga.sum() < 64


def _host(imgs, kinds, apply, ratio):
    from ffcv_amd import libffcv as L
    out = np.ascontiguousarray(imgs).copy()
    L.color_jitter_batch_host(out, list(kinds), np.asarray(apply, np.uint8), np.asarray(ratio, np.float64))
    return out


RATIOS = (0.0, 0.3, 0.5000000001, 0.97, 1.0, 1.4, 3.7)


def test_host_twin_saturation_all_rgb_triples(hip_lib):
    """Every one of the 2^24 RGB triples (one 4096 x 4096 image) through
    ffcv_color_jitter_batch_host's saturation, against numpy."""
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    ratio = 0.6180339887498949
    got = _host(img, [SATURATION], [[1]], [[ratio]])[0]
    for r0 in range(0, 4096, 512):   # saturation is per pixel: compare in slabs to bound numpy's temporaries
        assert np.array_equal(got[r0:r0 + 512], jitter_np(img[0, r0:r0 + 512], SATURATION, ratio)), r0


def test_host_twin_matches_numpy(hip_lib, near_image):
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (1, 7), (3, 5), (32, 32), (33, 31), (24, 71)):
        B = 9
        imgs = rng.integers(0, 256, (B,) + shape + (3,), dtype=np.uint8)
        if shape == (24, 71):
            imgs[0] = near_image
        imgs[1] //= 16                                   # a dark image: contrast mean near 0
        progs = [p for n in (1, 2, 3) for p in itertools.permutations(KINDS, n)]
        for kinds in progs:
            apply = rng.integers(0, 2, (len(kinds), B)).astype(np.uint8)
            apply[:, 0] = 1
            apply[:, 2] = 0
            ratio = rng.choice(RATIOS, (len(kinds), B))
            got = _host(imgs, kinds, apply, ratio)
            assert np.array_equal(got, apply_program_batch(imgs, kinds, apply, ratio)), (shape, kinds)
            assert np.array_equal(got[2], imgs[2])
    # the 1,704 near-integer triples, every operation, a spread of ratios
    for kind in KINDS:
        for r in RATIOS:
            got = _host(near_image[None], [kind], [[1]], [[r]])[0]
            assert np.array_equal(got, jitter_np(near_image, kind, r)), (kind, r)


def test_identity_and_clipping(hip_lib, golden):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(4)
    imgs = rng.integers(0, 256, (5, 9, 11, 3), dtype=np.uint8)
    ids = np.arange(5, dtype=np.uint64)
    for kind in KINDS:
        # p = 1, magnitude = 0: uniform(1, 1) is exactly 1.0 and every operation is the identity
        a, r = L.color_jitter_draw_batch_host(ids, 9, 0, OP_ID[kind], 1.0, 0.0)
        assert a.all() and (r == 1.0).all()
        assert np.array_equal(_host(imgs, [kind], a[None], r[None]), imgs)
    # magnitude >= 1: the reference's own small and large ratios clip at 0 and at 255
    bits = golden['rows_ratio_bits'].view(np.float64)
    big = golden['rows_magnitude'] >= 1
    small, large = bits[big].min(), bits[big].max()
    assert small < 0.05 and large > 5
    img = imgs[:1]
    dark = _host(img, [BRIGHTNESS], [[1]], [[small]])
    assert dark.max() <= 12 and (dark == 0).any()
    assert (_host(img, [BRIGHTNESS], [[1]], [[0.0]]) == 0).all()
    bright = _host(img, [BRIGHTNESS], [[1]], [[large]])
    assert (bright == 255).mean() > 0.7 and np.array_equal(bright, jitter_np(img[0], BRIGHTNESS, large)[None])
    for kind in (CONTRAST, SATURATION):
        out = _host(img, [kind], [[1]], [[large]])
        assert (out == 0).any() and (out == 255).any()
        assert np.array_equal(out, jitter_np(img[0], kind, large)[None])
        flat = _host(img, [kind], [[1]], [[small]])
        assert np.array_equal(flat, jitter_np(img[0], kind, small)[None])


def test_abi_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    img = np.full((2, 4, 4, 3), 77, np.uint8)
    apply = np.ones((3, 2), np.uint8)
    ratio = np.full((3, 2), 0.5)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def call(p, images=img, h=4, w=4):
        return lib.ffcv_color_jitter_batch_host(ptr(images) if images is not None else None, 2, h, w,
                                                ctypes.byref(p), ptr(apply), ptr(ratio))
    for steps, msg in (([], b'1 to 3 steps'), ([1, 2, 3, 1], b'1 to 3 steps'), ([2, 2], b'repeated'),
                       ([1, 9], b'unknown step'), ([0], b'unknown step')):
        assert call(L.color_jitter_params(steps)) == -1
        err = lib.ffcv_last_error()
        assert msg in err and b'ffcv_color_jitter_batch_host' in err
    ok = L.color_jitter_params([1])
    for kw in (dict(images=None), dict(h=0), dict(w=-1)):
        assert call(ok, **kw) == -1 and b'ffcv_color_jitter_batch_host' in lib.ffcv_last_error()
    assert (img == 77).all()
    ids = np.arange(2, dtype=np.uint64)
    a, r = np.zeros(2, np.uint8), np.zeros(2)
    for op_id, p, m in ((4, 0.5, 0.5), (8, 0.5, 0.5), (5, -0.1, 0.5), (5, 1.5, 0.5), (5, 0.5, -1.0),
                        (5, 0.5, float('inf')), (5, float('nan'), 0.5), (5, 0.5, float('nan'))):
        assert lib.ffcv_color_jitter_draw_batch_host(ptr(ids), 2, 0, 0, op_id, p, m, ptr(a), ptr(r)) == -1
        assert b'ffcv_color_jitter_draw_batch_host' in lib.ffcv_last_error()
    assert lib.ffcv_color_jitter_draw_batch_host(None, 2, 0, 0, 5, 0.5, 0.5, ptr(a), ptr(r)) == -1
    # the device entries check their arguments before anything is launched
    assert lib.ffcv_color_jitter_draw_batch(None, None, 2, 0, 0, 5, 0.5, 0.5, None, None, None) == -1
    assert b'ffcv_color_jitter_draw_batch' in lib.ffcv_last_error()
    assert lib.ffcv_color_jitter_batch(None, None, 2, 4, 4, ctypes.byref(ok), None, None, None, 0) == -1
    assert b'ffcv_color_jitter_batch' in lib.ffcv_last_error()
    assert L.color_jitter_workspace_bytes(0) == 0 and L.color_jitter_workspace_bytes(67) == 67 * 8
    assert 3 * 32 * 32 <= L.color_jitter_lds_bytes() <= 20 * 1024
    with pytest.raises(TypeError):
        L.color_jitter_batch_host(img[:, :, :, :2], [1], apply, ratio)


def test_graph_lowers_runs_of_jitter_ops(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, RandomResizedCropRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, NormalizeImage, ToTensor, ToDevice, ToTorchImage, RandomHorizontalFlip,
                                     RandomTranslate, RandomBrightness, RandomContrast, RandomSaturation)
    fields = lambda mode: {'image': RGBImageField(write_mode=mode), 'label': IntField()}  # noqa: E731
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)), fields('raw'))
    jpg = write(str(tmp_path / 'jpg.beton'), NaturalDS(6, hw=(48, 40)), fields('jpg'))
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])

    def graph(fn, ops, device='cuda:0'):
        r = Reader(fn)
        g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                  r.metadata, OSCacheManager(r).compile_reader(), device=device)
        return g, g._chains['image'][0]

    def absorbed(ops):
        return [i for i, o in enumerate(ops) if getattr(o, '_absorbed', False)]

    def tail():
        return [ToTensor(), ToDevice(ch.device('cuda:0'), non_blocking=True), ToTorchImage(),
                NormalizeImage(mean, std, np.float16)]

    # a run of three: one leader with the program, two absorbed; the decoder's prefix ends at the run
    ops = [SimpleRGBImageDecoder(), RandomHorizontalFlip(), RandomBrightness(0.4), RandomContrast(0.4),
           RandomSaturation(0.4), Cutout(4)] + tail()
    g, dec = graph(raw, ops)
    assert absorbed(ops) == [3, 4] and ops[2]._program == ops[2:5] and not dec.fused
    g.collect_requirements()
    assert g.groupable() and tuple(g.states[g.outputs['image'].id].shape) == (3, 32, 32)
    # a translate in front is still lowered into the decoder, up to the run
    ops = [SimpleRGBImageDecoder(), RandomTranslate(2), RandomHorizontalFlip(), RandomSaturation(0.4),
           RandomBrightness(0.4), Cutout(4)] + tail()
    g, dec = graph(raw, ops)
    assert dec.fused and list(dec._fused_steps) == ops[1:3] and dec._fused_normalize is None
    assert absorbed(ops) == [1, 2, 4] and ops[3]._program == ops[3:5]
    # a repeated kind splits the run; an operation in between ends it
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.1), RandomContrast(0.1), RandomBrightness(0.2),
           RandomSaturation(0.2), Cutout(4), RandomSaturation(0.3), ToTensor()]
    g, dec = graph(raw, ops)
    assert absorbed(ops) == [2, 4]
    assert ops[1]._program == ops[1:3] and ops[3]._program == ops[3:5] and ops[6]._program == [ops[6]]
    # a CPU graph lowers nothing
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.1), RandomContrast(0.1), ToTensor()]
    g, dec = graph(raw, ops, device='cpu')
    assert absorbed(ops) == [] and ops[1]._program == [ops[1]]
    # behind the layout change the operation refuses its input
    ops = [SimpleRGBImageDecoder(), ToTensor(), ToTorchImage(), RandomContrast(0.1)]
    g, dec = graph(raw, ops)
    with pytest.raises(TypeError, match='RandomContrast'):
        g.collect_requirements()

    # chains without a jitter operation lower as before: the CIFAR chain and the C3 chain
    ops = [SimpleRGBImageDecoder(), RandomHorizontalFlip(), RandomTranslate(2, (125, 123, 114)),
           Cutout(4, (125, 123, 114))] + tail()
    g, dec = graph(raw, ops)
    assert dec.fused and absorbed(ops) == [1, 2, 3, 7]
    ops = [RandomResizedCropRGBImageDecoder((32, 32)), Cutout(8, (124, 116, 103))] + tail()
    g, dec = graph(jpg, ops)
    assert absorbed(ops) == [1, 5]
    # and a jitter operation ends the ResizedCrop decoder's fused prefix like any unknown operation
    ops = [RandomResizedCropRGBImageDecoder((32, 32)), RandomHorizontalFlip(), RandomBrightness(0.4),
           RandomContrast(0.4), Cutout(8)] + tail()
    g, dec = graph(jpg, ops)
    assert absorbed(ops) == [1, 3] and ops[2]._program == ops[2:4]


def test_cpu_loader_flip_jitter_cutout(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import (ToTensor, Cutout, RandomHorizontalFlip, RandomBrightness, RandomContrast,
                                     RandomSaturation)
    from tests.translate_ref import apply_chain, cutout_draw
    ds = NaturalDS(24, hw=(13, 10), seed=3)
    fn = write(str(tmp_path / 'cj.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed = 12
    cfg = ((BRIGHTNESS, 0.5, 0.6), (CONTRAST, 0.7, 0.5), (SATURATION, 1.2, 0.5))   # kind, magnitude, p
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), RandomBrightness(0.5, 0.6),
                  RandomContrast(0.7), RandomSaturation(1.2, p=0.5), Cutout(4, (200, 201, 202)), ToTensor()]})
    for epoch in range(2):
        seen = 0
        counts = {k: 0 for k in KINDS}
        for b, (images, labels) in enumerate(loader):
            got = images.numpy()
            assert got.shape == (8, 13, 10, 3) and got.dtype == np.uint8
            for k in range(8):
                sid = b * 8 + k
                img, _ = apply_chain(ds.imgs[sid], 'f', seed, epoch, sid)
                draws = [jitter_draw(seed, epoch, sid, kind, p, m) for kind, m, p in cfg]
                img = apply_program(img, [c[0] for c in cfg], [d[0] for d in draws], [d[1] for d in draws])
                want = img.copy()
                y, x = cutout_draw(seed, epoch, sid, 13, 10, 4)
                want[y:y + 4, x:x + 4] = (200, 201, 202)
                assert np.array_equal(got[k], want), (epoch, sid)
                for (kind, _, _), d in zip(cfg, draws):
                    counts[kind] += d[0]
                seen += 1
        assert seen == 24 and all(0 < v < 24 for v in counts.values())
