"""The RandomResizedCrop transform on the host (no GPU): the drop-in names,
its state declaration, the host draw twin of the C ABI against the oracle's
get_random_crop under the seeding contract (op id 8), the host resize twin
against the oracle's resize_crop on a forced-crop table that covers every
resize kind, the ABI's argument checks and a CPU Loader.  Every comparison is
bit for bit (tests/rrc_transform_ref.py)."""
import numpy as np
import pytest

from tests import resize_ref
from tests.helpers import NaturalDS, write
from tests.rrc_transform_ref import (DEFAULT_RATIO, DEFAULT_SCALE, SAMPLE_OK, SAMPLE_RANGE, crop_draw,
                                     every_size_crops, expected_resize, expected_transform, forced_crops,
                                     invalid_crops, kinds)

REFERENCE_ALL = ['ToTensor', 'ToDevice', 'ToTorchImage', 'NormalizeImage', 'Convert', 'Squeeze', 'View',
                 'RandomResizedCrop', 'RandomHorizontalFlip', 'RandomTranslate', 'Cutout', 'ImageMixup',
                 'LabelMixup', 'MixupToOneHot', 'Poison', 'ReplaceLabel', 'ModuleWrapper', 'RandomBrightness',
                 'RandomContrast', 'RandomSaturation']  # ffcv/transforms/__init__.py __all__


def test_drop_in_names():
    from ffcv.transforms import RandomResizedCrop
    from ffcv.transforms.random_resized_crop import RandomResizedCrop as ByModule
    import ffcv_amd.transforms as T
    import ffcv.transforms as FT
    assert RandomResizedCrop is T.RandomResizedCrop and ByModule is RandomResizedCrop
    assert 'RandomResizedCrop' in T.__all__
    for name in REFERENCE_ALL:  # every public name of the reference, no exception
        assert name in T.__all__ and hasattr(FT, name), name
    op = RandomResizedCrop((0.08, 1.0), (0.75, 4 / 3), 32)
    assert op.size == 32 and op.scale == (0.08, 1.0) and op.ratio == (0.75, 4 / 3)
    assert RandomResizedCrop(scale=(0.5, 1), ratio=(1, 1), size=np.int64(7)).size == 7
    assert RandomResizedCrop.device_aware and RandomResizedCrop.per_sample
    for bad in (0, -1, 1.5, '32', None, True):
        with pytest.raises(ValueError):
            RandomResizedCrop((0.08, 1), (0.75, 4 / 3), bad)


def test_state_and_memory():
    import torch as ch
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomResizedCrop
    op = RandomResizedCrop((0.25, 1), (0.75, 4 / 3), 24)
    host = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(40, 56, 3))
    st, mem = op.declare_state_and_memory(host)
    assert tuple(st.shape) == (24, 24, 3) and np.dtype(st.dtype) == np.uint8 and st.device.type == 'cpu'
    assert tuple(mem[0].shape) == (24, 24, 3) and np.dtype(mem[0].dtype) == np.uint8
    assert tuple(mem[1].shape) == (4,) and np.dtype(mem[1].dtype) == np.int32
    dev = State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(32, 32, 3))
    st, mem = op.declare_state_and_memory(dev)
    assert tuple(st.shape) == (24, 24, 3) and st.dtype == ch.uint8 and st.device.type == 'cuda'
    assert mem[0].dtype == ch.uint8 and mem[0].device.type == 'cuda' and mem[1].dtype == ch.int32
    for bad in (State(jit_mode=False, device=ch.device('cpu'), dtype=ch.float32, shape=(32, 32, 3)),
                State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('f4'), shape=(32, 32, 3)),
                State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(3, 32, 32)),
                State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.float16, shape=(3, 32, 32))):
        with pytest.raises(TypeError, match='before ToTorchImage'):
            op.declare_state_and_memory(bad)


DRAW_CASES = [((32, 32), DEFAULT_SCALE, DEFAULT_RATIO), ((40, 56), DEFAULT_SCALE, DEFAULT_RATIO),
              ((56, 40), DEFAULT_SCALE, DEFAULT_RATIO),
              ((32, 32), (1.5, 2.0), DEFAULT_RATIO),      # all ten tries fail: the centre fallback
              ((40, 56), (1.5, 2.0), (2, 3)), ((56, 40), (1.5, 2.0), (2, 3)),          # in_ratio < min(ratio)
              ((40, 56), (1.5, 2.0), (0.2, 0.3)), ((56, 40), (1.5, 2.0), (0.2, 0.3)),  # in_ratio > max(ratio)
              ((40, 56), (0.08, 1.0), (2, 3)), ((56, 40), (0.08, 1.0), (0.2, 0.3)),
              ((32, 32), (1, 1), (1, 1)), ((40, 56), (1, 1), (1, 1))]                  # the full image


def test_host_draws_match_oracle(hip_lib, oracle):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(5)
    n = 250                                            # x 12 cases = 3,000 (seed, epoch, id) triples
    total = 0
    for case, ((H, W), scale, ratio) in enumerate(DRAW_CASES):
        seeds = rng.integers(0, 2 ** 63, n)
        epochs = rng.integers(0, 1000, n)
        ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
        ids[:8] = np.arange(8)
        seeds[:4], epochs[:4] = 0, 0
        for k in range(n):
            got = L.crop_draw_batch_host(ids[k:k + 1], H, W, scale, ratio, int(seeds[k]), int(epochs[k]))[0]
            want = crop_draw(oracle, seeds[k], epochs[k], ids[k], H, W, scale, ratio)
            assert tuple(got.tolist()) == want, (case, k)
            i, j, h, w = want
            assert 0 < h <= H and 0 < w <= W and 0 <= i <= H - h and 0 <= j <= W - w
            total += 1
        if scale == (1, 1):   # the full image of a square source; 40 x 56 has no 47 x 47 window: the fallback
            assert want == ((0, 0, H, W) if H == W else (0, 8, 40, 40))
    assert total >= 2000
    # one call over a batch (one seed / epoch), with the status array
    ids = np.arange(200, dtype=np.uint64) * 3
    st = np.full(200, -1, np.int32)
    batch = L.crop_draw_batch_host(ids, 40, 56, DEFAULT_SCALE, DEFAULT_RATIO, 9, 4, st)
    want = np.array([crop_draw(oracle, 9, 4, i, 40, 56) for i in ids])
    assert np.array_equal(batch, want) and (st == SAMPLE_OK).all()
    assert len({tuple(r) for r in batch.tolist()}) > 150
    # the decoder's stream (op id 1) gives other windows for most ids
    dec = np.array([crop_draw(oracle, 9, 4, i, 40, 56, op_id=1) for i in ids])
    assert (batch != dec).any(axis=1).mean() > 0.9
    # the fallback branches were taken where the cases say so
    assert tuple(L.crop_draw_batch_host(ids[:1], 40, 56, (1.5, 2), (2, 3), 1, 0)[0]) == (6, 0, 28, 56)
    assert tuple(L.crop_draw_batch_host(ids[:1], 56, 40, (1.5, 2), (0.2, 0.3), 1, 0)[0]) == (0, 11, 56, 17)
    assert tuple(L.crop_draw_batch_host(ids[:1], 40, 56, (1.5, 2), (0.2, 0.3), 1, 0)[0]) == (0, 22, 40, 12)


# (source H, W), window or None for a table, output (h, w), the kind it must be
HOST_CASES = [((32, 32), (0, 0, 32, 32), (32, 32), 0),      # copy
              ((64, 64), (0, 0, 64, 64), (32, 32), 1),      # integer scale
              ((70, 70), (5, 3, 64, 64), (32, 32), 1),
              ((64, 64), (7, 9, 48, 40), (32, 32), 2),      # area
              ((64, 64), (3, 5, 20, 50), (32, 32), 3),      # linear (upscaled rows, downscaled columns)
              ((64, 64), (3, 5, 50, 20), (32, 32), 3),
              ((40, 56), (0, 0, 1, 1), (32, 32), 3), ((40, 56), (39, 55, 1, 1), (32, 32), 3),
              ((40, 56), (17, 0, 1, 56), (32, 32), 3), ((40, 56), (0, 31, 40, 1), (32, 32), 3),
              ((40, 56), (20, 28, 20, 28), (32, 32), 3),    # the bottom-right corner
              ((40, 56), (3, 5, 20, 50), (30, 30), 3),      # 3 * 30 is no multiple of 8: the scalar tail
              ((40, 56), (3, 5, 33, 35), (30, 30), 2), ((40, 56), (3, 5, 20, 50), (33, 33), 3),
              ((40, 56), (0, 0, 40, 56), (33, 33), 2), ((33, 35), (0, 0, 33, 35), (33, 35), 0),
              ((40, 56), (3, 5, 20, 50), (24, 40), 3), ((40, 56), (8, 8, 24, 40), (24, 40), 0),
              ((56, 96), (4, 8, 48, 80), (24, 40), 1)]


@pytest.mark.parametrize('nthreads', [1, 3])
def test_host_twin_matches_oracle(hip_lib, oracle, nthreads):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(3)
    seen = set()
    for (H, W), crop, (oh, ow), kind in HOST_CASES:
        assert resize_ref.kind_of(crop[2], crop[3], oh, ow) == kind, (crop, oh, ow)
        seen.add(kind)
        imgs = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        crops = np.array([crop] * 3, np.int32)
        out = np.full((3, oh, ow, 3), 7, np.uint8)
        st = np.full(3, -1, np.int32)
        L.rrc_images_batch_host(imgs, crops, out, st, nthreads=nthreads)
        want, wst = expected_resize(oracle, imgs, crops, oh, ow)
        assert np.array_equal(out, want) and np.array_equal(st, wst), (H, W, crop, oh, ow)
    assert seen == {0, 1, 2, 3}
    # tables over whole batches: every kind again, per output size
    for (H, W), outs in (((64, 64), [(32, 32), (30, 30), (33, 33), (24, 40)]), ((40, 56), [(32, 32), (24, 40)]),
                         ((33, 35), [(32, 32), (33, 33)])):
        imgs = rng.integers(0, 256, (70, H, W, 3), dtype=np.uint8)
        imgs[::7] = np.where(imgs[::7] > 127, 255, 0)          # saturated extremes now and then
        crops = forced_crops(H, W, 70, seed=H)
        for oh, ow in outs:
            if (H, W) == (64, 64) and (oh, ow) == (32, 32):
                assert kinds(crops, oh, ow) == {0, 1, 2, 3}
            out = np.full((70, oh, ow, 3), 7, np.uint8)
            st = np.full(70, -1, np.int32)
            L.rrc_images_batch_host(imgs, crops, out, st, nthreads=nthreads)
            want, wst = expected_resize(oracle, imgs, crops, oh, ow)
            assert np.array_equal(out, want) and (st == SAMPLE_OK).all(), (H, W, oh, ow)


def test_host_twin_every_crop_size_of_32(hip_lib, oracle):
    """A window of every size (h, w) of a 32 x 32 source to 32 x 32: every
    linear tap pattern, the copy and the 1 x 1 window among them."""
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(4)
    crops = every_size_crops(32, 32)
    assert len(crops) == 1024 and kinds(crops, 32, 32) == {0, 3}
    imgs = rng.integers(0, 256, (len(crops), 32, 32, 3), dtype=np.uint8)
    out = np.empty((len(crops), 32, 32, 3), np.uint8)
    L.rrc_images_batch_host(imgs, crops, out, None, nthreads=3)
    want, _ = expected_resize(oracle, imgs, crops, 32, 32)
    assert np.array_equal(out, want)


def test_host_twin_invalid_crops(hip_lib, oracle):
    from ffcv_amd import libffcv as L
    H, W = 40, 56
    bad = invalid_crops(H, W)
    good = forced_crops(H, W, len(bad) + 1, seed=2)
    crops = np.empty((2 * len(bad) + 1, 4), np.int32)
    crops[0::2], crops[1::2] = good, bad
    imgs = np.random.default_rng(6).integers(1, 256, (len(crops), H, W, 3), dtype=np.uint8)
    out = np.full((len(crops), 32, 32, 3), 7, np.uint8)
    st = np.full(len(crops), -1, np.int32)
    L.rrc_images_batch_host(imgs, crops, out, st, nthreads=3)
    want, wst = expected_resize(oracle, imgs, crops, 32, 32)
    assert (wst[1::2] == SAMPLE_RANGE).all() and (wst[0::2] == SAMPLE_OK).all()
    assert np.array_equal(st, wst) and np.array_equal(out, want)
    assert (out[1::2] == 0).all() and all(o.any() for o in out[0::2])


def test_host_twin_within_exact_bound(hip_lib):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(8)
    for (H, W), crop, (oh, ow), kind in (HOST_CASES[1], HOST_CASES[3], HOST_CASES[4], HOST_CASES[11]):
        img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        out = np.empty((1, oh, ow, 3), np.uint8)
        L.rrc_images_batch_host(img, np.array([crop], np.int32), out)
        i, j, h, w = crop
        worst, _, _, _, bound = resize_ref.compare(out[0], img[0, i:i + h, j:j + w])
        print(kind, worst, bound)
        assert worst <= bound, (crop, oh, ow, worst, bound)


def test_host_abi_rejects_bad_arguments(hip_lib):
    import ctypes
    lib = hip_lib
    img = np.full((2, 8, 8, 3), 77, np.uint8)
    out = np.full((2, 4, 4, 3), 55, np.uint8)
    crops = np.array([[0, 0, 8, 8]] * 2, np.int32)
    st = np.zeros(2, np.int32)
    good = dict(inp=img.ctypes.data, in_stride=192, batch=2, height=8, width=8, crops=crops.ctypes.data, out_h=4,
                out_w=4, out=out.ctypes.data, out_stride=48, status=st.ctypes.data, nthreads=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ffcv_rrc_images_batch_host(a['inp'], a['in_stride'], a['batch'], a['height'], a['width'],
                                              a['crops'], a['out_h'], a['out_w'], a['out'], a['out_stride'],
                                              a['status'], a['nthreads'])
    assert call() == 0 and (out[:, 0, 0] == 77).all()
    out[:] = 55
    for kw in (dict(inp=None), dict(crops=None), dict(out=None), dict(batch=-1), dict(height=0), dict(width=-2),
               dict(out_h=0), dict(out_w=0), dict(in_stride=191), dict(out_stride=47),
               dict(out=img.ctypes.data + 100)):
        assert call(**kw) == -1, kw
        assert b'ffcv_rrc_images_batch_host' in lib.ffcv_last_error()
    assert (out == 55).all()
    assert call(batch=0, inp=img.ctypes.data) == 0 and (out == 55).all()
    assert call(status=None) == 0
    # draws
    ids = np.arange(4, dtype=np.uint64)
    cr = np.zeros((4, 4), np.int32)
    two = ctypes.c_double * 2

    def draw(ids_p=ids.ctypes.data, batch=4, H=8, W=8, scale=two(0.08, 1), ratio=two(0.75, 4 / 3),
             crops_p=cr.ctypes.data):
        return lib.ffcv_crop_draw_batch_host(ids_p, batch, H, W, scale, ratio, 0, 0, crops_p, None)
    assert draw() == 0
    for kw in (dict(ids_p=None), dict(crops_p=None), dict(batch=-1), dict(H=0), dict(W=0), dict(scale=None),
               dict(ratio=None), dict(ratio=two(0, 1)), dict(scale=two(float('nan'), 1))):
        assert draw(**kw) == -1, kw
        assert b'ffcv_crop_draw_batch_host' in lib.ffcv_last_error()
    assert draw(batch=0) == 0


def test_lowering_decisions(tmp_path):
    """No kernel launched: what the graph absorbs into the transform's launch."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, NormalizeImage, ToTensor, ToDevice, ToTorchImage, RandomBrightness,
                                     RandomHorizontalFlip, RandomResizedCrop, RandomTranslate)
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])

    def graph(ops, device='cuda:0'):
        r = Reader(raw)
        return Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                     r.metadata, OSCacheManager(r).compile_reader(), device=device)

    def tail():
        return [ToTensor(), ToDevice(ch.device('cuda:0')), ToTorchImage(), NormalizeImage(mean, std, np.float16)]
    rrc = RandomResizedCrop((0.08, 1), (0.75, 4 / 3), 24)
    ops = [SimpleRGBImageDecoder(), rrc, RandomHorizontalFlip(), Cutout(4, (1, 2, 3))] + tail()
    g = graph(ops)
    assert rrc._fused_flip is ops[2] and rrc._fused_cutout is ops[3] and rrc._fused_normalize is ops[7]
    assert not rrc._cutout_before_flip and all(o._absorbed for o in (ops[2], ops[3], ops[7]))
    g.collect_requirements()
    last = g.states[g.outputs['image'].id]
    assert last.dtype == ch.float16 and tuple(last.shape) == (3, 24, 24) and g.groupable()
    names = [name for name, alloc in g.allocation_signature() if alloc is not None]
    assert names == ['SimpleRGBImageDecoder', 'RandomResizedCrop']

    rrc = RandomResizedCrop((0.08, 1), (0.75, 4 / 3), 24)
    ops = [SimpleRGBImageDecoder(), rrc, Cutout(4), RandomHorizontalFlip(), Cutout(2)] + tail()
    graph(ops)                                       # cutout first; each operation once
    assert rrc._cutout_before_flip and rrc._fused_cutout is ops[2] and rrc._fused_flip is ops[3]
    assert not ops[4]._absorbed and rrc._fused_normalize is None

    rrc = RandomResizedCrop((0.08, 1), (0.75, 4 / 3), 24)
    ops = [SimpleRGBImageDecoder(), rrc, RandomBrightness(0.3), RandomHorizontalFlip(), Cutout(4)] + tail()
    graph(ops)                                       # an operation in between: nothing absorbed
    assert not rrc.fused and not any(getattr(o, '_absorbed', False) for o in ops[2:])

    rrc = RandomResizedCrop((0.08, 1), (0.75, 4 / 3), 24)
    ops = [SimpleRGBImageDecoder(), RandomTranslate(2), rrc, RandomHorizontalFlip()]
    graph(ops)                                       # behind the small-image launch
    assert ops[0].fused and ops[1]._absorbed and rrc._fused_flip is ops[3]

    rrc = RandomResizedCrop((0.08, 1), (0.75, 4 / 3), 24)
    ops = [SimpleRGBImageDecoder(), rrc, RandomHorizontalFlip()]
    graph(ops, device='cpu')                         # a CPU Loader lowers nothing
    assert not rrc.fused and not ops[2]._absorbed


def test_cpu_loader(tmp_path, hip_lib, oracle):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import RandomResizedCrop
    ds = NaturalDS(37, hw=(40, 56), seed=3)
    fn = write(str(tmp_path / 'rrc.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    scale, ratio = (0.25, 1), (0.75, 4 / 3)

    def mk(seed):
        return Loader(fn, batch_size=8, device='cpu', seed=seed, drop_last=False, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomResizedCrop(scale, ratio, 24)]})
    a, b = mk(12), mk(12)
    epochs = []
    for epoch in range(2):
        seen, outs = 0, []
        for bi, ((images, labels), (images_b, _)) in enumerate(zip(a, b)):
            got = np.asarray(images)
            assert got.shape[1:] == (24, 24, 3) and got.dtype == np.uint8
            assert np.array_equal(got, np.asarray(images_b))          # the same seed reproduces
            for k in range(got.shape[0]):
                sid = bi * 8 + k
                want = expected_transform(oracle, ds.imgs[sid], 12, epoch, sid, 24, scale, ratio)
                assert np.array_equal(got[k], want), (epoch, sid)
                seen += 1
            outs.append(got.copy())
        assert seen == 37
        epochs.append(np.concatenate(outs))
    assert not np.array_equal(epochs[0], epochs[1])                   # new windows every epoch
