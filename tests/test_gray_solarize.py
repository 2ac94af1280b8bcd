"""RandomGrayscale / RandomSolarization on the host (no GPU): public names and
argument checks, the two new steps of ffcv_color_jitter_batch_host against
numpy (tests/blur_ref.py on top of tests/color_jitter_ref.py) in every program
that contains one, and the graph lowering of runs with the new kinds.  (Their
draws, op ids 9 and 10, are checked in tests/test_blur.py.)"""
import inspect

import numpy as np
import pytest

from tests import blur_ref as R
from tests.color_jitter_ref import SATURATION, jitter_np, near_integer_triples
from tests.helpers import NaturalDS, write

THRESHOLDS = (0, 1, 128, 255, 256)
RATIOS = (0.0, 0.3, 0.5000000001, 0.97, 1.0, 1.4, 3.7)


def _host(imgs, kinds, apply, value):
    from ffcv_amd import libffcv as L
    out = np.ascontiguousarray(imgs).copy()
    L.color_jitter_batch_host(out, list(kinds), np.asarray(apply, np.uint8), np.asarray(value, np.float64))
    return out


def draw_values(rng, kinds, B):
    """A value per step and image: ratios for the jitter kinds, a threshold
    for solarize, and a value that must not matter for grayscale."""
    v = rng.choice(RATIOS, (len(kinds), B))
    for i, kind in enumerate(kinds):
        if kind == R.SOLARIZE:
            v[i] = rng.choice(THRESHOLDS, B)
        elif kind == R.GRAYSCALE:
            v[i] = rng.choice((0.0, 0.7, 5.0), B)
    return v


def test_public_names_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    from ffcv_amd.transforms.color_jitter import _ColorJitter
    G, S = T.RandomGrayscale, T.RandomSolarization
    for cls, op_id, kind in ((G, R.OP_GRAYSCALE, R.GRAYSCALE), (S, R.OP_SOLARIZE, R.SOLARIZE)):
        assert getattr(FT, cls.__name__) is cls and cls.__name__ in T.__all__ and issubclass(cls, _ColorJitter)
        assert cls.op_id == op_id and cls.kind == kind and cls.per_sample and cls.device_aware
    assert [p.name for p in inspect.signature(G.__init__).parameters.values()] == ['self', 'p']
    assert [(p.name, p.default) for p in inspect.signature(S.__init__).parameters.values()][1:] == \
        [('threshold', 128), ('p', 0.5)]
    assert G().p == 0.1 and (G().lo, G().hi) == (0.0, 0.0)
    s = S()
    assert s.threshold == 128 and s.p == 0.5 and (s.lo, s.hi) == (128.0, 128.0)
    assert S(0).threshold == 0 and S(256, 1).lo == 256.0
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError):
            G(bad)
        with pytest.raises(ValueError):
            S(128, bad)
    for bad in (-1, 257, 127.5, None, 'x', True):
        with pytest.raises(ValueError):
            S(bad)


def test_state_must_be_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomGrayscale, RandomSolarization
    for op in (RandomGrayscale(), RandomSolarization()):
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
        assert alloc is None and st.shape == (8, 6, 3)
        for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('u1'), (8, 6))):
            with pytest.raises(TypeError, match=type(op).__name__):
                op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_host_numpy_functions():
    from ffcv_amd.transforms import color_jitter as CJ
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(CJ.grayscale_np(img.copy()), R.step_np(img, R.GRAYSCALE, 0))
    for t in THRESHOLDS:
        assert np.array_equal(CJ.solarize_np(img.copy(), float(t)), R.step_np(img, R.SOLARIZE, t))
    assert np.array_equal(R.step_np(img, R.SOLARIZE, 0), 255 - img)
    assert np.array_equal(R.step_np(img, R.SOLARIZE, 256), img)


@pytest.mark.parametrize('shape', ((1, 1), (3, 5), (32, 32), (33, 31)), ids=str)
def test_host_twin_matches_numpy_in_every_program_with_a_new_kind(hip_lib, shape):
    progs = R.programs_with_new_kind()
    assert len(progs) == 2 + (20 - 6) + (60 - 6)
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    B = 9
    imgs = rng.integers(0, 256, (B,) + shape + (3,), dtype=np.uint8)
    imgs[1] //= 16
    for kinds in progs:
        apply = rng.integers(0, 2, (len(kinds), B)).astype(np.uint8)
        apply[:, 0] = 1
        apply[:, 2] = 0
        value = draw_values(rng, kinds, B)
        got = _host(imgs, kinds, apply, value)
        assert np.array_equal(got, R.apply_program_batch(imgs, kinds, apply, value)), (shape, kinds)
        assert np.array_equal(got[2], imgs[2])


def test_thresholds_and_near_integer_triples(hip_lib):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1, 16, 16, 3), dtype=np.uint8)
    img[0, 0, :, 0] = np.arange(120, 136)
    for t in THRESHOLDS:
        got = _host(img, [R.SOLARIZE], [[1]], [[float(t)]])[0]
        assert np.array_equal(got, np.where(img[0] >= t, 255 - img[0], img[0])), t
    near = near_integer_triples()
    assert len(near) == 1704
    near = near.reshape(1, 24, 71, 3)
    gray = _host(near, [R.GRAYSCALE], [[1]], [[0.0]])
    assert np.array_equal(gray, _host(near, [SATURATION], [[1]], [[0.0]]))
    assert np.array_equal(gray[0], jitter_np(near[0], SATURATION, 0.0))
    assert np.array_equal(gray[0], R.step_np(near[0], R.GRAYSCALE, 0))
    assert (gray[..., 0] == gray[..., 1]).all() and (gray[..., 1] == gray[..., 2]).all()


def test_existing_program_rules_hold(hip_lib):
    import ctypes
    from ffcv_amd import libffcv as L
    lib = L.lib()
    img = np.full((2, 4, 4, 3), 77, np.uint8)
    apply, ratio = np.ones((3, 2), np.uint8), np.full((3, 2), 0.5)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for steps, msg in (([4, 4], b'repeated'), ([5, 1, 5], b'repeated'), ([4, 5, 1, 2], b'1 to 3 steps'),
                       ([4, 6], b'unknown step'), ([0], b'unknown step'), ([7], b'unknown step'),
                       ([9], b'unknown step')):
        p = L.color_jitter_params(steps)
        assert lib.ffcv_color_jitter_batch_host(ptr(img), 2, 4, 4, ctypes.byref(p), ptr(apply), ptr(ratio)) == -1
        assert msg in lib.ffcv_last_error()
    assert (img == 77).all()
    assert (L.CJ_GRAYSCALE, L.CJ_SOLARIZE) == (R.GRAYSCALE, R.SOLARIZE)


def test_graph_lowers_runs_with_the_new_kinds(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, ToTensor, RandomBrightness, RandomContrast, RandomSaturation,
                                     RandomGrayscale, RandomSolarization, GaussianBlur)
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})

    def graph(ops, device='cuda:0'):
        r = Reader(raw)
        return Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                     r.metadata, OSCacheManager(r).compile_reader(), device=device)

    def absorbed(ops):
        return [i for i, o in enumerate(ops) if getattr(o, '_absorbed', False)]

    # five distinct kinds: the run closes at three steps, the next two form a second run
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomContrast(0.4), RandomSaturation(0.4),
           RandomGrayscale(0.2), RandomSolarization(128), ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 3, 5] and ops[1]._program == ops[1:4] and ops[4]._program == ops[4:6]
    g.collect_requirements()
    assert g.groupable()
    # the blur in between ends a run; a repeated new kind splits one
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomGrayscale(0.2), GaussianBlur(5),
           RandomSolarization(128), RandomGrayscale(0.5), RandomSolarization(10), Cutout(4), ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 5]
    assert ops[1]._program == ops[1:3] and ops[4]._program == ops[4:6] and ops[6]._program == [ops[6]]
    g.collect_requirements()
    assert g.groupable() and not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes[:-1])
    # a CPU graph lowers nothing
    ops = [SimpleRGBImageDecoder(), RandomGrayscale(0.2), RandomSolarization(128), ToTensor()]
    graph(ops, device='cpu')
    assert absorbed(ops) == [] and ops[1]._program == [ops[1]]
    # the chains asserted in tests/test_color_jitter.py lower as before
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.1), RandomContrast(0.1), RandomBrightness(0.2),
           RandomSaturation(0.2), Cutout(4), RandomSaturation(0.3), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [2, 4]
    assert ops[1]._program == ops[1:3] and ops[3]._program == ops[3:5] and ops[6]._program == [ops[6]]
