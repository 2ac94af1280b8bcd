"""RandomHue / RandomColorJitter on the host (no GPU): the draws (op ids 12
and 13) against numpy's RandomState, the host twin of ffcv_hue_batch against
the numpy statement of the contract (tests/hue_ref.py) on all 2^24 RGB
triples, the evaluation order, the transforms on host arrays and in a CPU
Loader, argument checks of the classes and of the six C entries, and the graph
lowering around the new operations."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import hue_ref as R
from tests.color_jitter_ref import BRIGHTNESS, CONTRAST, SATURATION
from tests.helpers import NaturalDS, write

EXHAUSTIVE_D = (0.05, 0.23, -0.37)   # the d at which a fused multiply-add changes triples


@pytest.fixture(scope='module')
def triples():
    return R.all_triples()


@pytest.fixture(scope='module')
def reference(triples):
    """tests/hue_ref.py on all triples at d, computed once per d and shared (read only)."""
    cache = {}

    def ref(d):
        if d not in cache:
            cache[d] = R.hue_np(triples, d)
            cache[d].setflags(write=False)
        return cache[d]
    return ref


def _host(imgs, apply, shift):
    from ffcv_amd import libffcv as L
    out = np.ascontiguousarray(imgs).copy()
    L.hue_batch_host(out, apply, shift)
    return out


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _draw_cases(n=300):
    rng = np.random.default_rng(11)
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    seeds[:3] = (0, 1, 2 ** 63 + 5)
    epochs = rng.integers(0, 500, n)
    ids = rng.integers(0, 2 ** 20, n).astype(np.uint64)
    ids[n // 2:] = rng.integers(2 ** 32, 2 ** 48, n - n // 2).astype(np.uint64)   # beyond 32 bits
    return seeds, epochs, ids


# ---------------------------------------------------------------- draws --
def test_hue_draws_match_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    seeds, epochs, ids = _draw_cases()
    applied = 0
    for k in range(len(ids)):
        p, m = (0.5, 0.1) if k % 2 else (0.8, 0.5)
        a, d = L.hue_draw_batch_host(ids[k:k + 1], int(seeds[k]), int(epochs[k]), p, m)
        wa, wd = R.hue_draw(int(seeds[k]), int(epochs[k]), int(ids[k]), p, m)
        assert a[0] == wa and d.view(np.uint64)[0] == np.float64(wd).view(np.uint64), k
        assert abs(d[0]) <= m
        applied += int(a[0])
    assert 120 < applied < 260
    # a batch is its samples side by side; p = 0 / 1 and magnitude 0
    a, d = L.hue_draw_batch_host(ids, 7, 3, 0.5, 0.25)
    for k in (0, 1, 150, 299):
        wa, wd = R.hue_draw(7, 3, int(ids[k]), 0.5, 0.25)
        assert a[k] == wa and d[k] == wd
    assert not L.hue_draw_batch_host(ids, 7, 3, 0.0, 0.1)[0].any()
    a, d = L.hue_draw_batch_host(ids, 7, 3, 1.0, 0.0)
    assert a.all() and (d == 0).all()


def test_joint_draws_match_randomstate(hip_lib):
    from ffcv_amd import libffcv as L
    seeds, epochs, ids = _draw_cases()
    mags = (0.4, 0.4, 0.2, 0.1)
    for k in range(len(ids)):
        a, v = L.color_jitter_joint_draw_batch_host(ids[k:k + 1], int(seeds[k]), int(epochs[k]), 0.8, mags)
        wa, wv = R.joint_draw(int(seeds[k]), int(epochs[k]), int(ids[k]), 0.8, mags)
        assert a.shape == (4, 1) and (a[:, 0] == wa).all(), k
        assert np.array_equal(v[:, 0].view(np.uint64), np.array(wv, np.float64).view(np.uint64)), k
    # the five draws come from ONE stream of op id 13, not from the streams of the separate operations
    from ffcv_amd.transforms.rng import contract_seed
    rs = np.random.RandomState(contract_seed(5, 2, 77, 13))
    five = [rs.rand(), rs.uniform(0.6, 1.4), rs.uniform(0.6, 1.4), rs.uniform(0.8, 1.2), rs.uniform(-0.1, 0.1)]
    a, v = L.color_jitter_joint_draw_batch_host(np.array([77], np.uint64), 5, 2, 0.8, mags)
    assert (a[:, 0] == (five[0] < 0.8)).all() and list(v[:, 0]) == five[1:]


def test_joint_draw_compacts_rows_for_every_subset_of_zero_magnitudes(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    full = (0.4, 1.5, 0.2, 0.1)
    ids = np.array([0, 5, 2 ** 40 + 3, 99, 12345, 7], np.uint64)
    B = len(ids)
    for active in itertools.product((0, 1), repeat=4):
        mags = np.array([m if on else 0.0 for m, on in zip(full, active)])
        rows = sum(active)
        assert L.color_jitter_joint_rows(mags) == rows
        apply = np.full((5, B), 9, np.uint8)
        ratio = np.full((5, B), -7.0)
        assert lib.ffcv_color_jitter_joint_draw_batch_host(_ptr(ids), B, 21, 4, 0.6, _ptr(mags), _ptr(apply),
                                                           _ptr(ratio)) == 0
        assert (apply[rows:] == 9).all() and (ratio[rows:] == -7.0).all()     # only `rows` rows are written
        for k in range(B):
            wa, wv = R.joint_draw(21, 4, int(ids[k]), 0.6, list(mags))       # all five drawn, whatever is zero
            assert (apply[:rows, k] == wa).all()
            want = [wv[j] for j in range(4) if active[j]]
            assert list(ratio[:rows, k]) == want, (active, k)
        a, v = L.color_jitter_joint_draw_batch_host(ids, 21, 4, 0.6, mags)
        assert a.shape == (rows, B) and np.array_equal(a, apply[:rows]) and np.array_equal(v, ratio[:rows])


def test_existing_draw_entries_still_reject_the_new_op_ids(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ids = np.arange(4, dtype=np.uint64)
    apply, value = np.full(4, 9, np.uint8), np.full(4, -7.0)
    for op_id in (12, 13):
        assert lib.ffcv_color_jitter_draw_batch_host(_ptr(ids), 4, 0, 0, op_id, 0.5, 0.4, _ptr(apply),
                                                     _ptr(value)) == -1
        assert lib.ffcv_uniform_draw_batch_host(_ptr(ids), 4, 0, 0, op_id, 0.5, 0.0, 1.0, _ptr(apply),
                                                _ptr(value)) == -1
        with pytest.raises(L.FFCVError):
            L.color_jitter_draw_batch_host(ids, 0, 0, op_id, 0.5, 0.4)
        with pytest.raises(L.FFCVError):
            L.uniform_draw_batch_host(ids, 0, 0, op_id, 0.5, 0.0, 1.0)
    assert (apply == 9).all() and (value == -7.0).all()
    # the two ids are served by the entries of their own
    assert L.hue_draw_batch_host(ids, 0, 0, 0.5, 0.4)[1].shape == (4,)
    assert L.color_jitter_joint_draw_batch_host(ids, 0, 0, 0.5, (0.4, 0.4, 0.2, 0.1))[1].shape == (4, 4)


# --------------------------------------------------------------- pixels --
@pytest.mark.parametrize('d', EXHAUSTIVE_D)
def test_host_twin_equals_numpy_on_all_triples(hip_lib, triples, reference, d):
    got = _host(triples[None], [1], [d])[0]
    want = reference(d)
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    assert (got != triples).any(-1).sum() > 2 ** 23


def test_identities_on_all_triples(hip_lib, triples):
    batch = np.stack([triples, triples])
    assert np.array_equal(_host(batch, [1, 1], [0.0, -0.0]), batch)
    once = _host(batch, [1, 1], [0.5, -0.5])
    assert (once[0] != triples).any(-1).sum() > 2 ** 23
    assert np.array_equal(_host(once, [1, 1], [0.5, -0.5]), batch)       # half a turn twice
    assert np.array_equal(_host(batch, [0, 0], [0.3, 0.3]), batch)       # apply = 0


def test_gray_pixels_and_hand_values(hip_lib):
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1).reshape(1, 16, 16, 3)
    for d in (0.05, -0.37, 0.5, 1 / 3):
        assert np.array_equal(_host(gray, [1], [d]), gray)
        assert np.array_equal(R.hue_np(gray[0], d), gray[0])
    px = np.array([[255, 0, 0], [10, 200, 30]], np.uint8).reshape(1, 1, 2, 3)
    assert _host(px, [1], [1 / 3])[0, 0, 0].tolist() == [0, 255, 0]      # pure red, a third of a turn: pure green
    assert _host(px, [1], [0.1])[0, 0, 1].tolist() == [10, 200, 144]
    assert R.hue_np(px[0], 1 / 3)[0, 0].tolist() == [0, 255, 0]
    assert R.hue_np(px[0], 0.1)[0, 1].tolist() == [10, 200, 144]
    # a batch: each image with its own d, the middle one left alone
    rng = np.random.default_rng(3)
    imgs = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    got = _host(imgs, [1, 0, 1], [0.2, 0.4, -0.45])
    assert np.array_equal(got[0], R.hue_np(imgs[0], 0.2)) and np.array_equal(got[1], imgs[1])
    assert np.array_equal(got[2], R.hue_np(imgs[2], -0.45))


def test_the_exhaustive_case_pins_the_evaluation_order(hip_lib, triples, reference):
    """1 - s * f and 1 - s * (1 - f) computed with one rounding, as a fused
    multiply-add would, give other bytes on some triples at d = 0.05 (87,959
    when this was written), so the exhaustive comparison above fails for a
    kernel or a twin that contracts them; the host twin sides with the
    contract on a triple where the two differ."""
    want = reference(0.05)
    fused = R.hue_np(triples, 0.05, contracted=True)
    differ = (want != fused).any(-1)
    n = int(differ.sum())
    print('triples changed by contraction at d = 0.05:', n)
    assert n > 0
    y, x = (int(v[0]) for v in np.nonzero(differ))
    got = _host(triples[y:y + 1, x:x + 1][None], [1], [0.05])[0, 0, 0]
    assert np.array_equal(got, want[y, x]) and not np.array_equal(got, fused[y, x])


def test_module_numpy_statement_equals_the_reference_statement():
    from ffcv_amd.transforms.hue import hue_np
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (37, 41, 3), dtype=np.uint8)
    img[:4] = img[:4, :, :1]                                             # gray rows
    for d in (0.0, 0.05, 0.23, -0.37, 0.5, -0.5, 1 / 3):
        work = img.copy()
        assert hue_np(work, d) is work and np.array_equal(work, R.hue_np(img, d)), d
    view = np.zeros((37, 41, 4), np.uint8)[..., :3]                      # not contiguous: still in place
    view[...] = img
    hue_np(view, 0.23)
    assert np.array_equal(view, R.hue_np(img, 0.23))


# ----------------------------------------------------------- transforms --
def test_public_names_and_arguments():
    import inspect
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    from ffcv.transforms import RandomHue, RandomColorJitter            # the alias package
    from ffcv_amd.transforms.color_jitter import _ColorJitter
    for cls, op_id in ((RandomHue, 12), (RandomColorJitter, 13)):
        assert getattr(T, cls.__name__) is cls and getattr(FT, cls.__name__) is cls and cls.__name__ in T.__all__
        assert not issubclass(cls, _ColorJitter) and cls.op_id == op_id and cls.per_sample and cls.device_aware
    sig = lambda c: [(p.name, p.default) for p in inspect.signature(c.__init__).parameters.values()][1:]  # noqa: E731
    assert sig(RandomHue) == [('magnitude', inspect.Parameter.empty), ('p', 0.5)]
    assert sig(RandomColorJitter) == [('brightness', 0.0), ('contrast', 0.0), ('saturation', 0.0), ('hue', 0.0),
                                      ('p', 0.8)]
    h = RandomHue(0.1)
    assert (h.magnitude, h.p) == (0.1, 0.5) and RandomHue(0.5, 1).p == 1 and RandomHue(0).magnitude == 0
    j = RandomColorJitter(0.4, 0.4, 0.2, 0.1)
    assert j.magnitudes == [0.4, 0.4, 0.2, 0.1] and j.p == 0.8
    for bad in (-0.01, 0.51, float('nan'), float('inf'), None, 'x'):
        with pytest.raises(ValueError, match='RandomHue: magnitude'):
            RandomHue(bad)
        with pytest.raises(ValueError, match='RandomColorJitter: hue'):
            RandomColorJitter(hue=bad)
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError, match='RandomHue: p'):
            RandomHue(0.1, bad)
        with pytest.raises(ValueError, match='RandomColorJitter: p'):
            RandomColorJitter(0.4, p=bad)
    for name in ('brightness', 'contrast', 'saturation'):
        for bad in (-0.01, float('nan'), float('inf'), None, 'x'):
            with pytest.raises(ValueError, match=f'RandomColorJitter: {name}'):
                RandomColorJitter(**{name: bad})
        RandomColorJitter(**{name: 3.5})                                 # no upper bound, as RandomBrightness


def test_state_must_be_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomHue, RandomColorJitter
    for op in (RandomHue(0.1), RandomColorJitter(0.4, 0.4, 0.2, 0.1)):
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
        assert alloc is None and st.shape == (8, 6, 3) and st.jit_mode
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
        assert alloc is None and not st.jit_mode
        for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('u1'), (8, 6))):
            with pytest.raises(TypeError, match=f'{type(op).__name__} works on uint8'):
                op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


@pytest.mark.parametrize('mags', ((0.4, 0.4, 0.2, 0.1), (0.0, 0.0, 0.0, 0.3), (0.5, 0.7, 0.0, 0.0)),
                         ids=('all', 'hue_only', 'b_c_only'))
def test_color_jitter_on_host_arrays_is_the_sequential_numpy_chain(mags):
    from ffcv_amd.transforms import RandomColorJitter
    rng = np.random.default_rng(6)
    ids = np.array([0, 1, 2, 3, 50, 2 ** 33 + 1, 77, 1000, 4, 5, 6, 7])
    imgs = rng.integers(0, 256, (len(ids), 13, 10, 3), dtype=np.uint8)
    code = RandomColorJitter(*mags, p=0.6).generate_code()
    assert code.with_indices
    work = imgs.copy()
    assert code(work, None, ids) is work                                 # in place; outside a Loader: seed 0, epoch 0
    draws = [R.joint_draw(0, 0, int(s), 0.6, mags) for s in ids]
    applied = [a for a, _ in draws]
    assert 2 < sum(applied) < len(ids)
    for k, (a, v) in enumerate(draws):
        want = imgs[k].copy()
        if a:
            for kind, m, r in zip((BRIGHTNESS, CONTRAST, SATURATION), mags[:3], v[:3]):
                if m:
                    want = R.jitter_np(want, kind, r)
            if mags[3]:
                want = R.hue_np(want, v[3])
            assert not np.array_equal(want, imgs[k])
        assert np.array_equal(work[k], want), (mags, k, a)
    assert np.array_equal(work, R.joint_batch(imgs, ids, 0, 0, 0.6, mags))
    # p = 0: all drawn, nothing run; every magnitude 0: nothing to run
    for op in (RandomColorJitter(*mags, p=0.0), RandomColorJitter(p=1.0)):
        work = imgs.copy()
        op.generate_code()(work, None, ids)
        assert np.array_equal(work, imgs)


def test_random_hue_on_host_arrays():
    from ffcv_amd.transforms import RandomHue
    rng = np.random.default_rng(7)
    ids = np.arange(20)
    imgs = rng.integers(0, 256, (20, 6, 9, 3), dtype=np.uint8)
    work = imgs.copy()
    RandomHue(0.3, p=0.5).generate_code()(work, None, ids)
    draws = [R.hue_draw(0, 0, int(s), 0.5, 0.3) for s in ids]
    assert 4 < sum(a for a, _ in draws) < 16
    for k, (a, d) in enumerate(draws):
        assert np.array_equal(work[k], R.hue_np(imgs[k], d) if a else imgs[k]), k


# ------------------------------------------------------------------ ABI --
def test_abi_rejects_bad_arguments(hip_lib):
    """All six entries, the device ones included: a bad argument comes back as
    FFCV_EINVAL before any launch (no GPU is touched), with the entry's name in
    ffcv_last_error and every buffer as it was."""
    from ffcv_amd import libffcv as L
    lib = L.lib()
    B = 2
    img = np.full((B, 4, 4, 3), 77, np.uint8)
    img[..., 0] = 99
    before = img.copy()
    ids = np.arange(B, dtype=np.uint64)
    apply, val = np.ones((4, B), np.uint8), np.full((4, B), 0.25)
    mags = np.array([0.4, 0.4, 0.2, 0.1])
    nan, inf = float('nan'), float('inf')
    i, a, v, d, m = _ptr(img), _ptr(apply), _ptr(val), _ptr(ids), _ptr(mags)

    def rejected(name, rc):
        assert rc == -1 and (name + ':').encode() in lib.ffcv_last_error(), (name, lib.ffcv_last_error())

    batch_args = ((None, B, 4, 4, a, v), (i, B, 4, 4, None, v), (i, B, 4, 4, a, None), (i, -1, 4, 4, a, v),
                  (i, B, 0, 4, a, v), (i, B, 4, 0, a, v), (i, B, -4, 4, a, v), (i, B, 26755, 26755, a, v),
                  (i, B, 2 ** 31 - 1, 2, a, v))
    for args in batch_args:
        rejected('ffcv_hue_batch_host', lib.ffcv_hue_batch_host(*args))
        rejected('ffcv_hue_batch', lib.ffcv_hue_batch(None, *args))
    draw_args = ((None, B, 0, 0, 0.5, 0.1, a, v), (d, B, 0, 0, 0.5, 0.1, None, v), (d, B, 0, 0, 0.5, 0.1, a, None),
                 (d, -1, 0, 0, 0.5, 0.1, a, v)) + \
        tuple((d, B, 0, 0, p, 0.1, a, v) for p in (-0.1, 1.1, nan, inf)) + \
        tuple((d, B, 0, 0, 0.5, mag, a, v) for mag in (-0.01, 0.5000001, nan, inf, -inf))
    for args in draw_args:
        rejected('ffcv_hue_draw_batch_host', lib.ffcv_hue_draw_batch_host(*args))
        rejected('ffcv_hue_draw_batch', lib.ffcv_hue_draw_batch(None, *args, None))
    bad_mags = [np.array(x) for x in ([-0.1, 0, 0, 0], [0, nan, 0, 0], [0, 0, inf, 0], [0, 0, 0, 0.51],
                                      [0, 0, 0, -0.1], [0, 0, 0, nan], [0.4, 0.4, 0.2, inf])]
    joint_args = ((None, B, 0, 0, 0.5, m, a, v), (d, B, 0, 0, 0.5, None, a, v), (d, B, 0, 0, 0.5, m, None, v),
                  (d, B, 0, 0, 0.5, m, a, None), (d, -1, 0, 0, 0.5, m, a, v)) + \
        tuple((d, B, 0, 0, p, m, a, v) for p in (-0.1, 1.1, nan)) + \
        tuple((d, B, 0, 0, 0.5, _ptr(bm), a, v) for bm in bad_mags)
    for args in joint_args:
        rejected('ffcv_color_jitter_joint_draw_batch_host', lib.ffcv_color_jitter_joint_draw_batch_host(*args))
        rejected('ffcv_color_jitter_joint_draw_batch', lib.ffcv_color_jitter_joint_draw_batch(None, *args, None))
    assert np.array_equal(img, before) and (apply == 1).all() and (val == 0.25).all()
    # B == 0 is fine, on every entry
    assert lib.ffcv_hue_batch_host(i, 0, 4, 4, a, v) == 0 and lib.ffcv_hue_batch(None, i, 0, 4, 4, a, v) == 0
    assert lib.ffcv_hue_draw_batch_host(d, 0, 0, 0, 0.5, 0.1, a, v) == 0
    assert lib.ffcv_hue_draw_batch(None, d, 0, 0, 0, 0.5, 0.1, a, v, None) == 0
    assert lib.ffcv_color_jitter_joint_draw_batch_host(d, 0, 0, 0, 0.5, m, a, v) == 0
    assert lib.ffcv_color_jitter_joint_draw_batch(None, d, 0, 0, 0, 0.5, m, a, v, None) == 0
    assert np.array_equal(img, before) and (apply == 1).all() and (val == 0.25).all()
    with pytest.raises(TypeError):
        L.hue_batch_host(img.transpose(0, 2, 1, 3), apply[0], val[0])
    with pytest.raises(TypeError):
        L.hue_batch_host(img, apply[0, :1], val[0])


# ---------------------------------------------------------------- graph --
def test_graph_lowering_around_the_new_operations(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, ToTensor, RandomBrightness, RandomContrast, RandomSaturation,
                                     RandomGrayscale, RandomSolarization, GaussianBlur, RandomHue,
                                     RandomColorJitter)
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})

    def graph(ops, device='cuda:0'):
        r = Reader(raw)
        return Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
                     r.metadata, OSCacheManager(r).compile_reader(), device=device)

    def absorbed(ops):
        return [i for i, o in enumerate(ops) if getattr(o, '_absorbed', False)]

    def no_host_hop(g):
        return not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes[:-1])

    # hue between two jitter operations: two separate colour runs
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomHue(0.1), RandomContrast(0.4), ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [] and ops[1]._program == [ops[1]] and ops[3]._program == [ops[3]]
    g.collect_requirements()
    assert g.groupable() and no_host_hop(g)
    # the joint jitter ends a run too; the SSL chain keeps its launch groups and stays on the device
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomContrast(0.4), RandomColorJitter(0.4, 0.4, 0.2, 0.1),
           RandomGrayscale(0.2), GaussianBlur(5), RandomSolarization(128), RandomSaturation(0.1), ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 7]
    assert ops[1]._program == ops[1:3] and ops[4]._program == [ops[4]] and ops[6]._program == ops[6:8]
    g.collect_requirements()
    assert g.groupable() and no_host_hop(g)
    # the runs of the five older kinds lower exactly as before (tests/test_gray_solarize.py)
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomContrast(0.4), RandomSaturation(0.4),
           RandomGrayscale(0.2), RandomSolarization(128), ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 3, 5] and ops[1]._program == ops[1:4] and ops[4]._program == ops[4:6]
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.4), RandomGrayscale(0.2), GaussianBlur(5),
           RandomSolarization(128), RandomGrayscale(0.5), RandomSolarization(10), Cutout(4), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [2, 5]
    assert ops[1]._program == ops[1:3] and ops[4]._program == ops[4:6] and ops[6]._program == [ops[6]]
    ops = [SimpleRGBImageDecoder(), RandomBrightness(0.1), RandomContrast(0.1), RandomBrightness(0.2),
           RandomSaturation(0.2), Cutout(4), RandomSaturation(0.3), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [2, 4]
    assert ops[1]._program == ops[1:3] and ops[3]._program == ops[3:5] and ops[6]._program == [ops[6]]
    # a CPU graph with the new operations lowers nothing
    ops = [SimpleRGBImageDecoder(), RandomHue(0.1), RandomColorJitter(0.4, 0.4, 0.2, 0.1), ToTensor()]
    g = graph(ops, device='cpu')
    g.collect_requirements()
    assert absorbed(ops) == [] and g.groupable()


# --------------------------------------------------------------- Loader --
def test_cpu_loader_color_jitter_equals_the_numpy_chain(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandomColorJitter, RandomHue
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'hue.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed, mags = 12, (0.4, 0.4, 0.2, 0.1)
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomColorJitter(*mags), RandomHue(0.25, p=0.5), ToTensor()]})
    for epoch in range(2):
        seen, jittered, turned = 0, 0, 0
        for b, (images, _) in enumerate(loader):
            got = images.numpy()
            assert got.shape == (8, 32, 32, 3) and got.dtype == np.uint8
            for k in range(8):
                sid = b * 8 + k
                a, v = R.joint_draw(seed, epoch, sid, 0.8, mags)
                want = R.joint_np(ds.imgs[sid], mags, a, v)
                ha, hd = R.hue_draw(seed, epoch, sid, 0.5, 0.25)
                if ha:
                    want = R.hue_np(want, hd)
                assert np.array_equal(got[k], want), (epoch, sid, a, ha)
                seen, jittered, turned = seen + 1, jittered + a, turned + ha
        assert seen == 24 and 12 < jittered < 24 and 5 < turned < 19
