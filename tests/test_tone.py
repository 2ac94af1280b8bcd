"""RandomPosterize / RandomAutocontrast / RandomEqualize / RandomInvert on the
host (no GPU): the statement (tests/tone_ref.py) against Pillow's ImageOps, the
host twin of ffcv_tone_batch against the statement for every ordered program
of one to three steps, autocontrast's table for every pair of ends, the draws
(op ids 15..18) against numpy's RandomState, the transforms on host arrays and
in a CPU Loader, argument checks of the classes and of the C entries, and the
graph lowering of runs of the new operations."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import tone_ref as R
from tests.helpers import NaturalDS, write


@pytest.fixture(scope='module')
def image_set():
    batches = R.image_set()
    for b in batches:
        b.setflags(write=False)
    return batches


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _programs(max_len):
    return [p for n in range(1, max_len + 1) for p in itertools.permutations(R.KINDS, n)]


# ------------------------------------------------------------ statement --
def test_the_statement_equals_pillow(image_set):
    """ImageOps.invert, posterize (bits 1..8), autocontrast and equalize on 400
    images of five families, 1 x 1 to 39 x 39; the set holds channels where
    equalize exceeds 255 before the min, channels with step == 0 and channels
    with hi <= lo."""
    from PIL import Image, ImageOps
    assert sum(len(b) for b in image_set) >= 400
    assert {b.shape[1:3] for b in image_set} >= {(1, 1), (39, 39)}
    over, step0, single = 0, 0, 0
    for batch in image_set:
        for img in batch:
            pil = Image.fromarray(np.ascontiguousarray(img), 'RGB')
            assert np.array_equal(R.step_np(img, R.INVERT), np.asarray(ImageOps.invert(pil)))
            for bits in range(1, 9):
                assert np.array_equal(R.step_np(img, R.POSTERIZE, bits), np.asarray(ImageOps.posterize(pil, bits)))
            assert np.array_equal(R.step_np(img, R.AUTOCONTRAST), np.asarray(ImageOps.autocontrast(pil)))
            assert np.array_equal(R.step_np(img, R.EQUALIZE), np.asarray(ImageOps.equalize(pil)))
            for c in range(3):
                h = R.histogram(img[..., c])
                raw, step = R.equalize_raw(h)
                over += raw is not None and max(raw) > 255
                step0 += step == 0
                single += np.count_nonzero(h) == 1
    print('channels: over 255 before the min', over, '; step == 0', step0, '; hi <= lo', single)
    assert over > 0 and step0 > 0 and single > 0


# ------------------------------------------------------------ host twin --
@pytest.mark.parametrize('n_steps', (1, 2, 3))
def test_host_twin_equals_the_statement_for_every_program(hip_lib, image_set, n_steps):
    """Every ordered program of n distinct steps on every batch of the set (8
    images of one shape), with mixed apply flags: image 0 runs every step, image
    2 none and comes back untouched.  A twin that built a later step's table
    from the original histogram would fail here."""
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(100 + n_steps)
    for j, program in enumerate(itertools.permutations(R.KINDS, n_steps)):
        bits = 1 + j % 8
        apply = (rng.random((n_steps, 8)) < 0.6).astype(np.uint8)
        apply[:, 0], apply[:, 2] = 1, 0
        for batch in image_set:
            got = L.tone_batch_host(batch.copy(), program, bits, apply)
            want = R.apply_program_batch(batch, program, bits, apply)
            bad = [k for k in range(8) if not np.array_equal(got[k], want[k])]
            assert not bad, (program, bits, batch.shape, bad)
            assert np.array_equal(got[2], batch[2])


def test_four_step_programs_and_the_order_of_steps(hip_lib):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(5)
    batch = np.stack([R.family(rng, f, 23, 31) for f in R.FAMILIES + ('flat',)])
    ones = np.ones((4, len(batch)), np.uint8)
    results = set()
    for program in itertools.permutations(R.KINDS, 4):
        got = L.tone_batch_host(batch.copy(), program, 2, ones)
        assert np.array_equal(got, R.apply_program_batch(batch, program, 2, ones)), program
        results.add(got.tobytes())
    assert len(results) > 6                              # the order matters


def test_autocontrast_table_for_every_pair_of_ends(hip_lib):
    """All 32,640 pairs lo < hi, every entry of the table: v * scale + offset
    with the product and the sum rounded separately, truncated toward zero.
    This pins the evaluation order: see DESIGN.md s22 for what a contracted
    multiply-add would change."""
    from ffcv_amd import libffcv as L
    lo, hi = (a.reshape(-1) for a in np.triu_indices(256, 1))
    assert lo.size == 32640 and (lo < hi).all()
    hists = np.zeros((lo.size, 256), np.uint32)
    hists[np.arange(lo.size), lo] = 3
    hists[np.arange(lo.size), hi] = 1
    got = L.tone_tables_host(R.AUTOCONTRAST, 8, hists)
    scale = np.float64(255.0) / (hi - lo).astype(np.float64)
    offset = -lo.astype(np.float64) * scale
    prod = np.arange(256, dtype=np.float64)[None, :] * scale[:, None]
    want = np.clip(np.trunc(prod + offset[:, None]), 0, 255).astype(np.uint8)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (bad.size, int(lo[bad[0]]), int(hi[bad[0]]))
    rng = np.random.default_rng(1)
    for j in rng.integers(0, lo.size, 200):               # the vectorised form is the plain-Python statement
        assert want[j].tolist() == R.autocontrast_table(hists[j])
    assert (got[:, 0] == 0).all() and (got[np.arange(lo.size), lo] == 0).all()
    # the separately rounded sum leaves the top end at 254 for some pairs (Pillow's own result); one rounding
    # would give 255 there: lo = 1, hi = 10 is the first of the 8,484 pairs a fused multiply-add changes
    j = int(np.nonzero((lo == 1) & (hi == 10))[0][0])
    assert got[j, 10] == 254 and got[j, 7] == 169
    print('pairs whose top end maps below 255:', int((got[np.arange(lo.size), hi] != 255).sum()))
    # the other tables from the builder, and its argument checks
    h = rng.integers(0, 50, (40, 256)).astype(np.uint32)
    h[:5, 3:] = 0
    assert L.tone_tables_host(R.EQUALIZE, 8, h).tolist() == [R.equalize_table(x) for x in h]
    assert L.tone_tables_host(R.INVERT, 8, h[:1]).tolist() == [R.invert_table()]
    assert L.tone_tables_host(R.POSTERIZE, 3, h[:1]).tolist() == [R.posterize_table(3)]
    for kind, bits in ((0, 8), (5, 8), (R.POSTERIZE, 0), (R.POSTERIZE, 9)):
        with pytest.raises(L.FFCVError, match='ffcv_tone_tables_host'):
            L.tone_tables_host(kind, bits, h)


# ---------------------------------------------------------------- draws --
@pytest.mark.parametrize('kind', R.KINDS)
def test_host_draws_match_randomstate(hip_lib, kind):
    from ffcv_amd import libffcv as L
    n = 300
    rng = np.random.default_rng(11)
    seeds = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    seeds[:3] = (0, 1, 2 ** 63 + 5)
    epochs = rng.integers(0, 500, n)
    ids = rng.integers(0, 2 ** 20, n).astype(np.uint64)
    ids[n // 2:] = rng.integers(2 ** 32, 2 ** 48, n - n // 2).astype(np.uint64)   # beyond 32 bits
    op = R.OP_ID[kind]
    hits = 0
    for s, e, i in zip(seeds, epochs, ids):
        p = float(rng.random())
        got = L.tone_draw_batch_host([i], int(s), int(e), [op], [p])
        want = R.draw(int(s), int(e), int(i), kind, p)
        assert got.shape == (1, 1) and bool(got[0, 0]) == want
        hits += want
    assert 90 < hits < 210
    # four operations at once: a row per operation, each from its own stream
    ops, ps = [R.OP_ID[k] for k in (R.INVERT, R.POSTERIZE, R.EQUALIZE, R.AUTOCONTRAST)], [0.5, 0.2, 1.0, 0.0]
    got = L.tone_draw_batch_host(ids, 7, 3, ops, ps)
    assert got.shape == (4, n) and got[2].all() and not got[3].any()
    for row, k, p in zip(got, (R.INVERT, R.POSTERIZE, R.EQUALIZE, R.AUTOCONTRAST), ps):
        assert row.tolist() == [int(R.draw(7, 3, int(i), k, p)) for i in ids]


# ----------------------------------------------------------- transforms --
def test_public_names_and_arguments():
    import inspect
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    from ffcv.transforms import RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
    from ffcv_amd.transforms.color_jitter import _ColorJitter
    for cls, op_id in ((RandomPosterize, 15), (RandomAutocontrast, 16), (RandomEqualize, 17), (RandomInvert, 18)):
        assert getattr(T, cls.__name__) is cls and getattr(FT, cls.__name__) is cls and cls.__name__ in T.__all__
        assert not issubclass(cls, _ColorJitter) and cls.op_id == op_id and cls.per_sample and cls.device_aware
    sig = lambda c: [(p.name, p.default) for p in inspect.signature(c.__init__).parameters.values()][1:]  # noqa: E731
    assert sig(RandomPosterize) == [('bits', inspect.Parameter.empty), ('p', 0.5)]
    for cls in (RandomAutocontrast, RandomEqualize, RandomInvert):
        assert sig(cls) == [('p', 0.5)]
        assert cls().p == 0.5 and cls(1).p == 1 and cls(p=0.0).p == 0.0
        for bad in (-0.01, 1.01, float('nan'), None, 'x'):
            with pytest.raises(ValueError, match=f'{cls.__name__}: p'):
                cls(bad)
    assert (RandomPosterize(4).bits, RandomPosterize(4).p) == (4, 0.5) and RandomPosterize(np.int64(1), 1).bits == 1
    for bad in (0, 9, -1, 4.0, True, None, '4'):
        with pytest.raises(ValueError, match='RandomPosterize: bits'):
            RandomPosterize(bad)
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError, match='RandomPosterize: p'):
            RandomPosterize(4, bad)


def test_state_must_be_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
    for op in (RandomPosterize(4), RandomAutocontrast(), RandomEqualize(), RandomInvert()):
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
        assert alloc is None and st.shape == (8, 6, 3) and st.jit_mode
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
        assert alloc is None and not st.jit_mode
        for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('u1'), (8, 6))):
            with pytest.raises(TypeError, match=f'{type(op).__name__} works on uint8'):
                op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_operations_on_host_arrays_are_the_sequential_numpy_chain():
    from ffcv_amd.transforms import RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
    rng = np.random.default_rng(6)
    ids = np.array([0, 1, 2, 3, 50, 2 ** 33 + 1, 77, 1000, 4, 5, 6, 7])
    imgs = np.stack([R.family(rng, R.FAMILIES[k % 5], 13, 10) for k in range(len(ids))])
    chain = [(RandomPosterize(3, p=0.6), R.POSTERIZE), (RandomEqualize(p=0.5), R.EQUALIZE),
             (RandomInvert(p=0.4), R.INVERT), (RandomAutocontrast(p=0.7), R.AUTOCONTRAST)]
    work = imgs.copy()
    for op, _ in chain:
        code = op.generate_code()
        assert code.with_indices and code(work, None, ids) is work    # in place; outside a Loader: seed 0, epoch 0
    apply = [[R.draw(0, 0, int(s), kind, op.p) for s in ids] for op, kind in chain]
    assert all(1 < sum(row) < len(ids) for row in apply)
    assert np.array_equal(work, R.apply_program_batch(imgs, [k for _, k in chain], 3, apply))
    view = np.zeros((13, 10, 4), np.uint8)[..., :3]                   # not contiguous: still in place
    for op, kind in chain:
        view[...] = imgs[0]
        type(op).host_fn(view, 3)
        assert np.array_equal(view, R.step_np(imgs[0], kind, 3)), kind


# ------------------------------------------------------------------ ABI --
def test_abi_rejects_bad_arguments(hip_lib):
    """The batch and draw entries, the device ones included: a bad argument
    comes back as FFCV_EINVAL before any launch (no GPU is touched), with the
    entry's name in ffcv_last_error and every buffer as it was."""
    from ffcv_amd import libffcv as L
    lib = L.lib()
    B = 2
    img = np.full((B, 4, 4, 3), 77, np.uint8)
    img[0, 0, 0] = 99
    before = img.copy()
    ids = np.arange(B, dtype=np.uint64)
    apply = np.ones((4, B), np.uint8)
    ws = np.zeros(768 * B + 1, np.uint32)
    i, a, d, w = _ptr(img), _ptr(apply), _ptr(ids), _ptr(ws)
    good = L.tone_params([R.POSTERIZE, R.EQUALIZE], 4)
    g = ctypes.byref(good)

    def rejected(name, rc):
        assert rc == -1 and (name + ':').encode() in lib.ffcv_last_error(), (name, lib.ffcv_last_error())

    shape_args = ((None, B, 4, 4, g, a), (i, B, 4, 4, None, a), (i, B, 4, 4, g, None), (i, -1, 4, 4, g, a),
                  (i, B, 0, 4, g, a), (i, B, 4, 0, g, a), (i, B, -4, 4, g, a), (i, B, 26755, 26755, g, a),
                  (i, B, 2 ** 31 - 1, 2, g, a))
    bad_programs = [L.tone_params([], 4), L.tone_params([1, 2, 3, 4], 4), L.tone_params([0], 4),
                    L.tone_params([5], 4), L.tone_params([R.INVERT, R.EQUALIZE, R.INVERT], 4),
                    L.tone_params([R.POSTERIZE], 0), L.tone_params([R.EQUALIZE, R.POSTERIZE], 9)]
    bad_programs[1].n_steps = 5
    for args in shape_args + tuple((i, B, 4, 4, ctypes.byref(p), a) for p in bad_programs):
        rejected('ffcv_tone_batch_host', lib.ffcv_tone_batch_host(*args))
        rejected('ffcv_tone_batch', lib.ffcv_tone_batch(None, *args, w, ws.nbytes))
    # beyond the whole-image regime a statistics step needs its workspace
    assert 80 * 80 * 3 > L.tone_lds_bytes() and L.tone_workspace_bytes(B) == 3072 * B == ws.nbytes - 4
    for wsp, nbytes in ((None, 0), (None, ws.nbytes), (w, 3072 * B - 1), (ctypes.c_void_p(ws.ctypes.data + 2), 3072 * B)):
        rejected('ffcv_tone_batch', lib.ffcv_tone_batch(None, i, B, 80, 80, g, a, wsp, nbytes))
    ops, ps = np.array([15, 18], np.int32), np.array([0.5, 0.5])
    o, p = _ptr(ops), _ptr(ps)
    nan = float('nan')
    draw_args = ((None, B, 0, 0, 2, o, p, a), (d, B, 0, 0, 2, None, p, a), (d, B, 0, 0, 2, o, None, a),
                 (d, B, 0, 0, 2, o, p, None), (d, -1, 0, 0, 2, o, p, a), (d, B, 0, 0, 0, o, p, a),
                 (d, B, 0, 0, 5, o, p, a)) + \
        tuple((d, B, 0, 0, 2, _ptr(np.array([15, bad], np.int32)), p, a) for bad in (14, 19, 5, 0, -1)) + \
        tuple((d, B, 0, 0, 2, o, _ptr(np.array([0.5, bad])), a) for bad in (-0.1, 1.1, nan))
    for args in draw_args:
        rejected('ffcv_tone_draw_batch_host', lib.ffcv_tone_draw_batch_host(*args))
        rejected('ffcv_tone_draw_batch', lib.ffcv_tone_draw_batch(None, *args, None))
    assert np.array_equal(img, before) and (apply == 1).all() and not ws.any()
    # the older draw entries keep rejecting the new op ids
    val = np.zeros(B)
    for op_id in (15, 16, 17, 18):
        assert lib.ffcv_uniform_draw_batch_host(d, B, 0, 0, op_id, 0.5, 0.0, 0.0, a, _ptr(val)) == -1
        assert lib.ffcv_color_jitter_draw_batch_host(d, B, 0, 0, op_id, 0.5, 0.1, a, _ptr(val)) == -1
    # B == 0 is fine, on every entry
    assert lib.ffcv_tone_batch_host(i, 0, 4, 4, g, a) == 0 and lib.ffcv_tone_batch(None, i, 0, 80, 80, g, a, None, 0) == 0
    assert lib.ffcv_tone_draw_batch_host(d, 0, 0, 0, 2, o, p, a) == 0
    assert lib.ffcv_tone_draw_batch(None, d, 0, 0, 0, 2, o, p, a, None) == 0
    assert np.array_equal(img, before) and (apply == 1).all()
    with pytest.raises(TypeError):
        L.tone_batch_host(img.transpose(0, 2, 1, 3), [R.INVERT], 8, apply[:1])
    with pytest.raises(TypeError):
        L.tone_draw_batch_host(ids, 0, 0, [15, 16], [0.5])


# ---------------------------------------------------------------- graph --
def test_graph_lowering_of_tone_runs(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (ToTensor, RandomBrightness, RandomContrast, RandomSolarization,
                                     RandomHorizontalFlip, RandomPosterize, RandomAutocontrast, RandomEqualize,
                                     RandomInvert)
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

    # adjacent: one run, the first carries the program
    ops = [SimpleRGBImageDecoder(), RandomPosterize(4), RandomEqualize(), RandomAutocontrast(), RandomInvert(),
           ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 3, 4] and ops[1]._program == ops[1:5]
    g.collect_requirements()
    assert g.groupable() and no_host_hop(g)
    # split by a foreign operation (a flip, a colour-jitter operation): two runs; the colour run is its own
    ops = [SimpleRGBImageDecoder(), RandomEqualize(), RandomInvert(), RandomHorizontalFlip(), RandomAutocontrast(),
           RandomBrightness(0.4), RandomContrast(0.4), RandomSolarization(128), RandomPosterize(2), RandomInvert(),
           ToTensor()]
    g = graph(ops)
    assert absorbed(ops) == [2, 6, 7, 9]
    assert ops[1]._program == ops[1:3] and ops[4]._program == [ops[4]] and ops[5]._program == ops[5:8]
    assert ops[8]._program == ops[8:10]
    g.collect_requirements()
    assert g.groupable() and no_host_hop(g)
    # a repeated type starts a new run
    ops = [SimpleRGBImageDecoder(), RandomInvert(), RandomPosterize(4), RandomInvert(), RandomEqualize(),
           RandomPosterize(2), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [2, 4, 5] and ops[1]._program == ops[1:3] and ops[3]._program == ops[3:6]
    # five in a row: the fifth repeats a type, so it starts a new run
    ops = [SimpleRGBImageDecoder(), RandomInvert(), RandomPosterize(4), RandomEqualize(), RandomAutocontrast(),
           RandomEqualize(), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [2, 3, 4] and ops[1]._program == ops[1:5] and ops[5]._program == [ops[5]]
    # an operation on two nodes stays alone
    shared = RandomInvert()
    ops = [SimpleRGBImageDecoder(), RandomPosterize(4), shared, shared, RandomEqualize(), ToTensor()]
    graph(ops)
    assert absorbed(ops) == [] and ops[1]._program == [ops[1]] and ops[4]._program == [ops[4]]
    # a CPU graph lowers nothing
    ops = [SimpleRGBImageDecoder(), RandomPosterize(4), RandomEqualize(), ToTensor()]
    g = graph(ops, device='cpu')
    g.collect_requirements()
    assert absorbed(ops) == [] and g.groupable()


# --------------------------------------------------------------- Loader --
def test_cpu_loader_equals_the_numpy_chain(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'tone.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    seed = 12
    steps, ps = [R.POSTERIZE, R.AUTOCONTRAST, R.EQUALIZE, R.INVERT], [0.5, 0.6, 0.4, 0.3]
    loader = Loader(fn, batch_size=8, device='cpu', seed=seed, pipelines={
        'image': [SimpleRGBImageDecoder(), RandomPosterize(3, p=ps[0]), RandomAutocontrast(p=ps[1]),
                  RandomEqualize(p=ps[2]), RandomInvert(p=ps[3]), ToTensor()]})
    for epoch in range(2):
        got = np.concatenate([images.numpy() for images, _ in loader])
        assert got.shape == (24, 32, 32, 3) and got.dtype == np.uint8
        apply = [[R.draw(seed, epoch, sid, kind, p) for sid in range(24)] for kind, p in zip(steps, ps)]
        assert all(3 < sum(row) < 21 for row in apply)
        want = R.apply_program_batch(np.stack(ds.imgs), steps, 3, apply)
        bad = [k for k in range(24) if not np.array_equal(got[k], want[k])]
        assert not bad, (epoch, bad)
