"""TrivialAugmentWide on the host (no GPU): the host twin of the draws against
the numpy statement (tests/auto_augment_ref.py) in every output array, the
value tables against the integer forms, the per-sample-bits tone twin against
single-bits calls, a CPU Loader sample of every operation against the sibling
operation's numpy statement, argument checks and the public name."""
import ctypes

import numpy as np
import pytest

from tests import affine_ref as AR
from tests import auto_augment_ref as R
from tests import tone_ref as TR
from tests.helpers import NaturalDS, write

SEED = 11      # loader seed of the draw and Loader tests: ids 0 .. 2047 draw every operation with both signs


def test_public_name_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls = T.TrivialAugmentWide
    assert FT.TrivialAugmentWide is cls and 'TrivialAugmentWide' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_POLICY
    op = cls()
    assert op.num_magnitude_bins == 31 and op.interpolation == 'nearest' and op.table.shape == (14, 31)
    assert cls(2, 'bilinear', 7).num_magnitude_bins == 2 and cls(256).table.shape == (14, 256)
    for bad in (1, 257, 0, -3, 31.0, None, True, 'x'):
        with pytest.raises(ValueError, match='TrivialAugmentWide'):
            cls(bad)
    for bad in ('cubic', None, 1):
        with pytest.raises(ValueError, match='TrivialAugmentWide'):
            cls(interpolation=bad)
    for bad in ('x', (1, 2), float('nan'), None):
        with pytest.raises(ValueError, match='TrivialAugmentWide'):
            cls(fill=bad)


def test_state_is_out_of_place_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import TrivialAugmentWide
    op = TrivialAugmentWide()
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
    assert isinstance(alloc, AllocationQuery) and tuple(alloc.shape) == (8, 6, 3) and st.shape == (8, 6, 3)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
    assert alloc.device == ch.device('cuda:0') and alloc.dtype == ch.uint8
    for dt, shape in ((ch.uint8, (3, 8, 6)), (np.dtype('f4'), (8, 6, 3)), (np.dtype('u1'), (32768, 6, 3))):
        with pytest.raises(TypeError, match='TrivialAugmentWide'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_value_tables():
    from ffcv_amd.transforms.auto_augment import value_table, OP_NAMES, SIGNED_OPS
    assert len(OP_NAMES) == R.NUM_OPS and tuple(SIGNED_OPS) == R.SIGNED
    t = value_table(31)
    assert t.dtype == np.float64 and np.array_equal(t.view(np.uint64), R.values(31).view(np.uint64))
    b = np.arange(31)
    assert np.array_equal(t[R.POSTERIZE], 8 - (6 * b + 15) // 30) and t[R.POSTERIZE, 0] == 8 and t[R.POSTERIZE, 30] == 2
    assert sorted(set(t[R.POSTERIZE])) == [2, 3, 4, 5, 6, 7, 8]
    assert np.array_equal(t[R.SOLARIZE], 255 - (17 * b) // 2) and t[R.SOLARIZE, 0] == 255 and t[R.SOLARIZE, 30] == 0
    assert np.array_equal(t[R.TRANSLATE_X], (32 * b) // 30) and np.array_equal(t[R.TRANSLATE_X], t[R.TRANSLATE_Y])
    assert t[R.ROTATE, 30] == 135 and t[R.BRIGHTNESS, 30] == 0.99 and t[R.SHARPNESS, 15] == 0.99 * (15 / 30)
    assert abs(t[R.SHEAR_X, 30] - np.degrees(np.arctan(0.99))) < 1e-12 and np.array_equal(t[R.SHEAR_X], t[R.SHEAR_Y])
    assert not t[[R.IDENTITY, R.AUTOCONTRAST, R.EQUALIZE]].any() and (t >= 0).all()
    for nbins in (2, 3, 10, 256):
        t = value_table(nbins)
        assert np.array_equal(t.view(np.uint64), R.values(nbins).view(np.uint64))
        assert t[R.POSTERIZE, 0] == 8 and t[R.POSTERIZE, -1] == 2 and t[R.SOLARIZE, 0] == 255
        assert t[R.SOLARIZE, -1] == 0 and t[R.TRANSLATE_X, -1] == 32
        m = np.arange(nbins) / (nbins - 1)
        assert np.array_equal(t[R.POSTERIZE], 8 - np.floor(6 * m + 0.5))
        assert (np.diff(t[R.POSTERIZE]) <= 0).all() and (np.diff(t[R.SOLARIZE]) < 0).all()


@pytest.mark.parametrize('nbins,hw', ((31, (32, 32)), (10, (33, 47))))
def test_host_draws_match_numpy(hip_lib, nbins, hw):
    """ids 0 .. 2047 in two epochs, every output array; every operation and
    both signs occur."""
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import value_table
    H, W = hw
    table = value_table(nbins)
    ids = np.arange(2048, dtype=np.uint64)
    coefs = {}
    for epoch in (0, 1):
        d = L.policy_draw_batch_host(ids, SEED, epoch, nbins, table, H, W)
        assert [d[name].dtype for name, _, _ in L.POLICY_ARRAYS] == [np.dtype(dt) for _, dt, _ in L.POLICY_ARRAYS]
        seen = set()
        for k in range(2048):
            op, b, neg = R.draw(SEED, epoch, k, nbins)
            seen.add((op, neg))
            sv = R.signed_value(table, op, b, neg)
            assert d['op'][k] == op, (epoch, k)
            cj = {R.BRIGHTNESS: 0, R.COLOR: 1, R.CONTRAST: 2, R.SOLARIZE: 3}.get(op, -1)
            assert list(d['cj_apply'][:, k]) == [int(i == cj) for i in range(4)]
            want = [np.float64(1.0) + sv if i == cj else 1.0 for i in range(3)] + [sv if cj == 3 else 256.0]
            assert np.array_equal(d['cj_ratio'][:, k].view(np.uint64), np.array(want, np.float64).view(np.uint64))
            tone = {R.POSTERIZE: 0, R.AUTOCONTRAST: 1, R.EQUALIZE: 2}.get(op, -1)
            assert list(d['tone_apply'][:, k]) == [int(i == tone) for i in range(3)]
            assert d['tone_bits'][k] == (R.posterize_bits(b, nbins) if op == R.POSTERIZE else 8)
            geo = R.SHEAR_X <= op <= R.ROTATE
            assert d['aff_apply'][k] == geo
            key = (op, b, neg) if geo else None
            if key not in coefs:
                m = AR.matrix_f64(H=H, W=W, **(R.affine_args(op, sv) if geo else dict(angle=0, tx=0, ty=0, s=1,
                                                                                         shx=0, shy=0)))
                assert AR.guard_holds(m), key
                coefs[key] = AR.quantise(m)
            assert np.array_equal(d['aff_coef'][k], coefs[key]), (epoch, k, key)
            assert d['sharp_apply'][k] == (1 if op == R.SHARPNESS else 2)
            f = np.float32(np.float64(1.0) + sv) if op == R.SHARPNESS else np.float32(1)
            assert d['sharp_factor'][k].view(np.uint32) == f.view(np.uint32)
        assert seen == {(op, neg) for op in range(R.NUM_OPS) for neg in (False, True)}, epoch
    assert np.array_equal(coefs[None], AR.IDENTITY)


def test_draw_entry_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import value_table
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    ids = np.arange(2, dtype=np.uint64)
    table = value_table(31)
    out = [np.full(shape(2), 9, dt) for _, dt, shape in L.POLICY_ARRAYS]

    def call(nbins=31, h=32, w=32, batch=2, ids_p=ptr(ids), table_p=ptr(table), drop=None, entry='host'):
        outs = [None if i == drop else ptr(a) for i, a in enumerate(out)]
        if entry == 'host':
            return lib.ffcv_policy_draw_batch_host(ids_p, batch, 0, 0, nbins, table_p, h, w, *outs)
        return lib.ffcv_policy_draw_batch(None, ids_p, batch, 0, 0, nbins, table_p, h, w, *outs, None)
    for entry, name in (('host', b'ffcv_policy_draw_batch_host'), ('device', b'ffcv_policy_draw_batch')):
        for kw in [dict(nbins=1), dict(nbins=257), dict(h=0), dict(w=-1), dict(h=32768), dict(w=32768), dict(batch=-1),
                   dict(ids_p=None), dict(table_p=None)] + [dict(drop=i) for i in range(len(out))]:
            assert call(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
    assert all((a == 9).all() for a in out)
    assert call() == 0 and call(batch=0) == 0 and call(h=32767, w=1) == 0
    with pytest.raises(TypeError):
        L.policy_draw_batch_host(ids, 0, 0, 31, table[:, :30], 32, 32)


def test_tone_bits_twin_equals_single_bits_calls(hip_lib):
    """[posterize, autocontrast, equalize] with per-sample bits 1 .. 8 against
    the statement and against one ffcv_tone_batch_host call per bits value."""
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(3)
    steps = (TR.POSTERIZE, TR.AUTOCONTRAST, TR.EQUALIZE)
    for h, w in ((32, 32), (7, 5), (80, 80)):
        B = 16
        imgs = np.stack([TR.family(rng, TR.FAMILIES[k % 5], h, w) for k in range(B)])
        bits = (np.arange(B) % 8 + 1).astype(np.uint8)
        for apply in (np.tile([[1], [0], [0]], (1, B)), rng.integers(0, 2, (3, B))):
            apply = apply.astype(np.uint8)
            got = imgs.copy()
            L.tone_batch_bits_host(got, steps, apply, bits)
            want = imgs.copy()
            for v in range(1, 9):          # one single-bits call per value, on the images that carry it
                sel = np.flatnonzero(bits == v)
                part = np.ascontiguousarray(imgs[sel])
                L.tone_batch_host(part, steps, v, np.ascontiguousarray(apply[:, sel]))
                want[sel] = part
                assert np.array_equal(part, np.stack([TR.apply_program_batch(imgs[k:k + 1], steps, v,
                                                                             apply[:, k:k + 1])[0] for k in sel]))
            assert np.array_equal(got, want), (h, w)
            assert not np.array_equal(got, imgs)
    # bits is read only with a posterize step, and checked before any image is touched
    imgs = rng.integers(0, 256, (2, 4, 4, 3), dtype=np.uint8)
    keep = imgs.copy()
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    for bad in (0, 9, 255):
        with pytest.raises(L.FFCVError, match='ffcv_tone_batch_bits_host'):
            L.tone_batch_bits_host(imgs, steps, np.ones((3, 2), np.uint8), np.array([8, bad], np.uint8))
        assert np.array_equal(imgs, keep)
    L.tone_batch_bits_host(imgs, (TR.AUTOCONTRAST,), np.zeros((1, 2), np.uint8), np.array([0, 9], np.uint8))
    params = L.tone_params(steps, 8)
    ones = np.ones((3, 2), np.uint8)
    # NULL bits: params->bits
    assert lib.ffcv_tone_batch_bits_host(ptr(imgs), 2, 4, 4, ctypes.byref(params), ptr(ones), None) == 0
    assert np.array_equal(imgs, TR.apply_program_batch(keep, steps, 8, ones))
    assert lib.ffcv_tone_batch_bits(None, None, 2, 4, 4, ctypes.byref(params), ptr(ones), None, 0, None) == -1
    assert b'ffcv_tone_batch_bits' in lib.ffcv_last_error()


def test_cpu_loader_every_operation_matches_its_sibling(tmp_path, hip_lib):
    """[decoder, TrivialAugmentWide()] on a CPU Loader: every sample equals
    the sibling operation's numpy statement at the drawn value; 192 samples in
    two epochs cover all 14 operations."""
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, TrivialAugmentWide
    n = 96
    ds = NaturalDS(n, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'taw.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    table = R.values(31)
    seen = set()
    for mode, fill in (('nearest', (0, 0, 0)), ('bilinear', (9, 200, 31))):
        loader = Loader(fn, batch_size=16, device='cpu', seed=SEED, pipelines={
            'image': [SimpleRGBImageDecoder(), TrivialAugmentWide(interpolation=mode, fill=fill), ToTensor()]})
        for epoch in range(2):
            got = np.concatenate([im.numpy().copy() for im, _ in loader])     # the Loader reuses its buffers
            assert got.shape == (n, 32, 32, 3) and got.dtype == np.uint8
            for sid in range(n):
                op, b, neg = R.draw(SEED, epoch, sid)
                want = R.expected(ds.imgs[sid], op, b, neg, table, AR.NEAREST if mode == 'nearest' else AR.BILINEAR,
                                  fill)
                assert np.array_equal(got[sid], want), (mode, epoch, sid, op, b, neg)
                if mode == 'nearest':
                    seen.add(op)
        if mode == 'nearest':
            assert seen == set(range(R.NUM_OPS))


def test_graph_keeps_launch_groups(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, TrivialAugmentWide
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    ops = [SimpleRGBImageDecoder(), TrivialAugmentWide(), RandomHorizontalFlip(), ToTensor(),
           ToDevice(ch.device('cuda:0'), non_blocking=True)]
    r = Reader(raw)
    g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
              r.metadata, OSCacheManager(r).compile_reader(), device='cuda:0')
    g.collect_requirements()
    assert g.groupable()
    assert not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes)
    assert not ops[1]._absorbed
