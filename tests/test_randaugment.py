"""RandAugment on the host (no GPU): the constructor's checks and the public
name, the value table against the numpy statement (tests/randaugment_ref.py)
and against values worked out by hand, the host twin of the draws against the
statement in every output array, a CPU Loader against the statement per
sample, and the C entries' argument checks."""
import ctypes

import numpy as np
import pytest

from tests import affine_ref as AR
from tests import auto_augment_ref as R
from tests import randaugment_ref as RA
from tests.helpers import NaturalDS, write

SEED = 29      # loader seed of the draw and Loader tests: ids 0 .. 2047 draw all 196 ordered pairs at num_ops = 2


def test_public_name_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls = T.RandAugment
    assert FT.RandAugment is cls and 'RandAugment' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == RA.OP_RANDAUGMENT
    op = cls()
    assert (op.num_ops, op.magnitude, op.num_magnitude_bins, op.interpolation) == (2, 9, 31, 'nearest')
    assert list(op.fill) == [0, 0, 0]
    op = cls(8, 1, 2, 'bilinear', 7)
    assert (op.num_ops, op.magnitude, op.num_magnitude_bins, op.interpolation) == (8, 1, 2, 'bilinear')
    assert cls(1, 255, 256).magnitude == 255 and cls(magnitude=0).magnitude == 0
    for bad in (0, 9, -1, 2.0, None, True, 'x'):
        with pytest.raises(ValueError, match='RandAugment: num_ops'):
            cls(num_ops=bad)
    for bad in (1, 257, 0, -3, 31.0, None, True, 'x'):
        with pytest.raises(ValueError, match='RandAugment: num_magnitude_bins'):
            cls(num_magnitude_bins=bad)
    for bad in (-1, 31, 9.0, None, True, False, 'x'):
        with pytest.raises(ValueError, match='RandAugment: magnitude'):
            cls(magnitude=bad)
    with pytest.raises(ValueError, match='RandAugment: magnitude'):
        cls(magnitude=10, num_magnitude_bins=10)
    for bad in ('cubic', None, 1):
        with pytest.raises(ValueError, match='RandAugment: interpolation'):
            cls(interpolation=bad)
    for bad in ('x', (1, 2), float('nan'), None):
        with pytest.raises(ValueError, match='RandAugment: fill'):
            cls(fill=bad)


def test_state_is_out_of_place_uint8_hwc_and_builds_the_table():
    import torch as ch
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandAugment
    op = RandAugment()
    assert op.table is None
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
    assert isinstance(alloc, AllocationQuery) and tuple(alloc.shape) == (8, 6, 3) and st.shape == (8, 6, 3)
    assert np.array_equal(op.table, RA.values(31, 8, 6)) and op.table_for(8, 6) is op.table
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
    assert alloc.device == ch.device('cuda:0') and alloc.dtype == ch.uint8
    for dt, shape in ((ch.uint8, (3, 8, 6)), (np.dtype('f4'), (8, 6, 3)), (np.dtype('u1'), (32768, 6, 3))):
        with pytest.raises(TypeError, match='RandAugment'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


def test_value_tables():
    from ffcv_amd.transforms.auto_augment import randaugment_table, OP_NAMES, SIGNED_OPS
    assert len(OP_NAMES) == RA.NUM_OPS and tuple(SIGNED_OPS) == R.SIGNED
    for nbins in (2, 10, 31, 256):
        for H, W in ((32, 32), (33, 47), (1, 1), (224, 160), (64, 65)):
            t = randaugment_table(nbins, H, W)
            assert t.dtype == np.float64 and t.shape == (14, nbins)
            assert np.array_equal(t.view(np.uint64), RA.values(nbins, H, W).view(np.uint64)), (nbins, H, W)
            m = np.arange(nbins) / (nbins - 1)
            assert np.array_equal(t[R.POSTERIZE], 8 - np.floor(4 * m + 0.5))          # round half up
            assert t[R.POSTERIZE, 0] == 8 and t[R.POSTERIZE, -1] == 4
            assert t[R.SOLARIZE, 0] == 255 and t[R.SOLARIZE, -1] == 0 and (np.diff(t[R.SOLARIZE]) < 0).all()
            assert t[R.TRANSLATE_X, -1] == (150 * W) // 331 and t[R.TRANSLATE_Y, -1] == (150 * H) // 331
            assert t[R.ROTATE, -1] == 30 and t[R.BRIGHTNESS, -1] == 0.9 and np.array_equal(t[R.SHEAR_X], t[R.SHEAR_Y])
            assert abs(t[R.SHEAR_X, -1] - np.degrees(np.arctan(0.3))) < 1e-12
            assert np.array_equal(t[R.BRIGHTNESS], t[R.SHARPNESS]) and np.array_equal(t[R.COLOR], t[R.CONTRAST])
            assert not t[[R.IDENTITY, R.AUTOCONTRAST, R.EQUALIZE]].any() and (t >= 0).all()
    # the default bin, by hand: 32 x 32, bin 9 of 31
    t = randaugment_table(31, 32, 32)
    assert t[R.TRANSLATE_X, 9] == 4 and t[R.TRANSLATE_Y, 9] == 4        # 150 * 32 * 9 = 43200; // (331 * 30 = 9930) = 4
    assert t[R.POSTERIZE, 9] == 7                                       # 8 - (72 + 30) // 60 = 8 - 1
    assert t[R.SOLARIZE, 9] == 179                                      # 255 - 2295 // 30 = 255 - 76
    assert abs(t[R.ROTATE, 9] - 9.0) < 1e-12                            # 30 * 0.3
    assert abs(t[R.BRIGHTNESS, 9] - 0.27) < 1e-12
    assert abs(t[R.SHEAR_X, 9] - np.degrees(np.arctan(0.09))) < 1e-12
    # a posterize tie: 4 m = 0.5 at bin 1 of 9 rounds up, to 7 bits (half-to-even would keep 8)
    assert randaugment_table(9, 8, 8)[R.POSTERIZE, 1] == 7


def _check_draws(d, seed, epoch, num_ops, nbins, mag, table, H, W, coefs, pairs):
    n = d['op'].shape[1]
    for k in range(n):
        slots = RA.draw(seed, epoch, k, num_ops)
        if num_ops == 2:
            pairs.add((slots[0][0], slots[1][0]))
        for s, (op, neg) in enumerate(slots):
            sv = R.signed_value(table, op, mag, neg)
            at = (seed, epoch, num_ops, k, s)
            assert d['op'][s, k] == op, at
            cj = {R.BRIGHTNESS: 0, R.COLOR: 1, R.CONTRAST: 2, R.SOLARIZE: 3}.get(op, -1)
            assert list(d['cj_apply'][s, :, k]) == [int(i == cj) for i in range(4)], at
            want = [np.float64(1.0) + sv if i == cj else 1.0 for i in range(3)] + [sv if cj == 3 else 256.0]
            want = np.array(want, np.float64)
            assert np.array_equal(d['cj_ratio'][s, :, k].view(np.uint64), want.view(np.uint64)), at
            tone = {R.POSTERIZE: 0, R.AUTOCONTRAST: 1, R.EQUALIZE: 2}.get(op, -1)
            assert list(d['tone_apply'][s, :, k]) == [int(i == tone) for i in range(3)], at
            assert d['tone_bits'][s, k] == (RA.posterize_bits(mag, nbins) if op == R.POSTERIZE else 8), at
            geo = R.SHEAR_X <= op <= R.ROTATE
            assert d['aff_apply'][s, k] == geo, at
            key = (op, neg, H, W, mag, nbins) if geo else None
            if key not in coefs:
                m = AR.matrix_f64(H=H, W=W, **(R.affine_args(op, sv) if geo else dict(angle=0, tx=0, ty=0, s=1,
                                                                                     shx=0, shy=0)))
                assert AR.guard_holds(m), key
                coefs[key] = AR.quantise(m)
            assert np.array_equal(d['aff_coef'][s, k], coefs[key]), at
            assert d['sharp_apply'][s, k] == (1 if op == R.SHARPNESS else 2), at
            f = np.float32(np.float64(1.0) + sv) if op == R.SHARPNESS else np.float32(1)
            assert d['sharp_factor'][s, k].view(np.uint32) == f.view(np.uint32), at


@pytest.mark.parametrize('num_ops', (1, 2, 3))
def test_host_draws_match_numpy(hip_lib, num_ops):
    """ids 0 .. 2047 at two (seed, epoch) pairs, every output array; at
    num_ops = 2 all 196 ordered pairs of operations occur under SEED."""
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import randaugment_table
    ids = np.arange(2048, dtype=np.uint64)
    coefs = {}
    for (seed, epoch), (nbins, mag, (H, W)) in (((SEED, 0), (31, 9, (32, 32))), ((2 ** 63 + 5, 7), (10, 7, (33, 47)))):
        table = randaugment_table(nbins, H, W)
        d = L.randaugment_draw_batch_host(ids, seed, epoch, num_ops, nbins, mag, table, H, W)
        arrays = L.randaugment_arrays(num_ops)
        assert [d[name].dtype for name, _, _ in arrays] == [np.dtype(dt) for _, dt, _ in arrays]
        assert [d[name].shape for name, _, _ in arrays] == [shape(2048) for _, _, shape in arrays]
        assert [shape(5) for _, _, shape in arrays] == [(num_ops,) + shape(5) for _, _, shape in L.POLICY_ARRAYS]
        pairs = set()
        _check_draws(d, seed, epoch, num_ops, nbins, mag, table, H, W, coefs, pairs)
        if num_ops == 2 and seed == SEED:
            assert len(pairs) == 196
        # a slot's slices are the policy draw's layout: contiguous, the pixel entries' arguments
        for s in range(num_ops):
            a = L.randaugment_slot(d, s)
            assert all(a[name].flags.c_contiguous and a[name].shape == shape(2048)
                       for name, _, shape in L.POLICY_ARRAYS)
    assert np.array_equal(coefs[None], AR.IDENTITY)
    # the stream of slot s does not depend on num_ops
    if num_ops == 3:
        table = randaugment_table(31, 32, 32)
        d3 = L.randaugment_draw_batch_host(ids[:64], SEED, 0, 3, 31, 9, table, 32, 32)
        d1 = L.randaugment_draw_batch_host(ids[:64], SEED, 0, 1, 31, 9, table, 32, 32)
        assert all(np.array_equal(d3[name][0], d1[name][0]) for name, _, _ in L.POLICY_ARRAYS)


def test_entries_reject_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import randaugment_table
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    ids = np.arange(2, dtype=np.uint64)
    table = randaugment_table(31, 32, 32)
    out = [np.full(shape(2), 9, dt) for _, dt, shape in L.randaugment_arrays(8)]

    def draw(num_ops=2, nbins=31, mag=9, h=32, w=32, batch=2, ids_p=ptr(ids), table_p=ptr(table), drop=None,
             entry='host'):
        outs = [None if i == drop else ptr(a) for i, a in enumerate(out)]
        if entry == 'host':
            return lib.ffcv_randaugment_draw_batch_host(ids_p, batch, 0, 0, num_ops, nbins, mag, table_p, h, w, *outs)
        return lib.ffcv_randaugment_draw_batch(None, ids_p, batch, 0, 0, num_ops, nbins, mag, table_p, h, w, *outs,
                                               None)
    for entry, name in (('host', b'ffcv_randaugment_draw_batch_host'), ('device', b'ffcv_randaugment_draw_batch')):
        for kw in [dict(num_ops=0), dict(num_ops=9), dict(num_ops=-1), dict(nbins=1), dict(nbins=257), dict(mag=-1),
                   dict(mag=31), dict(nbins=10, mag=10), dict(h=0), dict(w=-1), dict(h=32768), dict(w=32768),
                   dict(batch=-1), dict(ids_p=None), dict(table_p=None)] + [dict(drop=i) for i in range(len(out))]:
            assert draw(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
    assert all((a == 9).all() for a in out)
    assert draw() == 0 and draw(batch=0) == 0 and draw(h=32767, w=1) == 0 and draw(num_ops=8, mag=30) == 0
    assert draw(num_ops=1, nbins=2, mag=1) == 0 and draw(entry='device', batch=0) == 0
    with pytest.raises(TypeError):
        L.randaugment_draw_batch_host(ids, 0, 0, 2, 31, 9, table[:, :30], 32, 32)

    # the fused pixel entry: everything is refused before any launch
    assert L.randaugment_lds_bytes() == L.sharpness_lds_bytes()            # the whole-image regime of sharpness
    img = np.zeros((2, 8, 8, 3), np.uint8)
    dst = np.zeros_like(img)
    fill = np.zeros(3, np.uint8)
    d = [np.zeros(shape(2), dt) for _, dt, shape in L.randaugment_arrays(2)]

    def pix(src_p=ptr(img), dst_p=ptr(dst), batch=2, h=8, w=8, num_ops=2, mode=1, fill_p=ptr(fill), drop=None):
        arrs = [None if i == drop else ptr(a) for i, a in enumerate(d)]
        return lib.ffcv_randaugment_batch(None, src_p, dst_p, batch, h, w, num_ops, mode, fill_p, *arrs)
    edge = L.randaugment_lds_bytes() // 6
    for kw in [dict(src_p=None), dict(dst_p=None), dict(fill_p=None), dict(batch=-1), dict(h=0), dict(w=0),
               dict(num_ops=0), dict(num_ops=9), dict(mode=2), dict(mode=-1), dict(dst_p=ptr(img)),
               dict(dst_p=ctypes.c_void_p(img.ctypes.data + 8 * 8 * 3)), dict(h=1, w=edge + 1), dict(h=64, w=65),
               dict(h=32768, w=1)] + [dict(drop=i) for i in range(len(d))]:
        assert pix(**kw) == -1, kw
        assert b'ffcv_randaugment_batch' in lib.ffcv_last_error()
    assert pix(batch=0) == 0 and pix(batch=0, h=64, w=64) == 0 and pix(batch=0, h=1, w=edge) == 0
    assert not dst.any()


@pytest.mark.parametrize('mode,fill', (('nearest', (0, 0, 0)), ('bilinear', (9, 200, 31))))
def test_cpu_loader_matches_the_statement(tmp_path, hip_lib, mode, fill):
    """[decoder, RandAugment(num_ops=2)] on a CPU Loader: every sample equals
    the two sibling operations' numpy statements in sequence, every byte."""
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandAugment
    n = 224
    ds = NaturalDS(n, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'ra.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    table = RA.values(31, 32, 32)
    loader = Loader(fn, batch_size=32, device='cpu', seed=SEED, pipelines={
        'image': [SimpleRGBImageDecoder(), RandAugment(interpolation=mode, fill=fill), ToTensor()]})
    seen, changed = set(), 0
    for epoch in range(2):
        got = np.concatenate([im.numpy().copy() for im, _ in loader])     # the Loader reuses its buffers
        assert got.shape == (n, 32, 32, 3) and got.dtype == np.uint8
        for sid in range(n):
            slots = RA.draw(SEED, epoch, sid, 2)
            ops, negs = [s[0] for s in slots], [s[1] for s in slots]
            want = RA.expected(ds.imgs[sid], ops, negs, 9, table, AR.NEAREST if mode == 'nearest' else AR.BILINEAR,
                               fill)
            assert np.array_equal(got[sid], want), (mode, epoch, sid, slots)
            seen.update(ops)
            changed += not np.array_equal(got[sid], ds.imgs[sid])
    assert seen == set(range(RA.NUM_OPS)) and changed > n


def test_cpu_loader_three_operations_beyond_the_fused_regime(tmp_path, hip_lib):
    """num_ops = 3 on 40 x 72 images (the host path is rounds at every size)."""
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandAugment
    n = 48
    ds = NaturalDS(n, hw=(40, 72), seed=6)
    fn = write(str(tmp_path / 'ra3.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    table = RA.values(12, 40, 72)
    loader = Loader(fn, batch_size=16, device='cpu', seed=SEED, pipelines={
        'image': [SimpleRGBImageDecoder(), RandAugment(3, 11, 12, 'bilinear', 77), ToTensor()]})
    got = np.concatenate([im.numpy().copy() for im, _ in loader])
    for sid in range(n):
        slots = RA.draw(SEED, 0, sid, 3)
        want = RA.expected(ds.imgs[sid], [s[0] for s in slots], [s[1] for s in slots], 11, table, AR.BILINEAR,
                           (77, 77, 77))
        assert np.array_equal(got[sid], want), (sid, slots)


def test_graph_keeps_launch_groups(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, RandAugment
    raw = write(str(tmp_path / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    ops = [SimpleRGBImageDecoder(), RandAugment(), RandomHorizontalFlip(), ToTensor(),
           ToDevice(ch.device('cuda:0'), non_blocking=True)]
    r = Reader(raw)
    g = Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1},
              r.metadata, OSCacheManager(r).compile_reader(), device='cuda:0')
    g.collect_requirements()
    assert g.groupable()
    assert not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes)
    assert not ops[1]._absorbed
