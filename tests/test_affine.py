"""RandomAffine / RandomRotation on the host (no GPU): public names and
argument checks, the consequences of the contract (tests/affine_ref.py), the
host twins of the C ABI (draws and coefficients against numpy under the
coefficient guard, pixels bit for bit with numpy's integer coefficients), the
graph lowering, and a CPU Loader.

sin, cos and tan are the functions of the contract that are not pinned bit for
bit, so every comparison of drawn coefficients first asserts, on numpy's
float64 matrix, that no coefficient lies within 2^-20 of a rounding boundary
after the scaling by 65536 (affine_ref.guard_holds), for every sample, and then
demands equal integers."""
import ctypes

import numpy as np
import pytest

from tests import affine_ref as R
from tests.helpers import NaturalDS, write
from tests.test_blur import make_inputs, mixed_apply

SEED = 7     # with this loader seed the guard holds for CONFIGS x GUARD_SHAPES (ids 0 .. 255, epoch 0)
MODES = (R.BILINEAR, R.NEAREST)
WHOLE = 16384                               # asserted against the library in the GPU tests
# 43 x 127 is the largest whole-image shape (3 H W = 16,383), 43 x 128 the first beyond it
SHAPES = ((1, 1), (1, 7), (7, 1), (32, 32), (43, 127), (43, 128), (97, 131), (64, 224))
FILL = (7, 130, 251)


def coef_sets(H, W):
    """name -> six int64 coefficients for H x W images."""
    c = lambda *a, **kw: R.coefficients(*a, H=H, W=W, **kw)  # noqa: E731
    return {
        'identity': np.array(R.IDENTITY, np.int64),
        'rot90': c(90), 'rot180': c(180),
        'rot33.7_shear': c(33.7, shx=12.0, shy=-7.0),
        # minification by 4: footprints of 4 x the tile, clipped to a few columns where a tile meets the image's edge
        'scale_quarter': c(0, s=0.25, tx=12),
        'scale4': c(0, s=4.0),
        'far': c(0, tx=W + 5),                    # a translation larger than the image: all fill
        'zero_m': np.array([0, 0, (((W - 1) // 2) << 16) + 0x4321, 0, 0, (((H - 1) // 2) << 16) + 0x9ABC], np.int64),
        'frac255': np.array([65536, 0, 0xFFFF, 0, 65536, 0xFF00], np.int64),   # fx = fy = 255 everywhere
        'frac0_shift': np.array([65536, 0, -65536, 0, 65536, 65536], np.int64),  # fx = fy = 0, a whole-pixel shift
        'm_beyond': np.array([R.M_MAX + 1, 0, 0, 0, 65536, 0], np.int64),
        'b_beyond': np.array([65536, 0, 0, 0, 65536, -R.B_MAX - 1], np.int64),
        'm_at_bound': np.array([R.M_MAX, -R.M_MAX, R.B_MAX, -R.M_MAX, R.M_MAX, -R.B_MAX], np.int64),
    }


def test_public_names_and_arguments():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls, rot = T.RandomAffine, T.RandomRotation
    assert FT.RandomAffine is cls and FT.RandomRotation is rot
    assert 'RandomAffine' in T.__all__ and 'RandomRotation' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_AFFINE and rot.op_id == R.OP_AFFINE
    op = cls(30)
    assert op.degrees == (-30.0, 30.0) and op.translate == (0.0, 0.0) and op.scale == (1.0, 1.0)
    assert op.shear == (0.0, 0.0, 0.0, 0.0) and op.interpolation == 'bilinear' and op.p == 1.0
    assert (op.fill_u8() == 0).all()
    assert cls((-10, 45)).degrees == (-10.0, 45.0) and cls(0, shear=15).shear == (-15.0, 15.0, 0.0, 0.0)
    assert cls(0, shear=(-5, 8)).shear == (-5.0, 8.0, 0.0, 0.0) and cls(0, shear=(1, 2, 3, 4)).shear == (1, 2, 3, 4)
    assert (cls(0, fill=300).fill_u8() == 44).all() and list(cls(0, fill=(1, 2, 3)).fill_u8()) == [1, 2, 3]
    assert cls(360, (1, 1), (1 / 16, 16), 60, 'nearest', p=0).interpolation == 'nearest'
    for bad in (-1, 361, float('nan'), float('inf'), (10, -10), (-400, 0), (1, 2, 3), 'x', None, True):
        with pytest.raises(ValueError, match='RandomAffine: degrees'):
            cls(bad)
        with pytest.raises(ValueError, match='RandomRotation: degrees'):
            rot(bad)
    for bad in ((-0.1, 0), (0, 1.5), 0.5, (0.1,), (float('nan'), 0), None):
        with pytest.raises(ValueError, match='translate'):
            cls(0, translate=bad)
    for bad in ((0.01, 1), (1, 17), (2, 1), 1.0, (1, float('inf')), None):
        with pytest.raises(ValueError, match='scale'):
            cls(0, scale=bad)
    for bad in (-1, 61, (10, -10), (0, 0, 61, 62), (1, 2, 3), float('nan'), (0, float('inf')), None):
        with pytest.raises(ValueError, match='shear'):
            cls(0, shear=bad)
    for bad in ('bicubic', 0, None):
        with pytest.raises(ValueError, match='interpolation'):
            cls(0, interpolation=bad)
    for bad in ((1, 2), 'red', None, (0, 0, float('nan'))):
        with pytest.raises(ValueError, match='fill'):
            cls(0, fill=bad)
    for bad in (-0.01, 1.01, float('nan'), None):
        with pytest.raises(ValueError, match='p must'):
            cls(0, p=bad)


def test_rotation_is_affine_with_degenerate_ranges():
    from ffcv_amd.transforms import RandomAffine, RandomRotation
    a, r = RandomAffine((-20, 75), interpolation='nearest', fill=9, p=0.3), \
        RandomRotation((-20, 75), interpolation='nearest', fill=9, p=0.3)
    assert isinstance(r, RandomAffine)
    for attr in ('degrees', 'translate', 'scale', 'shear', 'interpolation', 'p', 'op_id'):
        assert getattr(a, attr) == getattr(r, attr)
    assert a.ranges(33, 71) == r.ranges(33, 71) == R.ranges(33, 71, (-20, 75))
    assert (a.fill_u8() == r.fill_u8()).all()


def test_state_must_be_uint8_hwc():
    import torch as ch
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomAffine, RandomRotation
    for op, name in ((RandomAffine(10), 'RandomAffine'), (RandomRotation(10), 'RandomRotation')):
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
        assert isinstance(alloc, AllocationQuery) and tuple(alloc.shape) == (8, 6, 3) and st.shape == (8, 6, 3)
        assert st.dtype == np.dtype('u1') and st.jit_mode
        st, alloc = op.declare_state_and_memory(
            State(jit_mode=False, device=ch.device('cuda:0'), dtype=ch.uint8, shape=(8, 6, 3)))
        assert alloc.device == ch.device('cuda:0') and alloc.dtype == ch.uint8 and not st.jit_mode
        for dt, shape in ((ch.uint8, (3, 8, 6)), (ch.float16, (8, 6, 3)), (np.dtype('f4'), (8, 6, 3)),
                          (np.dtype('u1'), (8, 6)), (np.dtype('u1'), (8, 6, 4)), (np.dtype('u1'), (40000, 6, 3))):
            with pytest.raises(TypeError, match=name):
                op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


# ------------------------------------------- consequences of the contract --
def _img(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize('mode', MODES)
def test_consequences_in_the_reference(mode):
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (5, 8), (32, 32), (33, 31)):
        img = _img(rng, H, W)
        q = R.coefficients(0, H=H, W=W)
        assert tuple(q) == R.IDENTITY and np.array_equal(R.warp(img, q, mode, FILL), img)
        assert np.array_equal(R.warp(img, R.coefficients(180, H=H, W=W), mode, FILL), img[::-1, ::-1])
    for n in (7, 8, 31, 32):                  # odd and even side: clockwise on screen
        img = _img(rng, n, n)
        q = R.coefficients(90, H=n, W=n)
        assert q[0] == 0 and q[4] == 0        # cos 90 degrees is 6e-17 in float64 and quantises to 0
        assert np.array_equal(R.warp(img, q, mode, FILL), np.rot90(img, 3))
    from ffcv_amd.transforms.translate import translate_window
    img = _img(rng, 9, 13)
    for tx, ty in ((0, 0), (3, -2), (-5, 4), (12, 0), (0, -8), (13, 9), (-40, 2)):
        q = R.coefficients(0, tx=tx, ty=ty, H=9, W=13)
        pad = 64
        want = translate_window(img, np.empty_like(img), pad - ty, pad - tx, pad, np.array(FILL, np.uint8))
        assert np.array_equal(R.warp(img, q, mode, FILL), want), (tx, ty)


def test_reference_bounds_and_weights():
    rng = np.random.default_rng(6)
    img = _img(rng, 12, 17)
    sets = coef_sets(12, 17)
    for name in ('m_beyond', 'b_beyond', 'far'):
        for mode in MODES:
            assert (R.warp(img, sets[name], mode, FILL) == np.array(FILL, np.uint8)).all(), name
    assert R.coef_ok(sets['m_at_bound']) and not R.coef_ok(sets['m_beyond'])
    # constructor limits keep the coefficients inside the bounds: the extremes of every range
    worst_m = worst_b = 0
    for angle in (-360, -225, -135, -45, 0, 45, 135, 225, 360):
        for shx in (-60, 60):
            for shy in (-60, 60):
                m = R.matrix_f64(angle, 32767, -32767, 1 / 16, shx, shy, 32767, 32767) * 65536
                worst_m = max(worst_m, np.abs(m[[0, 1, 3, 4]]).max())
                worst_b = max(worst_b, np.abs(m[[2, 5]]).max())
    assert worst_m <= R.M_MAX and worst_b <= R.B_MAX
    # frac255: out = (1 * tl + 255 * tr, ...) weights; frac0_shift: a copy shifted by whole pixels
    want = np.full_like(img, 0)
    want[:] = np.array(FILL, np.uint8)
    want[:-1, 1:] = img[1:, :-1]
    assert np.array_equal(R.warp(img, sets['frac0_shift'], R.BILINEAR, FILL), want)
    white = np.full((12, 17, 3), 255, np.uint8)
    q = sets['rot33.7_shear']
    assert (R.warp(white, q, R.BILINEAR, (255, 255, 255)) == 255).all()      # the weights sum to 65536
    out = R.warp(white, q, R.BILINEAR, (0, 0, 0))
    r, c = np.meshgrid(np.arange(12), np.arange(17), indexing='ij')
    ix, iy = (q[0] * c + q[1] * r + q[2]) >> 16, (q[3] * c + q[4] * r + q[5]) >> 16
    inside = (ix >= 0) & (ix + 1 < 17) & (iy >= 0) & (iy + 1 < 12)
    assert inside.sum() > 20 and (out[inside] == 255).all() and (out[~inside] < 255).any()


# ----------------------------------------------------------- host twins --
@pytest.mark.parametrize('config', range(3))
def test_draw_twin_matches_numpy_under_the_guard(hip_lib, config):
    from ffcv_amd import libffcv as L
    cfg = R.CONFIGS[config]
    ids = np.arange(256, dtype=np.uint64)
    for H, W in R.GUARD_SHAPES:
        rg = R.ranges(H, W, **cfg)
        for p in (0.5, 1.0):
            apply, coef = L.affine_draw_batch_host(ids, SEED, 0, p, rg, H, W)
            assert apply.shape == (256,) and coef.shape == (256, 6) and coef.dtype == np.int64
            for i in range(256):
                wa, m, q = R.draw_coefficients(SEED, 0, i, p, rg, H, W)
                assert R.guard_holds(m), (config, H, W, i)
                assert bool(apply[i]) == wa and np.array_equal(coef[i], q), (config, H, W, i, coef[i], q)
                assert R.coef_ok(q)
            assert apply.all() if p == 1.0 else 0 < apply.sum() < 256
        if config == 1:
            assert len({tuple(q) for q in coef}) == 256 and (coef[:, 2] != 0).any()
    # the translations are whole pixels: with no rotation, scale 1 and no shear, b is a multiple of 65536
    rg = R.ranges(97, 131, 0, translate=(0.3, 0.2))
    _, coef = L.affine_draw_batch_host(ids, SEED, 0, 1.0, rg, 97, 131)
    assert (coef[:, [0, 4]] == 65536).all() and (coef[:, [1, 3]] == 0).all() and (coef[:, [2, 5]] % 65536 == 0).all()
    assert len(set(coef[:, 2])) > 20 and np.abs(coef[:, 2]).max() <= 40 << 16


def test_draw_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    ids = np.arange(2, dtype=np.uint64)
    a, q = np.full(2, 9, np.uint8), np.full((2, 6), 9, np.int64)
    good = np.array(R.ranges(32, 32, **R.CONFIGS[0]))

    def call(rg=good, p=0.5, h=32, w=32, entry='host', n=2):
        rg = np.ascontiguousarray(rg, np.float64)
        if entry == 'host':
            return lib.ffcv_affine_draw_batch_host(ptr(ids), n, 0, 0, p, ptr(rg), h, w, ptr(a), ptr(q))
        return lib.ffcv_affine_draw_batch(None, ptr(ids), n, 0, 0, p, ptr(rg), h, w, ptr(a), ptr(q), None)

    def changed(i, v):
        rg = good.copy()
        rg[i] = v
        return rg
    for entry, name in (('host', b'ffcv_affine_draw_batch_host'), ('device', b'ffcv_affine_draw_batch')):
        for kw in (dict(p=-0.1), dict(p=1.5), dict(p=float('nan')), dict(h=0), dict(w=0), dict(h=32768), dict(w=40000),
                   dict(n=-1), dict(rg=changed(0, -361)), dict(rg=changed(1, 361)), dict(rg=changed(0, 40)),
                   dict(rg=changed(3, 33)), dict(rg=changed(4, -33)), dict(rg=changed(6, 0.01)),
                   dict(rg=changed(7, 17)), dict(rg=changed(8, -61)), dict(rg=changed(11, 61)),
                   dict(rg=changed(10, float('nan'))), dict(rg=changed(1, float('inf')))):
            assert call(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
        assert call(entry=entry, n=0) == 0
    assert lib.ffcv_affine_draw_batch_host(None, 2, 0, 0, 0.5, ptr(good), 32, 32, ptr(a), ptr(q)) == -1
    assert lib.ffcv_affine_draw_batch_host(ptr(ids), 2, 0, 0, 0.5, ptr(good), 32, 32, ptr(a), None) == -1
    assert (a == 9).all() and (q == 9).all()
    assert call() == 0 and (a <= 1).all()


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_host_twin_pixels_match_numpy(hip_lib, shape):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    imgs = make_inputs(rng, shape)
    apply = mixed_apply()
    sets = coef_sets(*shape)
    for mode in MODES:
        for name, q in sets.items():
            coef = np.stack([q] * len(imgs))
            got = np.full_like(imgs, 0x5A)
            L.affine_batch_host(imgs, got, mode, FILL, apply, coef, nthreads=3)
            want = R.warp_batch(imgs, coef, mode, apply, FILL)
            assert np.array_equal(got, want), (shape, mode, name)
            assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[4], imgs[4])
        # every image its own coefficients
        names = list(sets)
        coef = np.stack([sets[names[(3 * k + 1) % len(names)]] for k in range(len(imgs))])
        got = np.empty_like(imgs)
        L.affine_batch_host(imgs, got, mode, FILL, np.ones(len(imgs), np.uint8), coef)
        assert np.array_equal(got, R.warp_batch(imgs, coef, mode, np.ones(len(imgs)), FILL)), (shape, mode)


@pytest.mark.parametrize('mode', MODES)
def test_host_twin_consequences_and_rounding(hip_lib, mode):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(8)

    def run(img, q, fill=FILL):
        out = np.empty_like(img[None])
        L.affine_batch_host(img[None], out, mode, fill, np.ones(1, np.uint8), np.asarray(q, np.int64)[None])
        return out[0]
    for n in (7, 8):
        img = _img(rng, n, n)
        assert np.array_equal(run(img, R.IDENTITY), img)
        assert np.array_equal(run(img, R.coefficients(180, H=n, W=n)), img[::-1, ::-1])
        assert np.array_equal(run(img, R.coefficients(90, H=n, W=n)), np.rot90(img, 3))
    img = _img(rng, 12, 17)
    for name in ('m_beyond', 'b_beyond', 'far'):
        assert (run(img, coef_sets(12, 17)[name]) == np.array(FILL, np.uint8)).all()
    white = np.full((12, 17, 3), 255, np.uint8)
    assert (run(white, coef_sets(12, 17)['rot33.7_shear'], (255, 255, 255)) == 255).all()
    # the rounding of nearest at the +-32768 boundary, and bilinear's weights beside it
    row = _img(rng, 1, 4)
    fill = np.array(FILL, np.uint8)
    for q2, shift in ((32767, 0), (32768, 1), (-32768, 0), (-32769, -1), (65536 + 32767, 1), (-65536 - 32769, -2)):
        got = run(row, (65536, 0, q2, 0, 65536, 0))
        if mode == R.NEAREST:
            want = np.stack([row[0, c + shift] if 0 <= c + shift < 4 else fill for c in range(4)])[None]
            assert np.array_equal(got, want), q2
        assert np.array_equal(got, R.warp(row, (65536, 0, q2, 0, 65536, 0), mode, FILL)), q2


def test_pixel_entry_rejects_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    lib = L.lib()
    ptr = lambda x, off=0: ctypes.c_void_p(x.ctypes.data + off)  # noqa: E731
    src = np.full((2, 6, 5, 3), 77, np.uint8)
    dst = np.full((3, 6, 5, 3), 66, np.uint8)
    apply = np.ones(2, np.uint8)
    coef = np.stack([np.array(R.IDENTITY, np.int64)] * 2)
    fill = np.zeros(3, np.uint8)

    def call(s=None, d=None, h=6, wd=5, mode=0, stride=0, entry='host', n=2, f=fill):
        s = ptr(src) if s is None else s
        d = ptr(dst) if d is None else d
        f = None if f is None else ptr(f)
        if entry == 'host':
            return lib.ffcv_affine_batch_host(s, d, n, h, wd, mode, f, ptr(apply), ptr(coef), stride, 1)
        return lib.ffcv_affine_batch(None, s, d, n, h, wd, mode, f, ptr(apply), ptr(coef), stride)
    for entry, name in (('host', b'ffcv_affine_batch_host'), ('device', b'ffcv_affine_batch')):
        for kw in (dict(mode=2), dict(mode=-1), dict(h=0), dict(wd=-1), dict(wd=32768), dict(h=32768), dict(n=-1),
                   dict(h=32767, wd=32767), dict(f=None), dict(stride=89), dict(d=ptr(src)), dict(d=ptr(src, 90)),
                   dict(d=ptr(src, 179)), dict(s=ptr(dst, 90), stride=90)):
            assert call(entry=entry, **kw) == -1, kw
            assert name in lib.ffcv_last_error()
        assert b'overlap' in lib.ffcv_last_error()
        assert call(entry=entry, n=0) == 0
    assert (src == 77).all() and (dst == 66).all()
    assert call() == 0 and call(stride=135) == 0 and call(mode=1) == 0
    assert L.affine_whole_bytes() == WHOLE and min(L.affine_tile_shape()) >= 1 and L.affine_tile_lds() >= 1
    with pytest.raises(TypeError):
        L.affine_batch_host(src[:, :, :, :2], dst, 0, fill, apply, coef)


def test_tile_bytes_show_the_regimes(hip_lib):
    from ffcv_amd import libffcv as L
    th, tw = L.affine_tile_shape()
    lds = L.affine_tile_lds()
    ident = R.IDENTITY
    # whole-image regime: the image's chunks, or nothing
    assert L.affine_tile_bytes(32, 32, 0, ident, 0, 0) == ((3072 + 30) >> 4) * 16
    assert L.affine_tile_bytes(43, 127, 0, ident, 0, 0) == ((WHOLE - 1 + 30) >> 4) * 16
    assert L.affine_tile_bytes(32, 32, 0, coef_sets(32, 32)['far'], 0, 0) == 0
    assert L.affine_tile_bytes(32, 32, 0, ident, 0, 1) == 0                       # no such tile
    assert L.affine_tile_bytes(32, 32, 0, coef_sets(32, 32)['m_beyond'], 0, 0) == 0
    assert L.affine_tile_bytes(32, 32, 0, coef_sets(32, 32)['m_at_bound'], 0, 0) in (0, L.AFFINE_NOT_STAGEABLE)
    # tiles: the identity stages the tile's own pixels (and a row and column more for bilinear)
    H, W = 97, 131
    assert L.affine_tile_bytes(H, W, 1, ident, 0, 0) == th * (((3 * tw + 30) >> 4) * 16)
    assert L.affine_tile_bytes(H, W, 0, ident, 0, 0) == (th + 1) * (((3 * (tw + 1) + 30) >> 4) * 16)
    quarter = coef_sets(H, W)['scale_quarter']
    sizes = [L.affine_tile_bytes(H, W, 0, quarter, r, c) for r in range(-(-H // th)) for c in range(-(-W // tw))]
    assert any(s > lds for s in sizes) and any(0 < s <= lds for s in sizes) and any(s == 0 for s in sizes)
    assert all(L.affine_tile_bytes(H, W, 0, coef_sets(H, W)['scale4'], r, c) <= lds for r in range(3) for c in range(4))


def test_affine_ends_a_decoders_fused_prefix(tmp_path):
    """Lowering decisions on a CUDA-typed graph (no kernel launched)."""
    import torch as ch
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, RandomResizedCropRGBImageDecoder
    from ffcv_amd.pipeline import PipelineSpec
    from ffcv_amd.pipeline.graph import Graph
    from ffcv_amd.reader import Reader
    from ffcv_amd.memory_managers import OSCacheManager
    from ffcv_amd.transforms import (Cutout, NormalizeImage, ToTensor, ToDevice, ToTorchImage, RandomHorizontalFlip,
                                     RandomTranslate, RandomResizedCrop, RandomAffine, RandomRotation,
                                     RandomBrightness)
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

    ops = [RandomResizedCropRGBImageDecoder((32, 32)), RandomHorizontalFlip(), RandomAffine(15), Cutout(8)] + tail()
    g, dec = graph(jpg, ops)
    assert absorbed(ops) == [1]
    g.collect_requirements()
    assert g.groupable() and tuple(g.states[g.outputs['image'].id].shape) == (3, 32, 32)
    assert not any(type(n.operation).__name__ == '_ToHost' for n in g.exec_nodes)
    ops = [SimpleRGBImageDecoder(), RandomTranslate(2), RandomHorizontalFlip(), RandomRotation(30), Cutout(4)] + tail()
    g, dec = graph(raw, ops)
    assert dec.fused and list(dec._fused_steps) == ops[1:3] and dec._fused_normalize is None
    assert absorbed(ops) == [1, 2]
    # in front of colour jitter and behind a RandomResizedCrop transform nothing is absorbed past it
    ops = [SimpleRGBImageDecoder(), RandomResizedCrop((0.3, 1), (0.75, 4 / 3), 24), RandomAffine(10, shear=5),
           RandomBrightness(0.4), RandomHorizontalFlip()] + tail()
    g, dec = graph(raw, ops)
    assert 2 not in absorbed(ops) and not ops[1].fused
    g.collect_requirements()
    assert g.groupable()


def test_cpu_loader_matches_the_reference(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandomAffine
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'affine.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    cfg = R.CONFIGS[0]
    for interpolation, mode in (('bilinear', R.BILINEAR), ('nearest', R.NEAREST)):
        loader = Loader(fn, batch_size=8, device='cpu', seed=SEED, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomAffine(interpolation=interpolation, fill=FILL, p=0.7, **cfg),
                      ToTensor()]})
        epochs = []
        for epoch in range(2):
            applied = seen = 0
            got_all = []
            for b, (images, labels) in enumerate(loader):
                got = images.numpy()
                assert got.shape == (8, 32, 32, 3) and got.dtype == np.uint8
                for k in range(8):
                    sid = b * 8 + k
                    want, a = R.expected(ds.imgs[sid], SEED, epoch, sid, mode, fill=FILL, p=0.7, **cfg)
                    assert np.array_equal(got[k], want), (interpolation, epoch, sid, a)
                    applied += a
                    seen += 1
                got_all.append(got.copy())
            assert seen == 24 and 0 < applied < 24
            epochs.append(np.concatenate(got_all))
        assert not np.array_equal(epochs[0], epochs[1])
