"""RandomPerspective on the host (no GPU): the constructor, the host twins of
the C ABI against the numpy statement (tests/perspective_ref.py) bit for bit
(draws, coefficients, pixels), and a CPU Loader."""
import numpy as np
import pytest

from tests import affine_ref as A, perspective_ref as R
from tests.helpers import NaturalDS, write
from tests.test_blur import make_inputs, mixed_apply

SEED = 7
MODES = (A.BILINEAR, A.NEAREST)
FILL = (7, 130, 251)
WHOLE = 16384                # asserted against the library
# 43 x 127 is the largest whole-image shape (3 H W = 16,383), 43 x 128 the first beyond it; 97 x 131: 4 x 5 tiles
SHAPES = ((2, 2), (5, 7), (43, 127), (43, 128), (97, 131))


def strong_quad(H, W):
    """A top edge of a tenth of the width at 0.4 H: the horizon crosses the image above it."""
    return [int(0.45 * W), int(0.4 * H), int(0.55 * W) + 1, int(0.4 * H), int(0.76 * W), H - 1, 0, H - 1]


def coef_sets(H, W):
    """name -> nine float64 coefficients for H x W images."""
    drawn = next(q for a, q in (R.draw_coefficients(SEED, 0, i, 1.0, 0.5, H, W) for i in range(64)) if a)
    return {'identity': R.IDENTITY, 'drawn': drawn, 'strong': R.coefficients(strong_quad(H, W), H, W),
            # hand-written: den = 0 on the line r = 0.6 H - 0.15 c, fill beyond it
            'horizon': np.array([1, 0.25, -3, 0.125, 1, 2, -0.25 / H, -1 / (0.6 * H), 1], np.float64),
            'shift': np.array([1, 0, 1.5, 0, 1, -0.75, 0, 0, 1], np.float64),
            'nan': np.array([1, 0, 0, 0, 1, 0, 0, np.nan, 1], np.float64),
            'huge': np.array([1e9, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)}


def test_constructor_and_state():
    import torch as ch
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    from ffcv_amd.pipeline.state import State
    cls = T.RandomPerspective
    assert FT.RandomPerspective is cls and 'RandomPerspective' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_PERSPECTIVE
    op = cls()
    assert (op.distortion_scale, op.p, op.interpolation) == (0.5, 0.5, 'bilinear') and (op.fill_u8() == 0).all()
    assert cls(1, 1, 'nearest', 300).fill_u8().tolist() == [44, 44, 44] and cls(0).distortion_scale == 0.0
    for bad in (-0.1, 1.1, float('nan'), float('inf'), None, 'x', True, (0.5,)):
        with pytest.raises(ValueError, match='RandomPerspective: distortion_scale'):
            cls(bad)
    for kw in (dict(interpolation='bicubic'), dict(interpolation=0), dict(fill=(1, 2)), dict(fill='red'),
               dict(fill=(0, 0, float('nan'))), dict(p=-0.01), dict(p=1.01), dict(p=None)):
        with pytest.raises(ValueError, match=next(iter(kw)) if 'p' not in kw else 'p must'):
            cls(**kw)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(8, 6, 3)))
    assert tuple(alloc.shape) == (8, 6, 3) and st.jit_mode
    for dt, shape in ((ch.float16, (8, 6, 3)), (np.dtype('u1'), (8, 6, 4)), (np.dtype('u1'), (1, 6, 3)),
                      (np.dtype('u1'), (8, 1, 3)), (np.dtype('u1'), (40000, 6, 3))):
        with pytest.raises(TypeError, match='RandomPerspective'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


@pytest.mark.parametrize('d', (0.0, 0.5, 1.0))
def test_host_draws_match_numpy_bit_for_bit(hip_lib, d):
    from ffcv_amd import libffcv as L
    ids = np.arange(200, dtype=np.uint64)
    degenerate = 0
    for H, W in ((2, 2), (2, 9), (9, 2), (32, 32), (97, 131)):
        apply, coef = L.perspective_draw_batch_host(ids, SEED, 3, 0.7, d, H, W)
        for i in ids:
            a, q = R.draw_coefficients(SEED, 3, int(i), 0.7, d, H, W)
            assert bool(apply[i]) == a and np.array_equal(coef[i].view(np.uint64), q.view(np.uint64)), (H, W, i)
            degenerate += not R.convex(R.draws(SEED, 3, int(i), 0.7, d, H, W)[1])
        assert apply.sum() < 200 and (apply.sum() > 0 or (H, W) == (2, 2))   # 2 x 2 at d = 1: the identity or nothing
        if d == 0:
            assert (coef == R.IDENTITY).all()           # the image's own corners: the exact identity
    assert (degenerate > 0) == (d == 1.0)               # quadrilaterals that are not convex occur, at a side of 2
    lib = L.lib()
    for h, w, p, dd in ((1, 9, 0.5, 0.5), (9, 32768, 0.5, 0.5), (9, 9, 1.5, 0.5), (9, 9, 0.5, -0.1), (9, 9, 0.5, 2)):
        assert lib.ffcv_perspective_draw_batch_host(ids.ctypes.data, 2, 0, 0, p, dd, h, w, apply.ctypes.data,
                                                    coef.ctypes.data) == -1


@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_host_pixels_match_numpy(hip_lib, shape):
    from ffcv_amd import libffcv as L
    imgs = make_inputs(np.random.default_rng(shape[0] * 100 + shape[1]), shape)
    apply = mixed_apply()
    for mode in MODES:
        for name, q in coef_sets(*shape).items():
            coef = np.stack([q] * len(imgs))
            got = L.perspective_batch_host(imgs, np.full_like(imgs, 0x5A), mode, FILL, apply, coef, nthreads=3)
            assert np.array_equal(got, R.warp_batch(imgs, coef, mode, apply, FILL)), (shape, mode, name)
            if name == 'identity':
                assert np.array_equal(got, imgs)
            if name in ('nan', 'huge'):
                assert (got[0, :, 1:] == np.array(FILL, np.uint8)).all()
    H, W = shape
    far = R.warp(imgs[0], coef_sets(H, W)['horizon'], A.BILINEAR, FILL)[int(0.6 * H) + 1:]
    assert (far == np.array(FILL, np.uint8)).all()      # behind the horizon
    lib, fill = L.lib(), np.zeros(3, np.uint8)
    dst = np.empty_like(imgs)
    for h, w, mode, d in ((1, W, 0, dst), (H, 1, 0, dst), (H, W, 2, dst), (H, W, 0, imgs)):
        assert lib.ffcv_perspective_batch_host(imgs.ctypes.data, d.ctypes.data, 2, h, w, mode, fill.ctypes.data,
                                               apply.ctypes.data, coef.ctypes.data, 0, 1) == -1


def test_tile_bytes_show_the_regimes(hip_lib):
    from ffcv_amd import libffcv as L
    assert L.perspective_whole_bytes() == WHOLE
    th, tw = L.perspective_tile_shape()
    assert L.perspective_tile_bytes(43, 127, 0, R.IDENTITY, 0, 0) == ((WHOLE - 1 + 30) >> 4) * 16
    assert L.perspective_tile_bytes(43, 127, 0, R.IDENTITY, 0, 1) == 0         # no such tile
    # the identity stages the tile's pixels, a pixel more on each side, and bilinear's row and column
    assert L.perspective_tile_bytes(97, 131, 1, R.IDENTITY, 1, 1) == (th + 2) * (((3 * (tw + 2) + 30) >> 4) * 16)
    assert L.perspective_tile_bytes(97, 131, 0, R.IDENTITY, 1, 1) == (th + 3) * (((3 * (tw + 3) + 30) >> 4) * 16)


def test_cpu_loader_matches_the_statement(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, RandomPerspective
    ds = NaturalDS(24, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'persp.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    for interpolation, mode in (('bilinear', A.BILINEAR), ('nearest', A.NEAREST)):
        loader = Loader(fn, batch_size=8, device='cpu', seed=SEED, pipelines={
            'image': [SimpleRGBImageDecoder(), RandomPerspective(0.6, 0.7, interpolation, FILL), ToTensor()]})
        for epoch in range(2):
            applied = 0
            for b, (images, _) in enumerate(loader):
                for k in range(8):
                    sid = b * 8 + k
                    a, q = R.draw_coefficients(SEED, epoch, sid, 0.7, 0.6, 32, 32)
                    want = R.warp(ds.imgs[sid], q, mode, FILL) if a else ds.imgs[sid]
                    assert np.array_equal(images.numpy()[k], want), (interpolation, epoch, sid, a)
                    applied += a
            assert 0 < applied < 24
