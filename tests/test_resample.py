"""RandomResizedCrop's 'bilinear' / 'bicubic' modes without a device (DESIGN.md
s30): the statement against Pillow, the host twin against the statement."""
import numpy as np
import pytest
import torch as ch

from tests import resample_ref as R
from tests.helpers import NaturalDS, write
from tests.rrc_transform_ref import crop_draw

MODES = ('bilinear', 'bicubic')
SCALE, RATIO = (0.25, 1), (0.75, 4 / 3)         # those of resample_ref.loader


@pytest.mark.parametrize('mode', MODES)
def test_statement_is_pillow_and_coefficients_fit_24_bits(mode):
    rng, seen = np.random.default_rng(1), R.seen()
    for (h, w), (oh, ow) in R.SHAPES:
        for win in R.images(rng, h, w):
            got = R.resample(win, (0, 0, h, w), oh, ow, mode, seen)
            assert np.array_equal(got, R.pillow_resample(win, oh, ow, mode)), (mode, h, w, oh, ow)
    print(mode, seen)
    assert seen['low'] == seen['high'] == (mode == 'bicubic')    # bicubic overshoots on both sides
    assert seen['k'] < 2 ** 23 - 1       # RESAMPLE_KMAX: the shared coefficient function's clamp never acts


@pytest.mark.parametrize('mode', MODES)
def test_host_twin_is_the_statement(hip_lib, mode):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(3)
    for (h, w), (oh, ow) in R.SHAPES:
        imgs = R.images(rng, h + 5, w + 3)
        crops = np.array([(2, 3, h, w), (5, 1, h, w)], np.int32)          # windows off the origin
        out, st = np.full((2, oh, ow, 3), 0xA5, np.uint8), np.full(2, -1, np.int32)
        assert L.resample_fits(h + 5, w + 3, oh, ow, mode)
        L.resample_images_batch_host(imgs, crops, mode, out, st, nthreads=3)
        assert (st == 0).all()
        for k in range(2):
            assert np.array_equal(out[k], R.resample(imgs[k], crops[k], oh, ow, mode)), (mode, h, w, oh, ow, k)


def test_constructor_refusals():
    from ffcv_amd.transforms import RandomResizedCrop
    assert RandomResizedCrop(SCALE, RATIO, 8).interpolation == 'area'
    for m in MODES:
        assert RandomResizedCrop(SCALE, RATIO, 8, interpolation=m).interpolation == m
    for bad in ('nearest', 'lanczos', 'BICUBIC', '', None, 2):
        with pytest.raises(ValueError, match='interpolation'):
            RandomResizedCrop(SCALE, RATIO, 8, interpolation=bad)


def test_predicate_and_refused_shape(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.transforms import RandomResizedCrop
    for mode in MODES:
        for src in ((256, 256), (256, 1), (1, 256), (255, 131), (128, 256), (129, 256)):
            assert all(L.resample_fits(*src, s, s, mode) for s in range(1, 257)), (mode, src)
        ow = 256
        while L.resample_fits(256, 256, 256, ow, mode):      # a shape just past the predicate
            ow *= 2
        with pytest.raises(L.FFCVError, match='ffcv_resample_fits'):
            L.resample_images_batch_host(np.zeros((1, 256, 256, 3), np.uint8), [(0, 0, 256, 256)], mode,
                                         np.zeros((1, 256, ow, 3), np.uint8))
    op = RandomResizedCrop(SCALE, RATIO, 4096, interpolation='bicubic')
    with pytest.raises(ValueError, match='64 KiB'):
        op.declare_state_and_memory(State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'),
                                          shape=(4096, 4096, 3)))


def test_abi_guards(hip_lib):
    lib = hip_lib
    img, out = np.full((2, 8, 8, 3), 77, np.uint8), np.full((2, 4, 4, 3), 55, np.uint8)
    crops, st = np.array([[0, 0, 8, 8]] * 2, np.int32), np.zeros(2, np.int32)
    good = dict(inp=img.ctypes.data, in_stride=192, batch=2, height=8, width=8, crops=crops.ctypes.data, mode=2,
                out_h=4, out_w=4, out=out.ctypes.data, out_stride=48, status=st.ctypes.data)
    refused = (dict(inp=None), dict(crops=None), dict(out=None), dict(batch=-1), dict(height=0), dict(width=-2),
               dict(out_h=0), dict(out_w=0), dict(mode=0), dict(mode=3), dict(in_stride=191), dict(out_stride=47),
               dict(out=img.ctypes.data + 100), dict(out_w=70000))

    def host(**kw):
        return lib.ffcv_resample_images_batch_host(*dict(good, **kw).values(), 1)

    def device(**kw):                    # every refusal comes before any launch: no device is needed
        return lib.ffcv_resample_images_batch(*dict(good, **kw).values(), None)
    assert host() == 0 and (out == 77).all()
    out[:] = 55
    for kw in refused:
        assert host(**kw) == -1 and b'ffcv_resample_images_batch_host' in lib.ffcv_last_error(), kw
        assert device(**kw) == -1 and b'ffcv_resample_images_batch' in lib.ffcv_last_error(), kw
    assert (out == 55).all()
    assert host(batch=0) == 0 and device(batch=0) == 0 and (out == 55).all() and host(status=None) == 0


@pytest.fixture(scope='module')
def beton(tmp_path_factory):
    from ffcv_amd.fields import RGBImageField, IntField
    ds = NaturalDS(21, hw=(40, 56), seed=3)
    fn = write(str(tmp_path_factory.mktemp('resample') / 'raw.beton'), ds,
               {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn, ds


@pytest.mark.parametrize('mode', MODES)
def test_cpu_loader(beton, hip_lib, oracle, mode):
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    fn, ds = beton
    got = np.concatenate([np.asarray(images) for images, _ in R.loader(fn, SimpleRGBImageDecoder, 32, mode)])
    assert got.shape == (21, 32, 32, 3) and got.dtype == np.uint8
    for sid in range(21):
        window = crop_draw(oracle, 12, 0, sid, 40, 56, SCALE, RATIO)
        assert np.array_equal(got[sid], R.resample(ds.imgs[sid], window, 32, 32, mode)), sid


def test_area_is_unchanged(beton, hip_lib):
    """interpolation='area' (the default) gives rrc_images_batch_host's bytes at the contract's draws."""
    from ffcv_amd import libffcv as L
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    fn, ds = beton
    images, _ = next(iter(R.loader(fn, SimpleRGBImageDecoder, 24, 'area')))
    crops = L.crop_draw_batch_host(np.arange(8, dtype=np.uint64), 40, 56, SCALE, RATIO, 12, 0)
    want = L.rrc_images_batch_host(np.ascontiguousarray(ds.imgs[:8]), crops, np.empty((8, 24, 24, 3), np.uint8))
    assert np.array_equal(np.asarray(images), want)
