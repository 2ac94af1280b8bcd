"""ElasticTransform on the host (no GPU): the constructor, the host twin of the
C ABI against the numpy statement (tests/elastic_ref.py) byte for byte, the
identity at alpha = 0, and the tile query that shows the kernel's regimes."""
import numpy as np
import pytest

from tests import affine_ref as A, elastic_ref as R
from tests.test_blur import make_inputs

SEED, EPOCH = 7, 1
MODES = (A.BILINEAR, A.NEAREST)
FILL = (7, 130, 251)
IDS = np.arange(7, dtype=np.uint64) * 5 + 3
# (shape, sigma, alpha): R = min side - 1; a workgroup per image at the defaults; partial edge tiles on both
# axes; many tiles, each with its own footprint; footprints beyond LDS; the largest R (64) and LDS plan
CASES = (((5, 5), 1.0, 50.0), ((32, 32), 5.0, 50.0), ((33, 70), 2.0, 50.0), ((97, 131), 5.0, 50.0),
         ((97, 131), 5.0, 4096.0), ((97, 131), 16.1, 50.0))
CASE_IDS = [f'{s[0]}x{s[1]}-s{g:g}-a{a:g}' for s, g, a in CASES]


def inputs(shape):
    return make_inputs(np.random.default_rng(shape[0] * 100 + shape[1]), shape)


_want = {}


def expected(case, mode):
    """The numpy statement of a case, computed once."""
    if (case, mode) not in _want:
        shape, sigma, alpha = case
        _want[case, mode] = R.warp_batch(inputs(shape), SEED, EPOCH, IDS, alpha, sigma, mode, FILL)
        _want[case, mode].setflags(write=False)
    return _want[case, mode]


def test_constructor_and_state():
    import torch as ch
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    from ffcv_amd.pipeline.state import State
    cls = T.ElasticTransform
    assert FT.ElasticTransform is cls and 'ElasticTransform' in T.__all__
    assert cls.per_sample and cls.device_aware and cls.op_id == R.OP_ELASTIC
    op = cls()
    assert (op.alpha, op.sigma, op.interpolation) == (50.0, 5.0, 'bilinear') and (op.fill_u8() == 0).all()
    assert cls(0, 1, 'nearest', 300).fill_u8().tolist() == [44, 44, 44] and cls.radius(5) == 20 and cls.radius(1) == 4
    assert cls(4096, 16.1).sigma == 16.1 and cls.radius(16.1) == 64
    for kw in (dict(alpha=-1), dict(alpha=4097), dict(alpha=float('nan')), dict(alpha=None), dict(alpha=True),
               dict(sigma=0.99), dict(sigma=16.2), dict(sigma=float('inf')), dict(sigma='x'),
               dict(interpolation='bicubic'), dict(interpolation=0), dict(fill=(1, 2)), dict(fill='red')):
        with pytest.raises(ValueError, match='ElasticTransform: ' + next(iter(kw))):
            cls(**kw)
    st, alloc = op.declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(21, 40, 3)))
    assert tuple(alloc.shape) == (21, 40, 3) and st.jit_mode
    for dt, shape in ((ch.float16, (32, 32, 3)), (np.dtype('u1'), (32, 32, 4)), (np.dtype('u1'), (20, 40, 3)),
                      (np.dtype('u1'), (40, 20, 3)), (np.dtype('u1'), (40000, 32, 3))):
        with pytest.raises(TypeError, match='ElasticTransform'):
            op.declare_state_and_memory(State(jit_mode=False, device=ch.device('cpu'), dtype=dt, shape=shape))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_host_twin_matches_numpy(hip_lib, case, mode):
    from ffcv_amd import libffcv as L
    shape, sigma, alpha = case
    imgs = inputs(shape)
    got = L.elastic_batch_host(imgs, np.full_like(imgs, 0x5A), mode, FILL, IDS, SEED, EPOCH, alpha, sigma, nthreads=3)
    want = expected(case, mode)
    assert np.array_equal(got, want)
    if (alpha, sigma) == (50.0, 5.0):      # the comparison is not of copies: most pixels of a noise image move
        assert ((want[:4] != imgs[:4]).any(axis=-1).mean(axis=(1, 2)) > 0.5).all()
    assert np.array_equal(L.elastic_batch_host(imgs, np.empty_like(imgs), mode, FILL, IDS, SEED, EPOCH, 0, sigma), imgs)


def test_weights_and_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms import ElasticTransform
    for sigma in (1.0, 2.0, 5.0, 16.1):
        w = R.weights(sigma)
        assert len(w) == 2 * ElasticTransform.radius(sigma) + 1 and w.sum() == 65536
        assert (w >= 0).all() and w.max() < 32768 and np.array_equal(w, w[::-1])
    lib, fill = L.lib(), np.zeros(3, np.uint8)
    imgs = inputs((33, 70))
    dst = np.empty_like(imgs)

    def rc(h=33, w=70, mode=0, alpha=50.0, sigma=2.0, d=dst, ids=IDS):
        return lib.ffcv_elastic_batch_host(imgs.ctypes.data, d.ctypes.data, 2, h, w, mode, fill.ctypes.data,
                                           ids.ctypes.data if ids is not None else None, SEED, 0, alpha, sigma, 0, 1)
    assert rc() == 0
    for kw in (dict(h=1), dict(w=1), dict(mode=2), dict(alpha=-0.5), dict(alpha=4096.5), dict(sigma=0.5),
               dict(sigma=16.2), dict(sigma=float('nan')), dict(sigma=5.0, h=20, w=40), dict(d=imgs), dict(ids=None)):
        assert rc(**kw) == -1, kw


def test_tile_query_shows_both_regimes(hip_lib):
    """97 x 131, sigma 5: at alpha 50 a tile's own footprint is a few pixels
    around it and is staged; at alpha 4096 footprints exceed the budget."""
    from ffcv_amd import libffcv as L
    th, tw = L.elastic_tile_shape()
    lds = L.elastic_tile_lds()
    assert (th, tw) == (32, 32) and 0 < L.elastic_lds_bytes(97, 131, 5.0) <= 64 * 1024
    sizes = {alpha: [L.elastic_tile_bytes(97, 131, A.BILINEAR, int(IDS[0]), SEED, EPOCH, alpha, 5.0, r, c)
                     for r in range(4) for c in range(5)] for alpha in (0.0, 50.0, 4096.0)}
    # alpha 0: the tile itself and bilinear's row and column
    assert sizes[0.0][6] == 33 * (((3 * 33 + 30) >> 4) * 16) and sizes[0.0][19] == 1 * (((3 * 3 + 30) >> 4) * 16)
    assert all(0 < s <= lds for s in sizes[50.0]) and sizes[50.0][6] < 3 * sizes[0.0][6]
    assert any(s > lds for s in sizes[4096.0])
    assert L.elastic_tile_bytes(97, 131, A.BILINEAR, int(IDS[0]), SEED, EPOCH, 50.0, 5.0, 4, 0) == 0   # no such tile


def test_cpu_loader_matches_the_statement(tmp_path, hip_lib):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, ElasticTransform
    from tests.helpers import NaturalDS, write
    ds = NaturalDS(16, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'elastic.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    loader = Loader(fn, batch_size=8, device='cpu', seed=SEED, pipelines={
        'image': [SimpleRGBImageDecoder(), ElasticTransform(50.0, 5.0, 'bilinear', FILL), ToTensor()]})
    for epoch in range(2):
        for b, (images, _) in enumerate(loader):
            for k in range(8):
                sid = b * 8 + k
                want = R.warp(ds.imgs[sid], R.key(SEED, epoch, sid), 50.0, 5.0, A.BILINEAR, FILL)
                assert np.array_equal(images.numpy()[k], want), (epoch, sid)
