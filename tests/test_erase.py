"""RandomErasing on the CPU: the host twins of its draw and fill
(ffcv_erase_draw_batch_host, ffcv_erase_batch_host) bit for bit against the
numpy statement (tests/erase_ref.py) over the draw configurations, shapes,
element sizes, layouts, fill modes and hand-made boxes; the noise table; the
operation on host arrays; its constructor; and a CPU Loader."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import RandomErasing, RandomHorizontalFlip, NormalizeImage
from ffcv_amd.transforms.erase import noise_table
from ffcv_amd.transforms.rng import contract_seed
from tests.helpers import NaturalDS, write
from tests import cutmix_ref as C
from tests import erase_ref as R


@pytest.fixture(scope='module', autouse=True)
def built(hip_lib):
    return hip_lib


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope='module')
def ref_draws():
    """The reference draws of the six configurations, computed once."""
    return {case: R.draws(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, case[2], R.DEFAULT_RATIO, case[0], case[1])
            for case in R.DRAW_CASES}


# ---------------------------------------------------------------- draws --
@pytest.mark.parametrize('case', R.DRAW_CASES)
def test_draws_host_twin_equals_reference(ref_draws, case):
    H, W, scale = case
    boxes, keys, applied, tries = ref_draws[case]
    got_boxes, got_keys = L.erase_draw_batch_host(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, R.DRAW_P, scale,
                                                  R.DEFAULT_RATIO, H, W)
    assert got_boxes.dtype == np.int32 and np.array_equal(got_boxes, boxes)
    assert got_keys.dtype == np.uint64 and np.array_equal(got_keys, keys)
    assert np.array_equal(got_boxes[:, 2] > 0, applied & (tries > 0))
    assert np.array_equal(got_boxes[:, 3] > 0, applied & (tries > 0))


def test_draw_cases_cover_every_outcome(ref_draws):
    """Together the configurations hold samples not applied, accepted on the
    first try, accepted on a later try, and out of tries."""
    applied = np.concatenate([d[2] for d in ref_draws.values()])
    tries = np.concatenate([d[3] for d in ref_draws.values()])
    assert (~applied).any() and applied.any()
    assert (tries == 1).any() and (tries > 1).any() and (tries == 0).any()
    # an applied sample in each of the three
    assert (applied & (tries == 1)).any() and (applied & (tries > 1)).any() and (applied & (tries == 0)).any()
    # the seed of the statement is the package's contract seed
    assert contract_seed(7, 1, 5, 21) == R.hash3(7, 1, 5, 21) & 0xFFFFFFFF


def test_stream_does_not_depend_on_p_and_epochs_differ(ref_draws):
    H, W, scale = R.DRAW_CASES[0]
    args = (scale, R.DEFAULT_RATIO, H, W)
    none, keys0 = L.erase_draw_batch_host(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, 0.0, *args)
    every, keys1 = L.erase_draw_batch_host(R.DRAW_IDS, R.DRAW_SEED, R.DRAW_EPOCH, 1.0, *args)
    half = ref_draws[R.DRAW_CASES[0]][0]
    assert not none.any()
    want = np.array([R.draw(R.DRAW_SEED, R.DRAW_EPOCH, int(s), 1.0, *args)[2] or (0, 0, 0, 0) for s in R.DRAW_IDS])
    assert np.array_equal(every, want) and (every[:, 2] > 0).sum() >= 250
    on = half[:, 2] > 0
    assert np.array_equal(every[on], half[on])                       # the same boxes at p = 0.5 where it applies
    assert np.array_equal(keys0, keys1)
    other, keys2 = L.erase_draw_batch_host(R.DRAW_IDS, R.DRAW_SEED, 2, 1.0, *args)
    assert not np.array_equal(other, every) and not (keys2 == keys1).any()


def test_draw_abi_rejections():
    lib = L.lib()
    ids = np.arange(4, dtype=np.uint64)
    boxes = np.full((4, 4), -5, np.int32)

    def call(ids_p=ids.ctypes.data, n=4, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), h=32, w=32,
             b=boxes.ctypes.data):
        s, r = np.array(scale, np.float64), np.array(ratio, np.float64)
        return lib.ffcv_erase_draw_batch_host(ids_p, n, 7, 1, p, s.ctypes.data, r.ctypes.data, h, w, b, None)
    for kw in (dict(ids_p=None), dict(b=None), dict(n=-1), dict(p=-0.1), dict(p=1.5), dict(p=float('nan')),
               dict(scale=(0.5, 0.2)), dict(scale=(-0.1, 0.2)), dict(scale=(0.1, 1.2)), dict(scale=(float('nan'), 1)),
               dict(ratio=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(ratio=(1.0, float('inf'))), dict(h=0), dict(w=0),
               dict(h=32768), dict(w=-3)):
        assert call(**kw) == -1 and b'ffcv_erase_draw_batch_host' in lib.ffcv_last_error(), kw
    assert (boxes == -5).all()
    assert call() == 0 and not (boxes == -5).any()


# ----------------------------------------------------------------- fill --
def _fill_host(x, boxes, layout, value, tab, keys, nthreads):
    got = x.copy()
    if tab is not None:
        L.erase_batch_host(got, boxes, tab, keys, layout, nthreads=nthreads)
    else:
        C_ = x.shape[3] if layout == 'hwc' else x.shape[1]
        L.erase_batch_host(got, boxes, np.broadcast_to(value, (C_,)).copy(), None, layout, nthreads=nthreads)
    return got


def _random_boxes(rng, n, H, W):
    """(y, x, h, w) boxes, every fourth an edge case."""
    y, x = rng.integers(-2, H + 1, n), rng.integers(-2, W + 1, n)
    h, w = rng.integers(0, H + 3, n), rng.integers(0, W + 3, n)
    b = np.stack([y, x, h, w], 1)
    special = [(0, 0, 0, 0), (0, 0, H, W), (-3, -2, H + 5, W + 4), (H, W, 2, 2)]
    for j in range(0, n, 4):
        b[j] = special[(j // 4) % len(special)]
    return b.astype(np.int32)


@pytest.mark.parametrize('nthreads', [1, 4])
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('itemsize', [1, 2, 4])
def test_fill_shapes_and_forms_host(itemsize, mode, nthreads):
    rng = np.random.default_rng(31 + itemsize)
    for H, W in C.SIZES:
        for layout, ch_ in C.FORMS:
            for n in (1, 3, 67):
                if n == 67 and H * W > 64:
                    continue
                x = C.random_images(rng, n, H, W, layout, ch_, itemsize)
                boxes = _random_boxes(rng, n, H, W)
                value, tab, noisy = R.fill_case(rng, mode, itemsize, ch_)
                keys = rng.integers(0, 2**63, n, dtype=np.uint64) * 2 + 1 if noisy else None
                got = _fill_host(x, boxes, layout, value, tab, keys, nthreads)
                want = R.erase(x, boxes, layout, value, tab, keys)
                assert _same_bytes(got, want), (H, W, layout, ch_, n)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('layout,ch_', C.FORMS)
def test_fill_hand_made_boxes_host(layout, ch_, mode):
    """Empty, one element, a row minus a column, a column minus a row, boxes out
    of range on every side, and x swept over 0..W-1 at W = 47: row starts at
    every byte phase."""
    rng = np.random.default_rng(37)
    H, W = 33, 47
    boxes = R.hand_boxes(H, W)
    n = len(boxes)
    for itemsize in (1, 2, 4):
        x = C.random_images(rng, n, H, W, layout, ch_, itemsize)
        value, tab, noisy = R.fill_case(rng, mode, itemsize, ch_)
        keys = rng.integers(0, 2**63, n, dtype=np.uint64) if noisy else None
        want = R.erase(x, boxes, layout, value, tab, keys)
        for nthreads in (1, 4):
            assert _same_bytes(_fill_host(x, boxes, layout, value, tab, keys, nthreads), want), (itemsize, nthreads)
        hw, hx = C.as_hwc(want, layout), C.as_hwc(x, layout)
        for k in (0, 1, 2, 16, 17, 18, 19):                                   # empty or clamped to nothing
            assert np.array_equal(hw[k], hx[k]), k
        assert (hw[3] != hx[3]).any(axis=-1).sum() <= 1 and (hw[10] != hx[10]).any() and (hw[11] != hx[11]).any()
        assert np.array_equal(hw[6][:, W - 1], hx[6][:, W - 1]) and np.array_equal(hw[9][0], hx[9][0])


def test_fill_abi_rejections_host():
    lib = L.lib()
    x = np.full((4, 4, 8, 2), 7, np.uint8)
    boxes = np.array([[0, 0, 4, 8]] * 4, np.int32)
    pat = np.array([1, 1], np.uint8)
    tab = noise_table(128, 64, np.uint8)
    keys = np.arange(4, dtype=np.uint64)

    def call(im=x.ctypes.data, n=4, p=1, h=4, w=8, pb=2, b=boxes.ctypes.data, mode=0, isz=1, fill=pat.ctypes.data,
             k=None):
        return lib.ffcv_erase_batch_host(im, n, p, h, w, pb, b, mode, isz, fill, k, 1)
    noise = dict(mode=1, fill=tab.ctypes.data, k=keys.ctypes.data)
    for kw in (dict(im=None), dict(b=None), dict(fill=None), dict(n=0), dict(n=-4), dict(p=0), dict(p=-1), dict(h=0),
               dict(w=0), dict(w=-8), dict(pb=0), dict(pb=65), dict(pb=-2), dict(mode=2), dict(mode=-1),
               dict(h=2**31 - 1, w=2**31 - 1, pb=64), dict(p=2**31 - 1, h=2**31 - 1), dict(n=2**62, h=1024, w=1024),
               dict(noise, k=None), dict(noise, isz=3), dict(noise, isz=8), dict(noise, isz=0),
               dict(noise, isz=4, pb=2), dict(noise, isz=2, pb=3), dict(noise, isz=2, im=x.ctypes.data + 1)):
        assert call(**kw) == -1 and b'ffcv_erase_batch_host' in lib.ffcv_last_error(), kw
    assert (x == 7).all()
    assert call() == 0 and (x == 1).all()
    assert call(**noise) == 0 and _same_bytes(x, R.erase(np.zeros_like(x), boxes, 'hwc', None, tab, keys))


def test_fill_wrapper_rejections_host():
    x = np.zeros((4, 4, 8, 2), np.uint8)
    boxes = np.zeros((4, 4), np.int32)
    with pytest.raises(TypeError):
        L.erase_batch_host(x[:, :, ::2], boxes, np.zeros(2, np.uint8))            # not contiguous
    with pytest.raises(TypeError):
        L.erase_batch_host(x, boxes[:3], np.zeros(2, np.uint8))                   # a box short
    with pytest.raises(TypeError):
        L.erase_batch_host(x, boxes, np.zeros(3, np.uint8))                       # not one pixel
    with pytest.raises(TypeError):
        L.erase_batch_host(x, boxes, np.zeros(4096, np.uint16), np.zeros(4, np.uint64))   # another itemsize
    with pytest.raises(TypeError):
        L.erase_batch_host(x, boxes, np.zeros(4096, np.uint8), np.zeros(3, np.uint64))    # a key short


# ---------------------------------------------------------------- table --
def test_noise_table():
    t16, t32 = noise_table(0.0, 1.0, np.float16), noise_table(0.0, 1.0, np.float32)
    assert t16.shape == t32.shape == (4096,) and t16.dtype == np.float16 and t32.dtype == np.float32
    assert np.array_equal(t16, -t16[::-1]) and np.array_equal(t32, -t32[::-1])     # antisymmetric
    assert len(np.unique(t16)) == 4096 and (np.diff(t32) > 0).all()
    assert abs(float(t32.astype(np.float64).std()) - 0.9998) < 1e-3
    u8 = noise_table(128, 64, np.uint8)
    assert u8.dtype == np.uint8 and u8.min() == 0 and u8.max() == 255 and (np.diff(u8.astype(int)) >= 0).all()
    for dt, (m, s) in ((np.float16, (0.0, 1.0)), (np.float32, (0.5, 2.0)), (np.uint8, (128.0, 64.0))):
        assert _same_bytes(noise_table(m, s, dt), R.table(m, s, dt))
    with pytest.raises(TypeError):
        noise_table(0, 1, np.float64)


# ------------------------------------------------------------ operation --
def test_operation_on_host_arrays():
    rng = np.random.default_rng(5)
    idx = np.array([9, 4, 77, 1, 30, 12, 5, 200], np.uint64)
    u8 = rng.integers(0, 256, (8, 20, 24, 3), dtype=np.uint8)
    boxes, keys, _, _ = R.draws(idx, 0, 0, 0.7, R.DEFAULT_SCALE, R.DEFAULT_RATIO, 20, 24)
    assert 0 < (boxes[:, 2] > 0).sum() < 8
    for value, kw in (((3, 250, 17), dict(value=np.array([3, 250, 17], np.uint8))), (9, dict(value=np.uint8(9))),
                      ('pixel', dict(tab=R.table(128, 64, np.uint8), keys=keys))):
        x = u8.copy()
        got = RandomErasing(0.7, value=value, noise=(128, 64)).generate_code()(x, None, idx)
        assert got is x and _same_bytes(x, R.erase(u8, boxes, 'hwc', **kw)), value
    # float16 after a host NormalizeImage: N(0, 1) in normalized units
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])
    norm = NormalizeImage(mean, std, np.float16).generate_code()
    bits = np.array(norm(u8.copy(), np.zeros(u8.shape, np.int16), idx))       # float16 as its int16 bit pattern
    assert bits.dtype == np.int16 and bits.shape == u8.shape
    f16 = bits.view(np.float16)
    RandomErasing(0.7, value='pixel').generate_code()(bits, None, idx)
    x = bits.view(np.float16)
    f16 = np.array(norm(u8.copy(), np.zeros(u8.shape, np.int16), idx)).view(np.float16)
    want = R.erase(f16, boxes, 'hwc', None, R.table(0.0, 1.0, np.float16), keys)
    assert _same_bytes(x, want) and not _same_bytes(x, f16)
    y = f16.copy()
    RandomErasing(0.7, value=(0.5, -1.0, 2.0)).generate_code()(y, None, idx)   # and a float16 array as such
    assert _same_bytes(y, R.erase(f16, boxes, 'hwc', np.array([0.5, -1.0, 2.0], np.float16)))
    inside = np.concatenate([want[k, y:y + h, x0:x0 + w].reshape(-1) for k, (y, x0, h, w) in enumerate(boxes) if h > 0])
    assert abs(float(inside.astype(np.float64).mean())) < 0.1 and abs(float(inside.astype(np.float64).std()) - 1) < 0.1
    # planar float32 as a host tensor, and the NCHW view of channels-last storage
    f32 = rng.standard_normal((8, 3, 20, 24)).astype(np.float32)
    t = ch.from_numpy(f32.copy())
    RandomErasing(0.7, value=(1.5, -2.0, 0.25), layout='chw').generate_code()(t, None, idx)
    assert _same_bytes(t.numpy(), R.erase(f32, boxes, 'chw', np.array([1.5, -2.0, 0.25], np.float32)))
    hwc = rng.standard_normal((8, 20, 24, 3)).astype(np.float32)
    view = ch.from_numpy(hwc.copy()).permute(0, 3, 1, 2)
    RandomErasing(0.7, value='pixel').generate_code()(view, None, idx)
    assert _same_bytes(view.permute(0, 2, 3, 1).numpy(),
                       R.erase(hwc, boxes, 'hwc', None, R.table(0.0, 1.0, np.float32), keys))
    with pytest.raises(TypeError):
        RandomErasing(0.7, value=(1, 2)).generate_code()(u8.copy(), None, idx)      # two values, three channels
    with pytest.raises(ValueError):
        RandomErasing(0.7, value=256).generate_code()(u8.copy(), None, idx)
    with pytest.raises(ValueError):
        RandomErasing(0.7, value=1.5).generate_code()(u8.copy(), None, idx)


def test_constructor_errors():
    nan = float('nan')
    for kw, name in ((dict(p=-0.1), 'p'), (dict(p=1.1), 'p'), (dict(p=nan), 'p'), (dict(p='a'), 'p'),
                     (dict(scale=(0.3, 0.1)), 'scale'), (dict(scale=(-0.1, 0.3)), 'scale'),
                     (dict(scale=(0.1, 1.1)), 'scale'), (dict(scale=(nan, 0.3)), 'scale'), (dict(scale=0.3), 'scale'),
                     (dict(scale=(0.1, 0.2, 0.3)), 'scale'), (dict(ratio=(0.0, 1.0)), 'ratio'),
                     (dict(ratio=(2.0, 1.0)), 'ratio'), (dict(ratio=(1.0, nan)), 'ratio'),
                     (dict(ratio=(-1.0, 1.0)), 'ratio'), (dict(value='rand'), 'value'), (dict(value=nan), 'value'),
                     (dict(value=(1, float('inf'))), 'value'), (dict(value=()), 'value'), (dict(value=None), 'value'),
                     (dict(value=(1, 'a')), 'value'), (dict(noise=(0.0, -1.0)), 'noise'),
                     (dict(noise=(nan, 1.0)), 'noise'), (dict(noise=1.0), 'noise'), (dict(layout='nchw'), 'layout')):
        with pytest.raises(ValueError, match=name):
            RandomErasing(**kw)
    op = RandomErasing()
    assert (op.p, op.scale, op.ratio, op.value, op.noise, op.layout) == (0.5, (0.02, 0.33), (0.3, 3.3), (0,),
                                                                        (0.0, 1.0), 'auto')
    assert RandomErasing.per_sample and RandomErasing.device_aware and RandomErasing.with_indices
    assert not RandomErasing.per_batch


def test_dropin_imports():
    from ffcv.transforms import RandomErasing as A
    import ffcv.transforms.erase as m
    assert A is RandomErasing and m.RandomErasing is RandomErasing
    assert {'ffcv_erase_draw_batch', 'ffcv_erase_draw_batch_host', 'ffcv_erase_batch',
            'ffcv_erase_batch_host'} <= set(L.EXPORTED_SYMBOLS)


def test_declarations():
    from ffcv_amd.pipeline.state import State
    host = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(32, 32, 3))
    state, query = RandomErasing().declare_state_and_memory(host)
    assert state == host and query is None                                    # in place, no memory
    dev = ch.device('cuda:0')
    for dt in (ch.uint8, ch.float16, ch.float32, np.dtype('<i2')):           # int16: NormalizeImage's float16 bits
        s = State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32))
        assert RandomErasing(value='pixel').declare_state_and_memory(s) == (s, None)
    for dt in (ch.float64, ch.int64, ch.bfloat16):
        with pytest.raises(TypeError):
            RandomErasing().declare_state_and_memory(State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32)))
    with pytest.raises(TypeError):
        RandomErasing(value='pixel').declare_state_and_memory(
            State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('f8'), shape=(32, 32, 3)))


# --------------------------------------------------------------- Loader --
@pytest.fixture(scope='module')
def beton():
    fn = os.path.join(tempfile.mkdtemp(), 'erase_raw.beton')
    write(fn, NaturalDS(40, hw=(32, 32), seed=3), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn


def _epoch(loader):
    return np.concatenate([np.array(im.numpy() if isinstance(im, ch.Tensor) else im) for im, _ in loader])


def test_cpu_loader_matches_reference(beton):
    kw = dict(batch_size=16, device='cpu', seed=23, drop_last=False)
    head = [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5)]
    base = Loader(beton, pipelines={'image': list(head), 'label': [IntDecoder()]}, **kw)
    value = (7, 130, 255)

    def erased(**more):
        return Loader(beton, pipelines={'image': head + [RandomErasing(0.6, value=value)], 'label': [IntDecoder()]},
                      **kw, **more)
    one, again, grouped = erased(), erased(), erased(batches_per_launch=3)
    assert one.graph.groupable()
    idx = np.arange(40)
    firsts = []
    for epoch in range(2):
        b, got = _epoch(base), _epoch(one)
        assert b.shape == (40, 32, 32, 3) and got.shape == b.shape
        boxes, _, _, _ = R.draws(idx, 23, epoch, 0.6, R.DEFAULT_SCALE, R.DEFAULT_RATIO, 32, 32)
        assert 5 < (boxes[:, 2] > 0).sum() < 35
        assert _same_bytes(got, R.erase(b, boxes, 'hwc', np.array(value, np.uint8))), epoch
        assert _same_bytes(_epoch(again), got) and _same_bytes(_epoch(grouped), got)      # deterministic under a seed
        firsts.append(boxes)
    assert not np.array_equal(firsts[0], firsts[1])                                       # epochs differ
