"""Poison / ReplaceLabel on the CPU: the drop-in imports, the host twin of the
poison kernel (ffcv_poison_batch_host: the kernel's own membership and pixel
functions) bit for bit against numpy's statements on a float32 temp
(tests/poison_ref.py), the operations on host arrays, the constructors and
declarations, launch groups in the graph, and a CPU Loader epoch in random
order."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader, OrderOption
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.pipeline.state import State
from ffcv_amd.pipeline.allocation_query import AllocationQuery
from tests.helpers import NaturalDS, write
from tests import poison_ref as R

# ffcv/transforms/__init__.py of the reference
REFERENCE_ALL = ['ToTensor', 'ToDevice', 'ToTorchImage', 'NormalizeImage', 'Convert', 'Squeeze', 'View',
                 'RandomResizedCrop', 'RandomHorizontalFlip', 'RandomTranslate', 'Cutout', 'ImageMixup', 'LabelMixup',
                 'MixupToOneHot', 'Poison', 'ReplaceLabel', 'ModuleWrapper', 'RandomBrightness', 'RandomContrast',
                 'RandomSaturation']


@pytest.fixture(scope='module', autouse=True)
def built(hip_lib):
    return hip_lib


def _ops():
    from ffcv_amd.transforms import Poison, ReplaceLabel
    return Poison, ReplaceLabel


def _tables(mask, alpha):
    a3 = R.alpha3_of(alpha)
    return np.asarray(1 - a3, np.float64), np.asarray(mask.astype(float) * a3, np.float64)


def _twin(images, mask, alpha, sample_ids, indices, clamp=(0, 255), nthreads=1):
    keep, add = _tables(mask, alpha)
    ids = np.unique(np.asarray(indices, np.uint64))
    return L.poison_batch_host(images.copy(), sample_ids, ids, keep, add, clamp, nthreads=nthreads)


# -------------------------------------------------------------- imports --
def test_dropin_imports_and_reference_names():
    from ffcv.transforms import Poison, ReplaceLabel
    import ffcv.transforms as FT
    import ffcv.transforms.poison as p
    import ffcv.transforms.replace_label as r
    import ffcv_amd.transforms as T
    assert Poison is T.Poison is p.Poison and ReplaceLabel is T.ReplaceLabel is r.ReplaceLabel
    missing = [n for n in REFERENCE_ALL if n != 'RandomResizedCrop' and (n not in T.__all__ or not hasattr(FT, n))]
    assert not missing, missing
    assert Poison.per_sample and Poison.device_aware and Poison.with_indices
    assert ReplaceLabel.per_sample and ReplaceLabel.device_aware and ReplaceLabel.with_indices


# ------------------------------------------------------------ host twin --
@pytest.mark.parametrize('alpha_dtype', [np.float64, np.float32])
def test_all_pairs_bit_exact_and_discriminating(alpha_dtype):
    """Every (v, m) byte pair under every opacity of ALPHAS: the host twin
    equals the numpy statement bit for bit, and the same input tells the
    statement from its cheaper relatives."""
    image, mask, alpha = R.all_pairs(alpha_dtype)
    assert alpha.dtype == alpha_dtype
    want = R.poison_np(image, mask, alpha, [5], [5])
    got = _twin(image, mask, alpha, [5], [5], nthreads=3)
    assert np.array_equal(got, want)
    assert int(want.min()) == 0 and int(want.max()) == 255
    f32, f64, f64_once = R.other_forms(image[0], mask, alpha)
    n32, n64, nonce = (int((x != want[0]).sum()) for x in (f32, f64, f64_once))
    print(f'{np.dtype(alpha_dtype).name} alpha, differing values: float32 only {n32}, float64 without '
          f'intermediate rounding {n64}, float64 with one final rounding {nonce}')
    assert n32 > 0 and n64 > 0
    if alpha_dtype == np.float32:
        assert nonce > 0          # what catches a missing rounding of the product


@pytest.mark.parametrize('alpha_dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_host_twin_shapes_batches_index_sets(shape, alpha_dtype):
    rng = np.random.default_rng(sum(shape))
    case = 0
    for n in R.BATCHES:
        images, mask, alpha, sids = R.random_case(rng, shape, n, alpha_dtype)
        for kind in R.INDEX_SETS:
            indices = R.index_set(kind, sids)
            clamp = R.CLAMPS[case % len(R.CLAMPS)]
            nthreads = (1, 4)[case % 2]
            case += 1
            want = R.poison_np(images, mask, alpha, sids, indices, clamp)
            got = _twin(images, mask, alpha, sids, indices, clamp, nthreads)
            assert np.array_equal(got, want), (shape, n, kind, clamp)
            hit = R.chosen(sids, indices)
            for k in range(n):                      # unpoisoned samples are byte-identical
                if k not in hit:
                    assert np.array_equal(got[k], images[k])
            assert len(hit) == {'empty': 0, 'absent': 0, 'all': n, 'first': 1, 'last': 1,
                                'every_other': (n + 1) // 2, 'duplicates': min(n, 2)}[kind]


@pytest.mark.parametrize('clamp', R.CLAMPS)
@pytest.mark.parametrize('nthreads', [1, 4])
def test_host_twin_clamps_and_threads(clamp, nthreads):
    rng = np.random.default_rng(17)
    images, mask, alpha, sids = R.random_case(rng, (37, 29, 3), 9, np.float64)
    indices = R.index_set('every_other', sids)
    want = R.poison_np(images, mask, alpha, sids, indices, clamp)
    got = _twin(images, mask, alpha, sids, indices, clamp, nthreads)
    assert np.array_equal(got, want)
    hit = R.chosen(sids, indices)
    assert got[hit].min() >= int(clamp[0]) and got[hit].max() <= int(clamp[1])


def test_host_abi_rejections():
    lib = L.lib()
    a = np.full((4, 24), 7, np.uint8)
    sid = np.arange(4, dtype=np.int64)
    pid = np.array([1, 2], np.uint64)
    keep = np.full(24, 0.5)
    add = np.full(24, 3.0)

    def call(im=a.ctypes.data, n=4, e=24, s=sid.ctypes.data, p=pid.ctypes.data, npo=2, k=keep.ctypes.data,
             ad=add.ctypes.data, lo=0.0, hi=255.0):
        return lib.ffcv_poison_batch_host(im, n, e, s, p, npo, k, ad, lo, hi, 1)
    for kw in (dict(im=None), dict(s=None), dict(p=None), dict(k=None), dict(ad=None), dict(n=0), dict(n=-1),
               dict(e=0), dict(e=-3), dict(npo=-1), dict(n=1 << 40, e=1 << 40), dict(k=keep.ctypes.data + 4),
               dict(ad=add.ctypes.data + 1), dict(s=sid.ctypes.data + 4), dict(p=pid.ctypes.data + 2),
               dict(lo=-1.0), dict(hi=256.0), dict(lo=9.0, hi=8.0), dict(lo=float('nan')), dict(hi=float('nan'))):
        assert call(**kw) == -1 and b'ffcv_poison_batch_host' in lib.ffcv_last_error(), kw
    assert (a == 7).all()
    assert call(npo=0) == 0 and call(npo=0, p=None) == 0 and (a == 7).all()     # an empty set: nothing to do
    assert call() == 0
    assert (a[[1, 2]] == 6).all() and (a[[0, 3]] == 7).all()                    # float32(7 * 0.5) + 3 = 6.5 -> 6
    with pytest.raises(TypeError):
        L.poison_batch_host(a.astype(np.int16), sid, pid, keep, add)
    with pytest.raises(TypeError):
        L.poison_batch_host(a[:, ::2], sid, pid, keep[::2], add[::2])
    with pytest.raises(TypeError):
        L.poison_batch_host(a, sid[:3], pid, keep, add)
    with pytest.raises(TypeError):
        L.poison_batch_host(a, sid, pid, keep[:5], add)


# ------------------------------------------------------- the operations --
@pytest.mark.parametrize('alpha_dtype', [np.float64, np.float32])
def test_poison_op_on_host_arrays(alpha_dtype):
    Poison, _ = _ops()
    rng = np.random.default_rng(2)
    images, mask, alpha, sids = R.random_case(rng, (9, 7, 3), 6, alpha_dtype)
    indices = R.index_set('every_other', sids) + [10 ** 6]
    want = R.poison_np(images, mask, alpha, sids, indices, (3, 250))
    code = Poison(mask, alpha, indices, clamp=(3, 250)).generate_code()
    assert code.with_indices and code.is_parallel
    work = images.copy()
    out = code(work, np.zeros(images.shape, np.float32), sids)
    assert out is work and np.array_equal(work, want)                 # in place, returns images
    # other dtypes and layouts go through the numpy statements
    for dt in (np.int16, np.float32, np.float64):
        x = images.astype(dt)
        got = code(x, np.zeros(images.shape, np.float32), sids)
        assert got is x and got.dtype == dt
        assert np.array_equal(got, R.poison_np(images.astype(dt), mask, alpha, sids, indices, (3, 250))), dt
    strided = np.zeros((6, 9, 7, 4), np.uint8)[..., :3]
    strided[:] = images
    assert not strided.flags.c_contiguous
    assert np.array_equal(code(strided, np.zeros(images.shape, np.float32), sids), want)
    t = ch.from_numpy(images.copy())
    got = code(t, np.zeros(images.shape, np.float32), sids)
    assert got is t and np.array_equal(t.numpy(), want)
    # integer opacities and a float mask
    ia = rng.integers(0, 2, (9, 7))
    fm = rng.random((9, 7, 3)) * 255
    got = Poison(fm, ia, indices).generate_code()(images.copy(), None, sids)
    assert np.array_equal(got, R.poison_np(images, fm, ia, sids, indices))


def test_poison_constructor_errors():
    Poison, _ = _ops()
    mask, alpha = np.zeros((4, 5, 3), np.uint8), np.full((4, 5), 0.5)
    op = Poison(mask, alpha, [7, 3, 7, 1])
    assert op.indices.dtype == np.uint64 and op.indices.tolist() == [1, 3, 7] and op.clamp == (0, 255)
    assert Poison(mask, alpha, []).indices.size == 0
    assert Poison(mask, alpha, np.array([2, 2], np.int32), clamp=(0.5, 100.5)).indices.tolist() == [2]
    nan_alpha, inf_mask = alpha.copy(), mask.astype(np.float64)
    nan_alpha[1, 1] = np.nan
    inf_mask[0, 0, 0] = np.inf
    for bad_mask, bad_alpha in ((np.zeros((4, 5), np.uint8), alpha), (np.zeros((4, 5, 1), np.uint8), alpha),
                                (np.zeros((4, 5, 4), np.uint8), alpha), (mask, np.zeros((5, 4))),
                                (mask, np.zeros((4, 5, 3))), (mask, 0.5), (mask, nan_alpha), (inf_mask, alpha),
                                (np.zeros((0, 5, 3), np.uint8), np.zeros((0, 5)))):
        with pytest.raises(ValueError):
            Poison(bad_mask, bad_alpha, [1])
    for bad in ([-1], [1, -5], [0.5], [1.0], ['a'], [True]):
        with pytest.raises(ValueError):
            Poison(mask, alpha, bad)
    for bad in ((-1, 255), (0, 256), (9, 8), (0,), (0, 1, 2), None, (float('nan'), 5), ('a', 'b')):
        with pytest.raises(ValueError):
            Poison(mask, alpha, [1], clamp=bad)


def test_declarations():
    Poison, ReplaceLabel = _ops()
    op = Poison(np.zeros((32, 32, 3), np.uint8), np.zeros((32, 32)), [1])
    host = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(32, 32, 3))
    st, q = op.declare_state_and_memory(host)
    assert st == host and q == AllocationQuery((32, 32, 3), np.dtype('float32'))       # the reference's temp
    dev = ch.device('cuda:0')
    st, q = op.declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.uint8, shape=(32, 32, 3)))
    assert q is None and st.dtype == ch.uint8 and st.device == dev                    # in place, nothing allocated
    for dt, shape in ((ch.float16, (32, 32, 3)), (ch.float32, (32, 32, 3)), (ch.uint8, (3, 32, 32))):
        with pytest.raises(TypeError, match='NormalizeImage'):
            op.declare_state_and_memory(State(jit_mode=False, device=dev, dtype=dt, shape=shape))
    with pytest.raises(TypeError, match='mask'):
        op.declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.uint8, shape=(32, 16, 3)))
    with pytest.raises(TypeError, match='mask'):
        op.declare_state_and_memory(State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(16, 32, 3)))
    lab = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('<i8'), shape=(1,))
    assert ReplaceLabel([1], 3).declare_state_and_memory(lab) == (lab, None)
    st, q = ReplaceLabel([1], 3).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.int64, shape=(1,)))
    assert q is None
    with pytest.raises(TypeError, match='int64'):
        ReplaceLabel([1], 3).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.float32, shape=(1,)))


@pytest.mark.parametrize('dtype', [np.int64, np.int32])
@pytest.mark.parametrize('column', [False, True])
def test_replace_label_on_host(dtype, column):
    _, ReplaceLabel = _ops()
    rng = np.random.default_rng(4)
    sids = rng.permutation(50)[:13].astype(np.uint64) + np.uint64(3)
    labels = rng.integers(0, 10, (13, 1) if column else (13,)).astype(dtype)
    for kind in R.INDEX_SETS:
        indices = R.index_set(kind, sids)
        want = R.replace_label_np(labels, sids, indices, 42)
        work = labels.copy()
        got = ReplaceLabel(indices, 42).generate_code()(work, None, sids)
        assert got is work and got.dtype == dtype and got.shape == labels.shape
        assert np.array_equal(got, want), kind
        t = ch.from_numpy(labels.copy())
        assert np.array_equal(ReplaceLabel(indices, 42).generate_code()(t, None, sids).numpy(), want)
    for bad in (1.5, '3', None, True):
        with pytest.raises(ValueError):
            ReplaceLabel([1], bad)
    with pytest.raises(ValueError):
        ReplaceLabel([-1], 3)
    assert ReplaceLabel([4, 4, 2], np.int64(7)).indices.tolist() == [2, 4]


# ------------------------------------------------------ graph and Loader --
N_SAMPLES = 64


@pytest.fixture(scope='module')
def dataset():
    ds = NaturalDS(N_SAMPLES, hw=(32, 32), seed=8)
    fn = os.path.join(tempfile.mkdtemp(), 'poison_raw.beton')
    write(fn, ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn, ds


def _epoch(loader):
    ims, labs = [], []
    for im, lab in loader:
        ims.append(np.array(im))
        labs.append(np.array(lab))
    return np.concatenate(ims), np.concatenate(labs)


def test_cpu_loader_random_order(dataset):
    """Exactly the chosen dataset indices come out stamped and relabelled,
    whatever the batch order; all others equal a Loader without the
    operations."""
    Poison, ReplaceLabel = _ops()
    fn, ds = dataset
    rng = np.random.default_rng(1)
    mask = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    alpha = rng.random((32, 32))
    alpha[:8] = 1.0
    indices = [0, 5, 17, 18, 33, 63, 63, 1000]
    kw = dict(batch_size=16, device='cpu', seed=7, order=OrderOption.RANDOM, drop_last=False)
    base = Loader(fn, pipelines={'image': [SimpleRGBImageDecoder()], 'label': [IntDecoder()]}, **kw)
    both = Loader(fn, pipelines={'image': [SimpleRGBImageDecoder(), Poison(mask, alpha, indices)],
                                 'label': [IntDecoder(), ReplaceLabel(indices, 11)]}, **kw)
    assert both.graph.groupable()
    where = {im.tobytes(): i for i, (im, _) in enumerate(ds[i] for i in range(N_SAMPLES))}
    orders = []
    for epoch in range(2):
        b_im, b_lab = _epoch(base)
        p_im, p_lab = _epoch(both)
        sids = np.array([where[im.tobytes()] for im in b_im])
        assert sorted(sids.tolist()) == list(range(N_SAMPLES))
        orders.append(sids)
        assert np.array_equal(p_im, R.poison_np(b_im, mask, alpha, sids, indices))
        assert np.array_equal(p_lab, R.replace_label_np(b_lab, sids, indices, 11)) and p_lab.dtype == b_lab.dtype
        changed = sorted(int(s) for k, s in enumerate(sids) if not np.array_equal(p_im[k], b_im[k]))
        assert changed == [0, 5, 17, 18, 33, 63]
        assert sorted(int(s) for k, s in enumerate(sids) if p_lab[k] == 11) == changed
    assert not np.array_equal(orders[0], np.arange(N_SAMPLES)) and not np.array_equal(orders[0], orders[1])
