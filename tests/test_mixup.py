"""ImageMixup / LabelMixup / MixupToOneHot on the CPU: the host twin of the
mixup kernel (ffcv_mixup_batch_host, the kernel's own pixel function) bit for
bit against numpy's float64 statement (tests/mixup_ref.py), the operations on
host arrays, the constructors, the drop-in imports, launch groups in the
graph, and CPU Loaders with one and with three batches per launch."""
import os
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.pipeline.operation import Operation
from ffcv_amd.transforms import ToTensor, RandomHorizontalFlip, ImageMixup, LabelMixup, MixupToOneHot
from tests.helpers import NaturalDS, write
from tests import mixup_ref as R


@pytest.fixture(scope='module', autouse=True)
def built(hip_lib):
    return hip_lib


def _code(op):
    return op.generate_code()


# ------------------------------------------------------------ host twin --
def test_all_pairs_bit_exact_and_discriminating():
    """Every (a, b) byte pair under the fixed lambdas and 16 beta draws, one
    call: 25 batches of the two all-pairs samples, one lambda per batch."""
    pairs = R.all_pairs()
    lams = R.all_pairs_lambdas()
    assert len(lams) == 25 and set(R.FIXED_LAMBDAS) <= set(lams.tolist())
    imgs = np.concatenate([pairs] * len(lams))
    got = L.mixup_batch_host(imgs, np.full_like(imgs, 0xA5), lams, 2, True, nthreads=3)
    want = R.mix_segments(imgs, lams, 2, True)
    assert np.array_equal(got, want)
    assert int(want.max()) == 255 and int(want.min()) == 0

    # identical neighbours one below the input: 41 of 256 at l = 0.3
    k = list(lams).index(0.3)
    diag = want[2 * k].reshape(256, 256).diagonal().astype(int)
    assert int((diag == np.arange(256) - 1).sum()) == 41 and int((diag == np.arange(256)).sum()) == 215

    # the lambda set tells the float64 statement from its cheaper relatives
    a = pairs[0].astype(np.float64)
    b = pairs[1].astype(np.float64)
    n32 = nlerp = nfma = 0
    for l in lams:
        ref = (np.float64(l) * a + (1 - np.float64(l)) * b).astype(np.uint8)
        l32 = np.float32(l)
        f32 = (l32 * pairs[0].astype(np.float32) + (np.float32(1) - l32) * pairs[1].astype(np.float32))
        n32 += int((f32.astype(np.uint8) != ref).sum())
        nlerp += int(((b + np.float64(l) * (a - b)).astype(np.uint8) != ref).sum())
        # fma(l, a, fl((1 - l) * b)): only sums within 1e-9 of an integer can
        # truncate differently (the two forms differ by under one ulp)
        n = (1 - np.float64(l)) * b
        s = np.float64(l) * a + n
        for j in np.nonzero(np.abs(s - np.rint(s)) < 1e-9)[0]:
            fused = float(Fraction(float(l)) * int(a[j]) + Fraction(float(n[j])))
            nfma += int(int(fused) != int(ref[j]))
    print(f'differing values: float32 {n32}, lerp {nlerp}, fused multiply-add {nfma}')
    assert n32 > 0 and nlerp > 0 and nfma > 0


SEGMENT_CASES, ELEMS, _inputs, _lams = R.SEGMENT_CASES, R.ELEMS, R.random_inputs, R.random_lambdas


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_shapes_and_segments_host(dtype):
    rng = np.random.default_rng(11)
    for elems in ELEMS:
        for n, bs in SEGMENT_CASES:
            if n == 67 and elems > 3072:
                continue
            for same in (False, True):
                imgs = _inputs(rng, n, elems, dtype)
                lam = _lams(rng, n, bs, same)
                got = L.mixup_batch_host(imgs, np.zeros_like(imgs), lam, bs, same, nthreads=2)
                with np.errstate(over='ignore', invalid='ignore'):
                    want = R.mix_segments(imgs, lam, bs, same)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (elems, n, bs, same)


def test_host_abi_rejections():
    lib = L.lib()
    a = np.zeros((4, 8), np.uint8)
    o = np.full((4, 8), 7, np.uint8)
    lam = np.full(4, 0.5)

    def call(inp=a.ctypes.data, out=o.ctypes.data, n=4, e=8, dt=L.MIXUP_U8, bs=4, lm=lam.ctypes.data):
        return lib.ffcv_mixup_batch_host(inp, out, n, e, dt, bs, lm, 0, 1)
    for kw in (dict(inp=None), dict(out=None), dict(lm=None), dict(n=0), dict(e=0), dict(bs=0), dict(n=-1), dict(dt=0),
               dict(dt=3), dict(out=a.ctypes.data), dict(out=a.ctypes.data + 31)):
        assert call(**kw) == -1 and b'ffcv_mixup_batch_host' in lib.ffcv_last_error(), kw
    assert (o == 7).all()
    assert call() == 0
    with pytest.raises(TypeError):
        L.mixup_batch_host(a.astype(np.int16), o.astype(np.int16), lam, 4, False)
    with pytest.raises(TypeError):
        L.mixup_batch_host(a[:, ::2], o[:, ::2], lam, 4, False)


# ------------------------------------------------------- the operations --
@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('alpha', [0.2, 1.0, 2.0])
def test_ops_on_numpy_arrays(alpha, same):
    rng = np.random.default_rng(5)
    idx = np.array([9, 4, 77, 1, 30, 12, 5], np.uint64)
    imgs = rng.integers(0, 256, (7, 5, 6, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, (7, 1)).astype(np.int64)
    got = _code(ImageMixup(alpha, same))(imgs, np.zeros_like(imgs), idx)
    assert np.array_equal(got, R.image_mixup(imgs, idx, alpha, same))
    lab = _code(LabelMixup(alpha, same))(labels, np.zeros((7, 3), np.float32), idx)
    assert lab.dtype == np.float32 and np.array_equal(lab, R.label_mixup(labels, idx, alpha, same))
    # the same lambdas in both, and the wrap: sample 0's neighbour is the last
    lam = R.draw_lambdas(idx[-1], alpha, same, 7)
    assert np.array_equal(lab[:, 2], np.broadcast_to(np.asarray(lam, np.float64), (7,)).astype(np.float32))
    assert lab[0, 1] == labels[6, 0] and lab[1, 1] == labels[0, 0]
    l0 = np.float64(lam if same else lam[0])
    assert np.array_equal(got[0], (l0 * imgs[0].astype(np.float64) + (1 - l0) * imgs[6].astype(np.float64))
                          .astype(np.uint8))
    # B = 1 mixes a sample with itself
    one = _code(ImageMixup(alpha, same))(imgs[:1], np.zeros_like(imgs[:1]), idx[:1])
    assert np.array_equal(one, R.image_mixup(imgs[:1], idx[:1], alpha, same))


def test_image_mixup_other_host_dtypes():
    rng = np.random.default_rng(6)
    idx = np.arange(5, dtype=np.uint64) + 3
    for dt in (np.float32, np.float64, np.float16, np.int16):
        x = (rng.standard_normal((5, 4, 3)) * 100).astype(dt)
        got = _code(ImageMixup(0.5, False))(x, np.zeros_like(x), idx)
        assert got.dtype == dt and np.array_equal(got, R.image_mixup(x, idx, 0.5, False)), dt
    t = ch.from_numpy((rng.standard_normal((5, 4, 3)) * 100).astype(np.float32))
    got = _code(ImageMixup(0.5, True))(t, ch.zeros_like(t), idx)
    assert isinstance(got, ch.Tensor) and np.array_equal(got.numpy(), R.image_mixup(t.numpy(), idx, 0.5, True))


def test_one_hot_on_host_tensors():
    labels3 = ch.tensor([[1, 2, 0.25], [3, 3, 0.4], [0, 9, 1.0], [9, 0, 0.0]], dtype=ch.float32)
    keep = labels3.clone()
    out = _code(MixupToOneHot(10))(labels3, ch.full((6, 10), 7.0))
    assert tuple(out.shape) == (4, 10) and out.dtype == ch.float32
    assert np.array_equal(out.numpy(), R.one_hot(keep.numpy(), 10))
    assert ch.equal(labels3, keep)                          # the input's third column is not changed
    assert out[1].sum().item() == np.float32(1) - np.float32(0.4)   # a == b: the second store wins
    d = _code(MixupToOneHot(10))(labels3.double(), ch.zeros((4, 10), dtype=ch.float64))
    assert d.dtype == ch.float64 and d[0, 2].item() == 1 - float(np.float32(0.25))
    for bad in ([1, 10, 0.5], [-1, 2, 0.5], [11, 2, 0.5]):
        dst = ch.full((4, 10), 7.0)
        with pytest.raises(IndexError):
            _code(MixupToOneHot(10))(ch.tensor([[1, 2, 0.5], bad], dtype=ch.float32), dst)
        assert (dst == 7.0).all()                           # nothing was written


def test_constructor_errors():
    for cls in (ImageMixup, LabelMixup):
        for alpha in (0, -1.0, float('nan'), float('inf'), 'x', None, True):
            with pytest.raises(ValueError):
                cls(alpha, True)
        for same in (1, 0, None, 'yes'):
            with pytest.raises(ValueError):
                cls(0.5, same)
        assert cls(0.5, False).same_lambda is False and cls(2, True).alpha == 2
    for nc in (0, -3, 2.5, '10', None, True):
        with pytest.raises(ValueError):
            MixupToOneHot(nc)
    assert MixupToOneHot(np.int64(5)).num_classes == 5


def test_dropin_imports():
    from ffcv.transforms import ImageMixup as A, LabelMixup as B, MixupToOneHot as C
    import ffcv.transforms.mixup as m
    assert A is ImageMixup and B is LabelMixup and C is MixupToOneHot
    assert m.ImageMixup is ImageMixup


def test_declarations():
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    host = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(32, 32, 3))
    st, q = ImageMixup(0.5, True).declare_state_and_memory(host)
    assert st == host and q == AllocationQuery((32, 32, 3), np.dtype('u1'), None)    # its own buffer
    st, q = LabelMixup(0.5, True).declare_state_and_memory(
        State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('<i8'), shape=(1,)))
    assert st.shape == (3,) and st.dtype == np.float32 and q == AllocationQuery((3,), np.dtype(np.float32))
    dev = ch.device('cuda:0')
    for dt in (ch.float16, ch.int16, ch.float64):
        with pytest.raises(TypeError, match='NormalizeImage'):
            ImageMixup(0.5, True).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32)))
    for dt in (ch.uint8, ch.float32):
        st, q = ImageMixup(0.5, True).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=dt, shape=(32, 32, 3)))
        assert q == AllocationQuery((32, 32, 3), dt, dev)
    st, q = MixupToOneHot(10).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.float32, shape=(3,)))
    assert st.shape == (10,) and q == AllocationQuery((10,), ch.float32, dev)
    with pytest.raises(TypeError):
        MixupToOneHot(10).declare_state_and_memory(State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype(np.float32), shape=(3,)))
    assert ImageMixup.per_batch and LabelMixup.per_batch and not ImageMixup.per_sample
    assert MixupToOneHot.per_sample and Operation.per_batch is False


# ------------------------------------------------------ graph and Loader --
class _UserOp(Operation):
    def generate_code(self):
        return lambda x, dst: x

    def declare_state_and_memory(self, previous_state):
        return previous_state, None


@pytest.fixture(scope='module')
def beton():
    fn = os.path.join(tempfile.mkdtemp(), 'mix_raw.beton')
    write(fn, NaturalDS(40, hw=(32, 32), seed=3), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn


ALPHA = 0.5


def _mix_pipelines(same, extra=()):
    return {'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), ImageMixup(ALPHA, same)] + list(extra),
            'label': [IntDecoder(), LabelMixup(ALPHA, same), ToTensor(), MixupToOneHot(10)]}


def _epoch(loader):
    ims, labs = [], []
    for im, lab in loader:
        ims.append(np.array(im.numpy() if isinstance(im, ch.Tensor) else im))
        labs.append(np.array(lab.numpy() if isinstance(lab, ch.Tensor) else lab))
    return ims, labs


def test_graph_keeps_launch_groups(beton):
    kw = dict(batch_size=16, device='cpu', seed=1, drop_last=False)
    assert Loader(beton, pipelines=_mix_pipelines(True), **kw).graph.groupable()
    assert not Loader(beton, pipelines=_mix_pipelines(True, extra=[_UserOp()]), **kw).graph.groupable()


@pytest.mark.parametrize('same', [False, True])
def test_cpu_loader_matches_reference_per_batch(beton, same):
    kw = dict(batch_size=16, device='cpu', seed=23, drop_last=False)
    base = Loader(beton, pipelines={'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5)],
                                    'label': [IntDecoder()]}, **kw)
    mixed = Loader(beton, pipelines=_mix_pipelines(same), **kw)
    grouped = Loader(beton, pipelines=_mix_pipelines(same), batches_per_launch=3, **kw)
    first = None
    for epoch in range(2):
        b_im, b_lab = _epoch(base)
        m_im, m_lab = _epoch(mixed)
        g_im, g_lab = _epoch(grouped)
        assert [len(x) for x in b_im] == [16, 16, 8] == [len(x) for x in m_im] == [len(x) for x in g_im]
        for k in range(3):
            idx = np.arange(16 * k, 16 * k + len(b_im[k]))
            want_im = R.image_mixup(b_im[k], idx, ALPHA, same)
            want_lab = R.one_hot(R.label_mixup(b_lab[k], idx, ALPHA, same), 10)
            assert np.array_equal(m_im[k], want_im) and np.array_equal(g_im[k], want_im), (epoch, k)
            assert m_lab[k].dtype == np.float32 and np.array_equal(m_lab[k], want_lab), (epoch, k)
            assert np.array_equal(g_lab[k], want_lab), (epoch, k)
            assert not np.array_equal(want_im, b_im[k])
        if first is None:
            first = b_im
    assert not np.array_equal(np.concatenate(first), np.concatenate(b_im))   # the flips differ between epochs
