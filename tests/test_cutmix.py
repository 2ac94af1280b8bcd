"""ImageCutMix / LabelCutMix and the Mixup/CutMix switch on the CPU: the host
twin of the CutMix kernel (ffcv_cutmix_batch_host) bit for bit against the
numpy statement (tests/cutmix_ref.py) over shapes, element sizes, layouts,
batch segmentations and hand-made boxes; the operations on host arrays and
tensors; the constructors, declarations, drop-in imports and launch groups;
and CPU Loaders with one and with three batches per launch."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.pipeline.operation import Operation
from ffcv_amd.transforms import (ToTensor, RandomHorizontalFlip, MixupToOneHot, ImageCutMix, LabelCutMix,
                                 ImageMixupCutMix, LabelMixupCutMix)
from tests.helpers import NaturalDS, write
from tests import cutmix_ref as R
from tests.mixup_ref import SEGMENT_CASES, one_hot


@pytest.fixture(scope='module', autouse=True)
def built(hip_lib):
    return hip_lib


def _code(op):
    return op.generate_code()


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------ host twin --
@pytest.mark.parametrize('itemsize', R.ITEMSIZES)
def test_shapes_segments_and_forms_host(itemsize):
    rng = np.random.default_rng(17 + itemsize)
    for H, W in R.SIZES:
        for layout, C in R.FORMS:
            for n, bs in SEGMENT_CASES:
                if n == 67 and H * W > 64:
                    continue
                for same in (False, True):
                    x = R.random_images(rng, n, H, W, layout, C, itemsize)
                    boxes = R.random_boxes(rng, -(-n // bs) if same else n, H, W)
                    got = L.cutmix_batch_host(x, np.full_like(x, 0xA5), boxes, bs, same, layout, nthreads=2)
                    want = R.from_hwc(R.cut_segments(R.as_hwc(x, layout), boxes, bs, same), layout)
                    assert _same_bytes(got, want), (H, W, layout, C, n, bs, same)


@pytest.mark.parametrize('layout,C', R.FORMS)
def test_hand_made_boxes_host(layout, C):
    """Empty, full, corner pixels, a full row and column, out-of-range boxes,
    and x1 swept over 0..W at W = 47: box edges at every byte phase."""
    rng = np.random.default_rng(23)
    H, W = 33, 47
    boxes = R.hand_boxes(H, W)
    n = len(boxes)
    x = R.random_images(rng, n, H, W, layout, C, 1)
    hwc = R.as_hwc(x, layout)
    got = L.cutmix_batch_host(x, np.full_like(x, 0xA5), boxes, 5, False, layout, nthreads=3)
    want = R.cut_segments(hwc, boxes, 5, False)
    assert _same_bytes(got, R.from_hwc(want, layout))
    g = R.as_hwc(got, layout)
    assert np.array_equal(g[0], hwc[0]) and np.array_equal(g[1], hwc[1])         # empty boxes: the identity
    assert np.array_equal(g[2], hwc[1])                                           # the full image: the neighbour
    assert np.array_equal(g[3, 0, 0], hwc[2, 0, 0]) and np.array_equal(g[3, 0, 1:], hwc[3, 0, 1:])
    assert np.array_equal(g[9], hwc[8]) and np.array_equal(g[10], hwc[14])        # clamped to the full image
    assert np.array_equal(g[11], hwc[11])                                         # clamped to nothing
    # the sweep with two bytes per pixel too, and one box for the whole batch
    x2 = R.random_images(rng, 4, H, W, layout, C, 2)
    for b in boxes[12::5]:
        got = L.cutmix_batch_host(x2, np.zeros_like(x2), b, 4, True, layout)
        assert _same_bytes(got, R.from_hwc(R.cut_segments(R.as_hwc(x2, layout), b[None], 4, True), layout)), b


def test_host_abi_rejections():
    lib = L.lib()
    a = np.arange(128, dtype=np.uint8).reshape(4, 4, 4, 2) + 100
    o = np.full((4, 4, 4, 2), 7, np.uint8)
    bx = np.tile(np.array([0, 0, 4, 4], np.int32), (4, 1))

    def call(inp=a.ctypes.data, out=o.ctypes.data, n=4, p=1, h=4, w=4, pb=2, bs=4, b=bx.ctypes.data):
        return lib.ffcv_cutmix_batch_host(inp, out, n, p, h, w, pb, bs, b, 0, 1)
    for kw in (dict(inp=None), dict(out=None), dict(b=None), dict(n=0), dict(n=-1), dict(p=0), dict(h=0), dict(w=-2),
               dict(bs=0), dict(pb=0), dict(pb=65), dict(pb=-1), dict(h=2**31 - 1, w=2**31 - 1, pb=64),
               dict(p=2**31 - 1, h=2**31 - 1), dict(n=2**62, h=1024, w=1024), dict(out=a.ctypes.data),
               dict(out=a.ctypes.data + 31), dict(out=a.ctypes.data - 31)):
        assert call(**kw) == -1 and b'ffcv_cutmix_batch_host' in lib.ffcv_last_error(), kw
    assert (o == 7).all()
    assert call() == 0
    assert np.array_equal(o, np.roll(a, 1, 0))
    with pytest.raises(TypeError):
        L.cutmix_batch_host(a, o.astype(np.int16), bx, 4, False)
    with pytest.raises(TypeError):
        L.cutmix_batch_host(a[:, ::2], o[:, ::2], bx, 4, False)
    with pytest.raises(TypeError):
        L.cutmix_batch_host(a, o, bx[:3], 4, False)
    with pytest.raises(ValueError):
        L.cutmix_batch_host(a, o, bx, 4, False, layout='nchw')


# ------------------------------------------------------- the operations --
def test_scalar_draws_equal_size_one_draws():
    """same_lambda's scalar draws are the size-1 array draws (seeds 0..49)."""
    for seed in range(50):
        a, la = R.draw_boxes(seed, 0.7, True, 1, 32, 48)
        b, lb = R.draw_boxes(seed, 0.7, False, 1, 32, 48)
        assert np.array_equal(a, b) and np.array_equal(la, lb)


def test_reference_boxes_cover_the_clipped_cases():
    """At 32x32 with alpha 0.5 and 1 the Loader test's batches (last indices
    15, 31, 39) draw boxes clipped at all four edges, none empty or full."""
    boxes = np.concatenate([R.draw_boxes(last, alpha, False, n, 32, 32)[0]
                            for alpha in (0.5, 1.0) for last, n in ((15, 16), (31, 16), (39, 8))])
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    assert (boxes[:, 0] == 0).any() and (boxes[:, 1] == 0).any() and (boxes[:, 2] == 32).any() and \
        (boxes[:, 3] == 32).any()
    assert area.min() == 4 and area.max() == 784


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('alpha', [0.2, 1.0, 2.0])
def test_ops_on_numpy_arrays(alpha, same):
    rng = np.random.default_rng(5)
    idx = np.array([9, 4, 77, 1, 30, 12, 5], np.uint64)
    imgs = rng.integers(0, 256, (7, 9, 11, 3), dtype=np.uint8)
    labels = rng.integers(0, 10, (7, 1)).astype(np.int64)
    got = _code(ImageCutMix(alpha, same))(imgs, np.zeros_like(imgs), idx)
    assert np.array_equal(got, R.image_cutmix(imgs, idx, alpha, same))
    lab = _code(LabelCutMix(alpha, same, (9, 11)))(labels, np.zeros((7, 3), np.float32), idx)
    assert lab.dtype == np.float32 and np.array_equal(lab, R.label_cutmix(labels, idx, alpha, same, (9, 11)))
    # the image and the label operation draw the same boxes
    boxes, lam_adj = R.draw_boxes(idx[-1], alpha, same, 7, 9, 11)
    assert np.array_equal(lab[:, 2], lam_adj.astype(np.float32))
    assert lab[0, 1] == labels[6, 0] and lab[1, 1] == labels[0, 0]
    for i in range(7):
        y1, x1, y2, x2 = boxes[i]
        assert np.array_equal(got[i, y1:y2, x1:x2], imgs[i - 1, y1:y2, x1:x2])
        changed = (got[i] != imgs[i]).any(-1)
        assert not changed[:y1].any() and not changed[y2:].any() and not changed[:, :x1].any() and \
            not changed[:, x2:].any()
    # B = 1 pastes a sample into itself
    one = _code(ImageCutMix(alpha, same))(imgs[:1], np.zeros_like(imgs[:1]), idx[:1])
    assert np.array_equal(one, imgs[:1])
    lab1 = _code(LabelCutMix(alpha, same, (9, 11)))(labels[:1], np.zeros((1, 3), np.float32), idx[:1])
    assert np.array_equal(lab1, R.label_cutmix(labels[:1], idx[:1], alpha, same, (9, 11)))


def test_image_cutmix_host_dtypes_tensors_and_layouts():
    rng = np.random.default_rng(6)
    idx = np.arange(5, dtype=np.uint64) + 3
    for dt in (np.float32, np.float64, np.float16, np.int16, np.uint8):
        x = (rng.standard_normal((5, 6, 7, 3)) * 100).astype(dt)
        got = _code(ImageCutMix(0.5, False))(x, np.zeros_like(x), idx)
        assert _same_bytes(got, R.image_cutmix(x, idx, 0.5, False)), dt
    f = (rng.standard_normal((5, 6, 7, 3)) * 100).astype(np.float32)
    want = R.image_cutmix(f, idx, 0.5, True)
    t = ch.from_numpy(f)
    got = _code(ImageCutMix(0.5, True))(t, ch.zeros((8, 6, 7, 3)), idx)
    assert isinstance(got, ch.Tensor) and np.array_equal(got.numpy(), want)
    got = _code(ImageCutMix(0.5, True, layout='hwc'))(t, ch.zeros((8, 6, 7, 3)), idx)
    assert np.array_equal(got.numpy(), want)
    # the NCHW view of channels-last storage, and its destination as the Loader allocates it
    got = _code(ImageCutMix(0.5, True))(t.permute(0, 3, 1, 2), ch.zeros((8, 3, 6, 7)), idx)
    assert tuple(got.shape) == (5, 3, 6, 7) and got.is_contiguous(memory_format=ch.channels_last)
    assert np.array_equal(got.permute(0, 2, 3, 1).numpy(), want)
    # a contiguous (B, C, H, W)
    planar = t.permute(0, 3, 1, 2).contiguous()
    got = _code(ImageCutMix(0.5, True, layout='chw'))(planar, ch.zeros((8, 3, 6, 7)), idx)
    assert got.is_contiguous() and np.array_equal(got.permute(0, 2, 3, 1).numpy(), want)
    with pytest.raises(TypeError):
        _code(ImageCutMix(0.5, True, layout='hwc'))(t.permute(0, 3, 1, 2), ch.zeros((8, 3, 6, 7)), idx)


def test_one_hot_on_label_cutmix_rows():
    idx = np.arange(6, dtype=np.uint64) + 20
    labels = np.array([[1], [2], [2], [0], [9], [4]], np.int64)
    rows = _code(LabelCutMix(1.0, False, (32, 32)))(labels, np.zeros((6, 3), np.float32), idx)
    out = _code(MixupToOneHot(10))(ch.from_numpy(rows.copy()), ch.full((6, 10), 7.0))
    assert np.array_equal(out.numpy(), one_hot(R.label_cutmix(labels, idx, 1.0, False, (32, 32)), 10))
    assert out[0, 1].item() == rows[0, 2] and out[0, 4].item() == np.float32(1) - rows[0, 2]


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('prob', [0.0, 1.0, 0.5])
def test_switch_takes_both_branches(prob, same):
    rng = np.random.default_rng(8)
    picks = []
    for dt in (np.uint8, np.float32, np.float16):
        for last in range(100, 112):
            idx = np.arange(last - 5, last + 1, dtype=np.uint64)
            imgs = (rng.integers(0, 256, (6, 8, 9, 3))).astype(dt)
            labels = rng.integers(0, 10, (6, 1)).astype(np.int64)
            want_im, want_rows, cut = R.switch_batch(imgs, labels, last, 0.4, 1.0, prob, same)
            got = _code(ImageMixupCutMix(0.4, 1.0, prob, same))(imgs, np.zeros_like(imgs), idx)
            assert _same_bytes(got, want_im), (dt, last)
            rows = _code(LabelMixupCutMix(0.4, 1.0, prob, same, (8, 9)))(labels, np.zeros((6, 3), np.float32), idx)
            assert np.array_equal(rows, want_rows), (dt, last)
            picks.append(cut)
    assert (all(picks) if prob == 1.0 else not any(picks) if prob == 0.0 else (any(picks) and not all(picks)))
    # the leading draw shifts the stream against the stand-alone operations
    imgs = rng.integers(0, 256, (6, 8, 9, 3), dtype=np.uint8)
    idx = np.arange(6, dtype=np.uint64)
    alone = _code(ImageCutMix(1.0, same))(imgs, np.zeros_like(imgs), idx)
    switched = _code(ImageMixupCutMix(0.4, 1.0, 1.0, same))(imgs, np.zeros_like(imgs), idx)
    assert not np.array_equal(alone, switched)


def test_constructor_errors():
    makers = (lambda a, s: ImageCutMix(a, s), lambda a, s: LabelCutMix(a, s, (32, 32)),
              lambda a, s: ImageMixupCutMix(a, 1.0, 0.5, s), lambda a, s: ImageMixupCutMix(1.0, a, 0.5, s),
              lambda a, s: LabelMixupCutMix(a, 1.0, 0.5, s, (32, 32)),
              lambda a, s: LabelMixupCutMix(1.0, a, 0.5, s, (32, 32)))
    for make in makers:
        for alpha in (0, -1.0, float('nan'), float('inf'), 'x', None, True):
            with pytest.raises(ValueError):
                make(alpha, True)
        for same in (1, 0, None, 'yes'):
            with pytest.raises(ValueError):
                make(0.5, same)
        assert make(0.5, False).same_lambda is False
    for p in (-0.1, 1.5, float('nan'), 'x', None, True):
        with pytest.raises(ValueError):
            ImageMixupCutMix(1.0, 1.0, p, True)
        with pytest.raises(ValueError):
            LabelMixupCutMix(1.0, 1.0, p, True, (32, 32))
    assert ImageMixupCutMix(1.0, 1.0, 0, True).switch_prob == 0 and ImageMixupCutMix(1.0, 1.0, 1, True).switch_prob == 1
    for size in (None, 32, (32,), (32, 0), (32, -1), (32.0, 32), (32, 32, 3), (True, 32), '32'):
        with pytest.raises(ValueError):
            LabelCutMix(1.0, True, size)
        with pytest.raises(ValueError):
            LabelMixupCutMix(1.0, 1.0, 0.5, True, size)
    assert LabelCutMix(1.0, True, [np.int64(24), 32]).image_size == (24, 32)
    for layout in ('nchw', None, 0, 'HWC'):
        with pytest.raises(ValueError):
            ImageCutMix(1.0, True, layout=layout)
        with pytest.raises(ValueError):
            ImageMixupCutMix(1.0, 1.0, 0.5, True, layout=layout)
    assert [ImageCutMix(1.0, True, layout=l).layout for l in ('auto', 'hwc', 'chw')] == ['auto', 'hwc', 'chw']


def test_dropin_imports():
    from ffcv.transforms import ImageCutMix as A, LabelCutMix as B, ImageMixupCutMix as C, LabelMixupCutMix as D
    import ffcv.transforms.cutmix as m
    assert A is ImageCutMix and B is LabelCutMix and C is ImageMixupCutMix and D is LabelMixupCutMix
    assert m.ImageCutMix is ImageCutMix
    assert {'ffcv_cutmix_batch', 'ffcv_cutmix_batch_host'} <= set(L.EXPORTED_SYMBOLS)


def test_declarations():
    from ffcv_amd.pipeline.state import State
    from ffcv_amd.pipeline.allocation_query import AllocationQuery
    host = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('u1'), shape=(32, 32, 3))
    labels = State(jit_mode=True, device=ch.device('cpu'), dtype=np.dtype('<i8'), shape=(1,))
    dev = ch.device('cuda:0')
    for op in (ImageCutMix(0.5, True), ImageMixupCutMix(0.5, 1.0, 0.5, True)):
        st, q = op.declare_state_and_memory(host)
        assert st == host and q == AllocationQuery((32, 32, 3), np.dtype('u1'), None)    # its own buffer
    for op in (LabelCutMix(0.5, True, (32, 32)), LabelMixupCutMix(0.5, 1.0, 0.5, True, (32, 32))):
        st, q = op.declare_state_and_memory(labels)
        assert st.shape == (3,) and st.dtype == np.float32 and q == AllocationQuery((3,), np.dtype(np.float32))
        with pytest.raises(TypeError, match='label column'):
            op.declare_state_and_memory(State(jit_mode=False, device=dev, dtype=ch.int64, shape=(1,)))
    # CutMix moves bytes: every device dtype of 1, 2 or 4 bytes, so it may sit after NormalizeImage
    for dt in (ch.uint8, ch.float16, ch.bfloat16, ch.int16, ch.float32):
        st, q = ImageCutMix(0.5, True).declare_state_and_memory(
            State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32)))
        assert q == AllocationQuery((3, 32, 32), dt, dev)
    # NormalizeImage(float16) outside the fused launch declares its int16 bit pattern, as a numpy dtype
    st, q = ImageCutMix(0.5, True).declare_state_and_memory(
        State(jit_mode=False, device=dev, dtype=np.int16, shape=(3, 32, 32)))
    assert st.dtype == np.int16 and q == AllocationQuery((3, 32, 32), ch.int16, dev)
    for dt in (ch.float64, ch.int64, np.float64):
        with pytest.raises(TypeError, match='itemsize'):
            ImageCutMix(0.5, True).declare_state_and_memory(State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32)))
    # the switch keeps mixup's rule
    for dt in (ch.float16, ch.int16, ch.float64):
        with pytest.raises(TypeError, match='NormalizeImage'):
            ImageMixupCutMix(0.5, 1.0, 0.5, True).declare_state_and_memory(
                State(jit_mode=False, device=dev, dtype=dt, shape=(3, 32, 32)))
    for dt in (ch.uint8, ch.float32):
        st, q = ImageMixupCutMix(0.5, 1.0, 0.5, True).declare_state_and_memory(
            State(jit_mode=False, device=dev, dtype=dt, shape=(32, 32, 3)))
        assert q == AllocationQuery((32, 32, 3), dt, dev)
    for cls in (ImageCutMix, LabelCutMix, ImageMixupCutMix, LabelMixupCutMix):
        assert cls.per_batch and not cls.per_sample
    assert ImageCutMix.device_aware and ImageMixupCutMix.device_aware


# ------------------------------------------------------ graph and Loader --
class _UserOp(Operation):
    def generate_code(self):
        return lambda x, dst: x

    def declare_state_and_memory(self, previous_state):
        return previous_state, None


@pytest.fixture(scope='module')
def beton():
    fn = os.path.join(tempfile.mkdtemp(), 'cut_raw.beton')
    write(fn, NaturalDS(40, hw=(32, 32), seed=3), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    return fn


ALPHA = 0.5


def _cut_pipelines(same, extra=()):
    return {'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), ImageCutMix(ALPHA, same)] + list(extra),
            'label': [IntDecoder(), LabelCutMix(ALPHA, same, (32, 32)), ToTensor(), MixupToOneHot(10)]}


def _switch_pipelines(same):
    return {'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5), ImageMixupCutMix(ALPHA, 1.0, 0.5, same)],
            'label': [IntDecoder(), LabelMixupCutMix(ALPHA, 1.0, 0.5, same, (32, 32)), ToTensor(), MixupToOneHot(10)]}


def _epoch(loader):
    ims, labs = [], []
    for im, lab in loader:
        ims.append(np.array(im.numpy() if isinstance(im, ch.Tensor) else im))
        labs.append(np.array(lab.numpy() if isinstance(lab, ch.Tensor) else lab))
    return ims, labs


def test_graph_keeps_launch_groups(beton):
    kw = dict(batch_size=16, device='cpu', seed=1, drop_last=False)
    assert Loader(beton, pipelines=_cut_pipelines(True), **kw).graph.groupable()
    assert Loader(beton, pipelines=_switch_pipelines(False), **kw).graph.groupable()
    assert not Loader(beton, pipelines=_cut_pipelines(True, extra=[_UserOp()]), **kw).graph.groupable()


@pytest.mark.parametrize('same', [False, True])
@pytest.mark.parametrize('kind', ['cutmix', 'switch'])
def test_cpu_loader_matches_reference_per_batch(beton, kind, same):
    kw = dict(batch_size=16, device='cpu', seed=23, drop_last=False)
    pipes = _cut_pipelines if kind == 'cutmix' else _switch_pipelines
    base = Loader(beton, pipelines={'image': [SimpleRGBImageDecoder(), RandomHorizontalFlip(0.5)],
                                    'label': [IntDecoder()]}, **kw)
    mixed = Loader(beton, pipelines=pipes(same), **kw)
    grouped = Loader(beton, pipelines=pipes(same), batches_per_launch=3, **kw)
    first, picks = None, []
    for epoch in range(2):
        b_im, b_lab = _epoch(base)
        m_im, m_lab = _epoch(mixed)
        g_im, g_lab = _epoch(grouped)
        assert [len(x) for x in b_im] == [16, 16, 8] == [len(x) for x in m_im] == [len(x) for x in g_im]
        for k in range(3):
            idx = np.arange(16 * k, 16 * k + len(b_im[k]))
            if kind == 'cutmix':
                want_im = R.image_cutmix(b_im[k], idx, ALPHA, same)
                rows = R.label_cutmix(b_lab[k], idx, ALPHA, same, (32, 32))
            else:
                want_im, rows, cut = R.switch_batch(b_im[k], b_lab[k], idx[-1], ALPHA, 1.0, 0.5, same)
                picks.append(cut)
            want_lab = one_hot(rows, 10)
            assert np.array_equal(m_im[k], want_im) and np.array_equal(g_im[k], want_im), (epoch, k)
            assert m_lab[k].dtype == np.float32 and np.array_equal(m_lab[k], want_lab), (epoch, k)
            assert np.array_equal(g_lab[k], want_lab), (epoch, k)
            assert not np.array_equal(want_im, b_im[k])
        if first is None:
            first = b_im
    assert not np.array_equal(np.concatenate(first), np.concatenate(b_im))   # the flips differ between epochs
    assert kind == 'cutmix' or (any(picks) and not all(picks))              # the switch takes both branches
