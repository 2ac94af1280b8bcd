"""RandAugment on the MI355X: the device draws against the host twin in every
output array (compared as bits); the fused kernel on hand-written arrays -- all
196 ordered pairs of operations, single operations against TrivialAugmentWide's
launch sequence, triples across the buffer swaps -- against the rounds of host
twins, at an odd byte offset inside guarded buffers; the dispatch at the edge
of the fused regime and the rounds path beyond it; device Loaders against the
CPU Loader under the same seed."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.pipeline import runtime
from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, RandAugment
from ffcv_amd.transforms.auto_augment import randaugment_table
from tests import affine_ref as AR
from tests import auto_augment_ref as R
from tests import randaugment_ref as RA
from tests import tone_ref as TR
from tests.helpers import NaturalDS, write
from tests.test_randaugment import SEED

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)
FILL = (9, 200, 31)
FAMILIES = TR.FAMILIES + ('flat',)


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _torch_dtype(dt):
    return getattr(ch, np.dtype(dt).name)


def _to_device(d):
    return {name: ch.from_numpy(a).to(DEV) for name, a in d.items()}


# ---------------------------------------------------------------- draws --
@pytest.mark.parametrize('num_ops', (1, 3))
@pytest.mark.parametrize('nbins,mag,hw', ((31, 9, (32, 32)), (10, 7, (33, 47))))
def test_device_draws_equal_host_draws(num_ops, nbins, mag, hw):
    ids = np.arange(2048, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    table = randaugment_table(nbins, *hw)
    d_table = ch.from_numpy(table).to(DEV)
    arrays = L.randaugment_arrays(num_ops)
    for seed, epoch in ((SEED, 0), (2 ** 63 + 5, 7)):
        dev = {name: ch.full(shape(len(ids)), 77, dtype=_torch_dtype(dt), device=DEV) for name, dt, shape in arrays}
        status = ch.full((len(ids),), -1, dtype=ch.int32, device=DEV)
        L.randaugment_draw_batch(d_ids, seed, epoch, num_ops, nbins, mag, d_table, *hw, dev, status)
        assert (status == 0).all()
        host = L.randaugment_draw_batch_host(ids, seed, epoch, num_ops, nbins, mag, table, *hw)
        for name, dt, _ in arrays:
            got = dev[name].cpu().numpy()
            assert got.dtype == np.dtype(dt) and got.shape == host[name].shape
            assert np.array_equal(got.view(np.uint8), host[name].view(np.uint8)), (name, seed, epoch)
        assert len(set(host['op'].ravel())) == RA.NUM_OPS
    slots = RA.draw(SEED, 0, 5, num_ops)
    got = L.randaugment_draw_batch_host(ids[:8], SEED, 0, num_ops, nbins, mag, table, *hw)['op'][:, 5]
    assert list(got) == [op for op, _ in slots]


# ------------------------------------------- hand-written draw arrays --
_COEFS = {}


def hand_arrays(seqs, negs, H, W):
    """The draw's arrays for images that run the operations seqs[k] (negated
    where negs[k]) at fixed, non-trivial strengths, laid out as the draw lays
    them out."""
    seqs, negs = np.asarray(seqs), np.asarray(negs)
    B, S = seqs.shape
    d = {name: np.zeros(shape(B), dt) for name, dt, shape in L.randaugment_arrays(S)}
    d['cj_ratio'][:, :3] = 1.0
    d['cj_ratio'][:, 3] = 256.0
    d['tone_bits'][:] = 8
    d['sharp_apply'][:] = 2
    d['sharp_factor'][:] = 1.0
    d['aff_coef'][:] = AR.IDENTITY
    strength = {R.SHEAR_X: 14.0, R.SHEAR_Y: 11.0, R.TRANSLATE_X: float(max(1, W // 5)),
                R.TRANSLATE_Y: float(max(1, H // 7)), R.ROTATE: 27.0}
    for s in range(S):
        for k in range(B):
            op, sign = int(seqs[k, s]), -1.0 if negs[k, s] else 1.0
            d['op'][s, k] = op
            if R.SHEAR_X <= op <= R.ROTATE:
                key = (op, sign, H, W)
                if key not in _COEFS:
                    m = AR.matrix_f64(H=H, W=W, **R.affine_args(op, np.float64(sign * strength[op])))
                    assert AR.guard_holds(m)
                    _COEFS[key] = AR.quantise(m)
                d['aff_apply'][s, k] = 1
                d['aff_coef'][s, k] = _COEFS[key]
            elif op in (R.BRIGHTNESS, R.COLOR, R.CONTRAST):
                row = {R.BRIGHTNESS: 0, R.COLOR: 1, R.CONTRAST: 2}[op]
                d['cj_apply'][s, row, k] = 1
                d['cj_ratio'][s, row, k] = np.float64(1.0) + np.float64(sign * 0.6)
            elif op == R.SHARPNESS:
                d['sharp_apply'][s, k] = 1
                d['sharp_factor'][s, k] = np.float32(1.0 + sign * 0.7)
            elif op == R.POSTERIZE:
                d['tone_apply'][s, 0, k] = 1
                d['tone_bits'][s, k] = 3
            elif op == R.SOLARIZE:
                d['cj_apply'][s, 3, k] = 1
                d['cj_ratio'][s, 3, k] = 100.0
            elif op in (R.AUTOCONTRAST, R.EQUALIZE):
                d['tone_apply'][s, 1 + (op == R.EQUALIZE), k] = 1
    return d


def host_slot(cur, nxt, a, mode, fill):
    """One slot's five host twins, as TrivialAugmentWide runs them: in place on
    cur, then from cur into nxt."""
    L.color_jitter_batch_host(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
    L.color_jitter_batch_host(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
    L.tone_batch_bits_host(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'])
    L.affine_batch_host(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'], nthreads=4)
    L.sharpness_batch_host(cur, nxt, a['sharp_apply'], a['sharp_factor'], nthreads=4)


def host_rounds(imgs, d, mode, fill):
    """The expected bytes: the rounds of host twins, slot after slot."""
    cur = imgs.copy()
    for s in range(d['op'].shape[0]):
        nxt = np.full_like(cur, 0xA5)
        host_slot(cur, nxt, L.randaugment_slot(d, s), mode, fill)
        cur = nxt
    return cur


def images(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([TR.family(rng, FAMILIES[k % len(FAMILIES)], H, W) for k in range(B)])


def fused_in_guards(imgs, d, mode, fill):
    """ffcv_randaugment_batch with src and dst at odd byte offsets inside
    0xA5-guarded buffers: the result, after checking the guards and src."""
    n = imgs.size
    src_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    dst_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    sl, dl = 3, 21
    src = src_buf[sl:sl + n].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    L.randaugment_batch(src, dst_buf[dl:dl + n].view(imgs.shape), d['op'].shape[0], mode, fill, _to_device(d))
    s, o = src_buf.cpu().numpy(), dst_buf.cpu().numpy()
    assert (s[:sl] == 0xA5).all() and (s[sl + n:] == 0xA5).all() and np.array_equal(s[sl:sl + n], imgs.ravel())
    assert (o[:dl] == 0xA5).all() and (o[dl + n:] == 0xA5).all()
    return o[dl:dl + n].reshape(imgs.shape)


def assert_images_equal(got, want, seqs, what):
    bad = [(k, tuple(int(x) for x in seqs[k])) for k in range(len(got)) if not np.array_equal(got[k], want[k])]
    assert not bad, (what, bad[:8])


PAIRS = [(a, b) for a in range(RA.NUM_OPS) for b in range(RA.NUM_OPS)]


@pytest.mark.parametrize('mode', (AR.NEAREST, AR.BILINEAR), ids=('nearest', 'bilinear'))
@pytest.mark.parametrize('hw', ((1, 1), (2, 2), (7, 5), (32, 32), (64, 64)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_fused_pairs_match_host_rounds(hw, mode):
    """One image per ordered pair of operations, strengths of both signs."""
    H, W = hw
    assert 6 * H * W <= L.randaugment_lds_bytes()
    seqs = np.array(PAIRS)
    negs = np.array([[(a + b) % 2, (a // 2 + b) % 2] for a, b in PAIRS], bool)
    assert len(seqs) == 196 and {tuple(n) for n in negs} == {(False, False), (False, True), (True, False), (True, True)}
    imgs = images(196, H, W, 7 + H)
    d = hand_arrays(seqs, negs, H, W)
    want = host_rounds(imgs, d, mode, FILL)
    got = fused_in_guards(imgs, d, mode, FILL)
    assert_images_equal(got, want, seqs, (hw, mode))
    if H * W >= 35:
        changed = sum(not np.array_equal(want[k], imgs[k]) for k in range(196))
        assert changed > 150


@pytest.mark.parametrize('hw,mode', (((32, 32), AR.NEAREST), ((7, 5), AR.BILINEAR), ((64, 64), AR.BILINEAR)),
                         ids=('32x32-nearest', '7x5-bilinear', '64x64-bilinear'))
def test_fused_single_operation_matches_trivial_augment_launches(hw, mode):
    """num_ops = 1: the fused launch against TrivialAugmentWide's five device
    launches fed the same arrays (and the host twins)."""
    H, W = hw
    seqs = np.array([[op] for op in range(RA.NUM_OPS)] * 2)
    negs = np.array([[k >= RA.NUM_OPS] for k in range(len(seqs))], bool)
    B = len(seqs)
    imgs = images(B, H, W, 11)
    d = hand_arrays(seqs, negs, H, W)
    got = fused_in_guards(imgs, d, mode, FILL)
    assert_images_equal(got, host_rounds(imgs, d, mode, FILL), seqs, 'host')
    a = {name: t[0] for name, t in _to_device(d).items()}
    x = ch.from_numpy(imgs).to(DEV)
    out = ch.full_like(x, 0xA5)
    L.color_jitter_batch(x, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
    L.color_jitter_batch(x, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
    L.tone_batch_bits(x, TONE_STEPS, a['tone_apply'], a['tone_bits'])
    L.affine_batch(x, out, mode, FILL, a['aff_apply'], a['aff_coef'])
    L.sharpness_batch(x, out, a['sharp_apply'], a['sharp_factor'])
    assert_images_equal(got, out.cpu().numpy(), seqs, 'device launches')


TRIPLES = [(R.SHEAR_X, R.ROTATE, R.TRANSLATE_Y), (R.ROTATE, R.ROTATE, R.ROTATE), (R.SHARPNESS, R.ROTATE, R.EQUALIZE),
           (R.SHARPNESS, R.SHARPNESS, R.SHARPNESS), (R.TRANSLATE_X, R.SHARPNESS, R.SHEAR_Y),
           (R.EQUALIZE, R.SHARPNESS, R.AUTOCONTRAST), (R.CONTRAST, R.SHEAR_Y, R.CONTRAST),
           (R.IDENTITY, R.IDENTITY, R.IDENTITY), (R.IDENTITY, R.ROTATE, R.IDENTITY),
           (R.POSTERIZE, R.EQUALIZE, R.SOLARIZE), (R.COLOR, R.BRIGHTNESS, R.SHARPNESS),
           (R.AUTOCONTRAST, R.TRANSLATE_X, R.POSTERIZE)]


@pytest.mark.parametrize('hw,mode', (((32, 32), AR.BILINEAR), ((7, 5), AR.NEAREST), ((64, 64), AR.NEAREST)),
                         ids=('32x32-bilinear', '7x5-nearest', '64x64-nearest'))
def test_fused_triples_match_host_rounds(hw, mode):
    """num_ops = 3 on 48 triples: none, one, two and three swaps of the two
    image buffers, and table steps on either buffer."""
    H, W = hw
    rng = np.random.default_rng(23)
    seqs = np.array(TRIPLES + [tuple(rng.integers(0, RA.NUM_OPS, 3)) for _ in range(48 - len(TRIPLES))])
    negs = rng.integers(0, 2, seqs.shape).astype(bool)
    imgs = images(len(seqs), H, W, 13)
    d = hand_arrays(seqs, negs, H, W)
    got = fused_in_guards(imgs, d, mode, FILL)
    assert_images_equal(got, host_rounds(imgs, d, mode, FILL), seqs, (hw, mode))


def test_fused_refused_coefficients_give_fill():
    """Coefficients ffcv_affine_batch refuses (an image of fill) or whose
    footprint misses the image, followed by another operation."""
    H, W = 9, 6
    seqs = np.array([(R.ROTATE, R.BRIGHTNESS), (R.TRANSLATE_X, R.SHARPNESS), (R.ROTATE, R.IDENTITY)])
    negs = np.zeros(seqs.shape, bool)
    d = hand_arrays(seqs, negs, H, W)
    d['aff_coef'][0, 0] = (1 << 24, 0, 0, 0, 65536, 0)              # |m00| beyond FFCV_AFFINE_M_MAX
    d['aff_coef'][0, 1] = (65536, 0, 100 << 16, 0, 65536, 0)         # the footprint lies right of the image
    d['aff_coef'][0, 2] = (65536, 0, 0, 0, 65536, -(1 << 41))        # |b1| beyond FFCV_AFFINE_B_MAX
    imgs = images(3, H, W, 17)
    for mode in (AR.NEAREST, AR.BILINEAR):
        want = host_rounds(imgs, d, mode, FILL)
        assert (want[2] == np.array(FILL, np.uint8)).all()
        assert_images_equal(fused_in_guards(imgs, d, mode, FILL), want, seqs, mode)


# -------------------------------------------- the transform's device path --
class _Ctx:
    """What the operation's device code asks of a BatchContext."""

    def __init__(self, ids, seed, epoch):
        self.batch_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
        self.loader_seed, self.epoch, self.stream, self.batch_size = seed, epoch, None, len(ids)
        self._buffers = {}

    def device_buffer(self, key, n, dtype):
        buf = self._buffers.get(key)
        if buf is None or buf.numel() < n:
            buf = self._buffers[key] = ch.empty(int(n), dtype=dtype, device=DEV)
        return buf


def run_device_op(op, imgs, ids, seed, epoch, monkeypatch):
    """The operation's device code on a batch; returns (output, the names of
    the libffcv pixel entries it called, in order)."""
    calls = []
    for name in ('randaugment_batch', 'color_jitter_batch', 'tone_batch_bits', 'affine_batch', 'sharpness_batch'):
        def spy(*a, _f=getattr(L, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(L, name, spy)
    from ffcv_amd.pipeline.state import State
    H, W = imgs.shape[1:3]
    op.declare_state_and_memory(State(jit_mode=False, device=ch.device(DEV), dtype=ch.uint8, shape=(H, W, 3)))
    code = op.generate_code()
    x = ch.from_numpy(imgs).to(DEV)
    dst = ch.full_like(x, 0xA5)
    runtime.set_current(_Ctx(ids, seed, epoch))
    try:
        out = code(x, dst, ids)
    finally:
        runtime.set_current(None)
    return out.cpu().numpy(), calls


def host_expected(imgs, ids, seed, epoch, num_ops, nbins, mag, mode, fill):
    H, W = imgs.shape[1:3]
    d = L.randaugment_draw_batch_host(ids, seed, epoch, num_ops, nbins, mag, randaugment_table(nbins, H, W), H, W)
    return host_rounds(imgs, d, mode, fill), d


def test_dispatch_at_the_edge_of_the_fused_regime(monkeypatch):
    """64 x 64 is one fused launch, 64 x 65 the slots' launches; both equal
    the host twins.  The bound is libffcv's."""
    bound = L.randaugment_lds_bytes()
    assert 6 * 64 * 64 <= bound < 6 * 64 * 65
    ids = np.arange(28, dtype=np.uint64) + 300
    for (H, W), fused in (((64, 64), True), ((64, 65), False)):
        imgs = images(len(ids), H, W, 19)
        op = RandAugment(num_ops=2, interpolation='bilinear', fill=FILL)
        got, calls = run_device_op(op, imgs, ids, SEED, 2, monkeypatch)
        want, d = host_expected(imgs, ids, SEED, 2, 2, 31, 9, AR.BILINEAR, FILL)
        assert_images_equal(got, want, d['op'].T, (H, W))
        if fused:
            assert calls == ['randaugment_batch']
        else:
            assert calls == ['color_jitter_batch', 'color_jitter_batch', 'tone_batch_bits', 'affine_batch',
                             'sharpness_batch'] * 2


@pytest.mark.parametrize('hw,interpolation,num_ops', (((80, 80), 'nearest', 2), ((97, 131), 'bilinear', 2),
                                                      ((70, 66), 'bilinear', 3)),
                         ids=('80x80-nearest', '97x131-bilinear', '70x66-bilinear-3'))
def test_rounds_path_matches_host_twins(hw, interpolation, num_ops, monkeypatch):
    """The operation's launches on 56 images beyond the fused regime (every
    operation occurs), against the host twins of the same entries; the output
    starts as 0xA5 and every image of it is written."""
    H, W = hw
    assert 6 * H * W > L.randaugment_lds_bytes()
    ids = np.arange(56, dtype=np.uint64) + 100
    imgs = images(len(ids), H, W, 5)
    mode = AR.NEAREST if interpolation == 'nearest' else AR.BILINEAR
    op = RandAugment(num_ops=num_ops, interpolation=interpolation, fill=FILL)
    got, calls = run_device_op(op, imgs, ids, SEED, 1, monkeypatch)
    want, d = host_expected(imgs, ids, SEED, 1, num_ops, 31, 9, mode, FILL)
    assert len(set(d['op'].ravel())) == RA.NUM_OPS
    assert 'randaugment_batch' not in calls and len(calls) == 5 * num_ops
    assert not (want == 0xA5).all(axis=(1, 2, 3)).any()
    assert sum(not np.array_equal(want[k], imgs[k]) for k in range(len(ids))) > len(ids) // 2
    assert_images_equal(got, want, d['op'].T, hw)


# ------------------------------------------------------------- Loaders --
def _beton(tmpdir_m, name, mode, n, hw, seed):
    fn = os.path.join(tmpdir_m, name)
    if not os.path.exists(fn):
        write(fn, NaturalDS(n, hw=hw, seed=seed), {'image': RGBImageField(write_mode=mode), 'label': IntField()})
    return fn


@pytest.mark.parametrize('case', ['raw32', 'jpeg80'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case):
    """[decoder, RandAugment(), flip] on the device Loader (the fused launch at
    32 x 32, the rounds at 80 x 80), one batch per launch, with the Loader's own
    launch groups and with groups of 3, against the CPU Loader under the same
    seed, over two epochs; the launch group is what it is without the
    operation."""
    if case == 'raw32':
        fn = _beton(tmpdir_m, 'ra_raw.beton', 'raw', 40, (32, 32), 4)
        decoder = SimpleRGBImageDecoder
        assert 6 * 32 * 32 <= L.randaugment_lds_bytes()
    else:
        fn = _beton(tmpdir_m, 'ra_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = lambda: RandomResizedCropRGBImageDecoder((80, 80))  # noqa: E731
        assert 6 * 80 * 80 > L.randaugment_lds_bytes()
    seed = 17
    chain = lambda: [decoder(), RandAugment(), RandomHorizontalFlip()]  # noqa: E731
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': chain() + [ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]
    assert not np.array_equal(want[0], want[1])
    ops = {op for e in range(2) for k in range(40) for op, _ in RA.draw(seed, e, k, 2)}
    assert len(ops) >= 13          # the two epochs of 40 samples draw nearly every operation

    def dev(ops, **kw):
        return Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
            'image': ops + [ToTensor(), ToDevice(DEV)],
            'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict(), dict(batches_per_launch=3)):
        loader = dev(chain(), **kw)
        plain = dev([decoder(), RandomHorizontalFlip()], **kw)
        assert loader.graph.groupable()                     # launch groups are kept
        assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
        assert launch_group(loader, len(loader)) == launch_group(plain, len(plain)) == \
            (kw.get('batches_per_launch') or len(loader))
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            assert got.dtype == np.uint8 and got.shape == want_u8.shape
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (case, kw, bad[:8])
