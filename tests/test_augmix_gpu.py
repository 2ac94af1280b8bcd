"""AugMix on the MI355X: device draws against the host twin as bits; the fused
kernel on hand-written arrays against the statement (tests/augmix_ref.mix of
the chains' results, each chain the rounds of host twins that test_augmix.py
ties to the numpy statement); the mix kernel alone; dispatch; Loaders."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder, RandomResizedCropRGBImageDecoder
from ffcv_amd.transforms import ToTensor, ToDevice, RandomHorizontalFlip, AugMix
from ffcv_amd.transforms.auto_augment import augmix_table
from tests import affine_ref as AR
from tests import augmix_ref as AM
from tests import auto_augment_ref as R
from tests.test_augmix import SEED, host_chains
from tests.test_randaugment_gpu import FILL, hand_arrays, images, run_device_op, _beton, _to_device, tmpdir_m  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.mark.parametrize('width,depth,all_ops,alpha', ((1, -1, True, 0.5), (3, 2, False, 1.0), (4, -1, True, 2.5)))
def test_device_draws_equal_host_draws(width, depth, all_ops, alpha):
    ids = np.arange(2048, dtype=np.uint64)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    table = augmix_table(33, 47)
    arrays = L.augmix_arrays(width)
    for seed, epoch in ((SEED, 0), (2 ** 63 + 5, 7)):
        dev = {name: ch.full(shape(len(ids)), 77, dtype=getattr(ch, np.dtype(dt).name), device=DEV)
               for name, dt, shape in arrays}
        status = ch.full((len(ids),), -1, dtype=ch.int32, device=DEV)
        L.augmix_draw_batch(d_ids, seed, epoch, 7, width, depth, alpha, all_ops, ch.from_numpy(table).to(DEV), 33, 47,
                            dev, status)
        assert (status == 0).all()
        host = L.augmix_draw_batch_host(ids, seed, epoch, 7, width, depth, alpha, all_ops, table, 33, 47)
        for name, dt, _ in arrays:
            got = dev[name].cpu().numpy()
            assert got.dtype == np.dtype(dt) and got.shape == host[name].shape
            assert np.array_equal(got.view(np.uint8), host[name].view(np.uint8)), (name, seed, epoch)


def fused_in_guards(imgs, d, width, mode, fill):
    """ffcv_augmix_batch with src and dst at odd byte offsets inside 0xA5-guarded buffers."""
    n = imgs.size
    src_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    dst_buf = ch.full((n + 48,), 0xA5, dtype=ch.uint8, device=DEV)
    sl, dl = 3, 21
    src = src_buf[sl:sl + n].view(imgs.shape)
    src.copy_(ch.from_numpy(imgs))
    L.augmix_batch(src, dst_buf[dl:dl + n].view(imgs.shape), width, mode, fill, _to_device(d))
    o = dst_buf.cpu().numpy()
    assert np.array_equal(src_buf.cpu().numpy()[sl:sl + n], imgs.ravel())
    assert (o[:dl] == 0xA5).all() and (o[dl + n:] == 0xA5).all()
    return o[dl:dl + n].reshape(imgs.shape)


def statement(imgs, d, width, mode, fill):
    results = host_chains(imgs, d, width, mode, fill)
    return np.stack([AM.mix(imgs[k], [r[k] for r in results], d['weights'][:, k]) for k in range(len(imgs))])


def hand_chains(B, width, H, W):
    """Image k's chain i runs 1 + (i + k) % 3 steps; slots beyond a chain's depth are Identity."""
    depth = np.array([[1 + (i + k) % 3 for k in range(B)] for i in range(width)], np.uint8)
    seqs = np.zeros((B, 3 * width), np.int64)
    for k in range(B):
        for i in range(width):
            for j in range(depth[i, k]):
                seqs[k, 3 * i + j] = 1 + (k + 5 * i + 3 * j) % 13
    negs = (np.arange(B)[:, None] + np.arange(3 * width)[None, :]) % 2 == 1
    d = hand_arrays(seqs, negs, H, W)
    rng = np.random.default_rng(B + width)
    w = rng.gamma(1.0, size=(width + 1, B))
    d['depth'], d['weights'] = depth, (w / w.sum(axis=0)).astype(np.float32)
    return d, seqs


@pytest.mark.parametrize('width,mode', ((1, AR.NEAREST), (3, AR.BILINEAR), (4, AR.NEAREST)), ids=('w1', 'w3', 'w4'))
@pytest.mark.parametrize('hw', ((1, 1), (2, 2), (7, 5), (32, 32), (64, 64)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_fused_kernel_matches_the_statement(hw, width, mode):
    H, W = hw
    assert 9 * H * W <= L.augmix_lds_bytes()
    B = 39
    d, seqs = hand_chains(B, width, H, W)
    first, later = set(seqs[:, ::3].ravel()), set(seqs[:, [j for j in range(3 * width) if j % 3]].ravel())
    assert first >= set(range(1, 14)) and later >= set(range(1, 14))
    imgs = images(B, H, W, 7 + H)
    want = statement(imgs, d, width, mode, FILL)
    got = fused_in_guards(imgs, d, width, mode, FILL)
    bad = [(k, tuple(seqs[k])) for k in range(B) if not np.array_equal(got[k], want[k])]
    assert not bad, (hw, width, bad[:6])


def test_fused_kernel_rounds_half_to_even_and_caps():
    """One chain of one step.  Posterize to 7 bits (y = x & 254) and Solarize at
    threshold 0 (y = 255 - x) under (0.5, 0.5): x = 1, 3 with 0, 2 give 0.5, 2.5
    (down to even, where half-up differs), any x gives 127.5 under the inversion
    (up to even, where truncation differs).  (0.75, 0.75) on an unchanged 255: the cap."""
    H, W = 4, 3
    seqs = np.array([[R.POSTERIZE, 0, 0], [R.SOLARIZE, 0, 0], [R.IDENTITY, 0, 0], [R.POSTERIZE, 0, 0],
                     [R.SOLARIZE, 0, 0]])
    d = hand_arrays(seqs, np.zeros(seqs.shape, bool), H, W)
    d['tone_bits'][0, [0, 3]] = 7
    d['cj_ratio'][0, 3, [1, 4]] = 0.0
    d['depth'] = np.ones((1, 5), np.uint8)
    d['weights'] = np.array([[0.5, 0.5, 0.75, 1.0, 0.0], [0.5, 0.5, 0.75, 0.0, 1.0]], np.float32)
    imgs = np.tile(np.arange(36, dtype=np.uint8).reshape(1, H, W, 3), (5, 1, 1, 1))
    imgs[2] = 255
    got = fused_in_guards(imgs, d, 1, AR.NEAREST, FILL)
    x = imgs[0].astype(np.int64)
    assert np.array_equal(got[0], x & 254)                         # odd x: y + 0.5 with y = x - 1 even, down to y
    assert (got[1] == 128).all() and (got[2] == 255).all()
    assert np.array_equal(got[3], imgs[3]) and np.array_equal(got[4], 255 - imgs[4])
    assert np.array_equal(got, statement(imgs, d, 1, AR.NEAREST, FILL))


@pytest.mark.parametrize('hw', ((1, 1), (97, 131)), ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('width', (1, 4))
def test_mix_kernel_alone(hw, width):
    H, W = hw
    B = 5
    rng = np.random.default_rng(H + width)
    n = B * H * W * 3
    host = [rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) for _ in range(width + 1)]
    host[0][0] = 255
    w = rng.gamma(1.0, size=(width + 1, B))
    w = (w / w.sum(axis=0)).astype(np.float32)
    w[:, 0] = 0.6                                                  # the cap: 255 * 0.6 * 2 or more
    bufs = [ch.full((n + 64,), 0xA5, dtype=ch.uint8, device=DEV) for _ in range(width + 2)]
    offs = [1 + 2 * i for i in range(width + 1)] + [19]
    views = [b[o:o + n].view(B, H, W, 3) for b, o in zip(bufs, offs)]
    for v, a in zip(views, host):
        v.copy_(ch.from_numpy(a))
    L.augmix_mix_batch(views[0], views[1:-1], ch.from_numpy(w).to(DEV), views[-1])
    o = bufs[-1].cpu().numpy()
    assert (o[:19] == 0xA5).all() and (o[19 + n:] == 0xA5).all()
    want = np.stack([AM.mix(host[0][k], [r[k] for r in host[1:]], w[:, k]) for k in range(B)])
    assert np.array_equal(o[19:19 + n].reshape(B, H, W, 3), want) and (want[0] == 255).any()
    assert np.array_equal(L.augmix_mix_batch_host(host[0], host[1:], w, np.empty_like(host[0]), 3), want)


def operation_expected(imgs, ids, seed, epoch, op, mode):
    H, W = imgs.shape[1:3]
    return statement(imgs, L.augmix_draw_batch_host(ids, seed, epoch, op.severity, op.mixture_width, op.chain_depth,
                                                    op.alpha, op.all_ops, augmix_table(H, W), H, W),
                     op.mixture_width, mode, FILL)


def test_dispatch_at_the_edge_of_the_fused_regime(monkeypatch):
    bound = L.augmix_lds_bytes()
    assert 9 * 64 * 64 <= bound < 9 * 64 * 65
    ids = np.arange(20, dtype=np.uint64) + 300
    calls = []
    for name in ('augmix_batch', 'augmix_mix_batch'):
        monkeypatch.setattr(L, name, lambda *a, _f=getattr(L, name), _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    for (H, W), fused in (((64, 64), True), ((64, 65), False)):
        del calls[:]
        imgs = images(len(ids), H, W, 19)
        op = AugMix(severity=6, chain_depth=2, interpolation='bilinear', fill=FILL)
        got, _ = run_device_op(op, imgs, ids, SEED, 2, monkeypatch)
        assert np.array_equal(got, operation_expected(imgs, ids, SEED, 2, op, AR.BILINEAR)), (H, W)
        assert calls == (['augmix_batch'] if fused else ['augmix_mix_batch'])


def test_rounds_path_matches_the_statement(monkeypatch):
    H, W = 80, 80
    assert 9 * H * W > L.augmix_lds_bytes()
    ids = np.arange(40, dtype=np.uint64) + 100
    imgs = images(len(ids), H, W, 5)
    op = AugMix(severity=10, mixture_width=3, fill=FILL)
    got, calls = run_device_op(op, imgs, ids, SEED, 1, monkeypatch)
    want = operation_expected(imgs, ids, SEED, 1, op, AR.NEAREST)
    assert len(calls) == 5 * 3 * 3 and not (got == 0xA5).all(axis=(1, 2, 3)).any()
    bad = [k for k in range(len(ids)) if not np.array_equal(got[k], want[k])]
    assert not bad and sum(not np.array_equal(want[k], imgs[k]) for k in range(len(ids))) > 30, bad[:8]


@pytest.mark.parametrize('case', ['raw32', 'jpeg80'])
def test_device_loader_matches_cpu_loader(tmpdir_m, case):  # noqa: F811
    """The fused launch at 32 x 32, the rounds at 80 x 80; the launch group is the plain pipeline's."""
    if case == 'raw32':
        fn, decoder = _beton(tmpdir_m, 'am_raw.beton', 'raw', 40, (32, 32), 4), SimpleRGBImageDecoder
    else:
        fn = _beton(tmpdir_m, 'am_jpg.beton', 'jpg', 40, (96, 120), 5)
        decoder = lambda: RandomResizedCropRGBImageDecoder((80, 80))  # noqa: E731
    chain = lambda: [decoder(), AugMix(), RandomHorizontalFlip()]  # noqa: E731
    cpu = Loader(fn, batch_size=16, device='cpu', seed=17, drop_last=False, pipelines={'image': chain() + [ToTensor()]})
    want = [np.concatenate([im.numpy().copy() for im, _ in cpu]) for _ in range(2)]

    def dev(ops, **kw):
        return Loader(fn, batch_size=16, seed=17, drop_last=False, pipelines={
            'image': ops + [ToTensor(), ToDevice(DEV)], 'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)
    for kw in (dict(batches_per_launch=1), dict()):
        loader, plain = dev(chain(), **kw), dev([decoder(), RandomHorizontalFlip()], **kw)
        assert loader.graph.groupable()
        assert launch_group(loader, len(loader)) == launch_group(plain, len(plain))
        for want_u8 in want:
            got = np.concatenate([im.cpu().numpy() for im, _ in loader])
            bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
            assert not bad, (case, kw, bad[:8])
