"""AugMix on the host (no GPU): constructor, value table, the host twins of the
draws and of the mix and a CPU Loader against the numpy statement
(tests/augmix_ref.py), and the C entries' argument checks."""
import ctypes

import numpy as np
import pytest

from tests import affine_ref as AR
from tests import augmix_ref as AM
from tests import auto_augment_ref as R
from tests.helpers import NaturalDS, write

SEED = 29
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)


def host_chains(imgs, d, width, mode, fill):
    """Every chain's result batch: three rounds of the slots' host twins from a copy of imgs."""
    from ffcv_amd import libffcv as L
    results = []
    for i in range(width):
        cur = imgs.copy()
        for j in range(3):
            a, nxt = L.randaugment_slot(d, 3 * i + j), np.full_like(cur, 0xA5)
            L.color_jitter_batch_host(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
            L.color_jitter_batch_host(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
            L.tone_batch_bits_host(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'])
            L.affine_batch_host(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'], nthreads=4)
            L.sharpness_batch_host(cur, nxt, a['sharp_apply'], a['sharp_factor'], nthreads=4)
            cur = nxt
        results.append(cur)
    return results


def test_public_name_and_constructor_checks():
    import ffcv.transforms as FT
    import ffcv_amd.transforms as T
    cls = T.AugMix
    assert FT.AugMix is cls and 'AugMix' in T.__all__ and cls.per_sample and cls.op_id == AM.OP_CHAINS
    op = cls()
    assert (op.severity, op.mixture_width, op.chain_depth, op.alpha, op.all_ops) == (3, 3, -1, 1.0, True)
    assert cls(10, 4, 3, 100, False, 'bilinear', 7).alpha == 100.0 and cls(alpha=0.01).alpha == 0.01
    for arg, bads in (('severity', (0, 11, 3.0, True, None)), ('mixture_width', (0, 5, 2.0, True, 'x')),
                      ('chain_depth', (0, 4, -2, 1.0, True, None)), ('all_ops', (1, 0, None, 'yes')),
                      ('alpha', (0, 0.009, 101, float('nan'), float('inf'), True, None, 'x')),
                      ('interpolation', ('cubic', None, 1)), ('fill', ('x', (1, 2), float('nan'), None))):
        for bad in bads:
            with pytest.raises(ValueError, match=f'AugMix: {arg}'):
                cls(**{arg: bad})


def test_value_table():
    from ffcv_amd.transforms.auto_augment import augmix_table
    m = np.arange(10) / 9
    for H, W in ((32, 32), (33, 47), (1, 1)):
        t = augmix_table(H, W)
        assert t.dtype == np.float64 and t.shape == (14, 10)
        assert np.array_equal(t.view(np.uint64), AM.values(H, W).view(np.uint64)), (H, W)
        assert np.array_equal(t[R.POSTERIZE], np.maximum(1, 4 - np.floor(4 * m + 0.5)))
        assert t[R.TRANSLATE_X, -1] == W // 3 and t[R.TRANSLATE_Y, -1] == H // 3 and t[R.SOLARIZE, -1] == 0


@pytest.mark.parametrize('width,depth,all_ops,alpha', ((1, -1, True, 0.5), (3, 2, False, 1.0), (4, -1, False, 2.5),
                                                       (3, -1, True, 2.5)))
def test_host_draws_match_numpy(hip_lib, width, depth, all_ops, alpha):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import augmix_table
    ids = np.arange(2048, dtype=np.uint64)
    coefs, seen = {}, set()
    for (seed, epoch), severity, (H, W) in (((SEED, 0), 3, (32, 32)), ((2 ** 63 + 5, 7), 10, (33, 47))):
        table = augmix_table(H, W)
        d = L.augmix_draw_batch_host(ids, seed, epoch, severity, width, depth, alpha, all_ops, table, H, W)
        assert [(d[n].dtype, d[n].shape) for n, _, _ in L.augmix_arrays(width)] == \
            [(np.dtype(dt), shape(2048)) for _, dt, shape in L.augmix_arrays(width)]
        for k in range(2048):
            w = AM.draw_weights(seed, epoch, k, width, alpha)
            assert np.array_equal(d['weights'][:, k].view(np.uint32), w.view(np.uint32)), (seed, k)
            for i, steps in enumerate(AM.draw_chains(seed, epoch, k, severity, width, depth, all_ops)):
                assert d['depth'][i, k] == len(steps) and (depth < 0 or len(steps) == depth)
                for j in range(3):
                    op, b, neg = steps[j] if j < len(steps) else (R.IDENTITY, 0, False)
                    s, at = 3 * i + j, (seed, k, i, j)
                    sv = R.signed_value(table, op, b, neg)
                    seen.add(op)
                    assert d['op'][s, k] == op, at
                    cj = {R.BRIGHTNESS: 0, R.COLOR: 1, R.CONTRAST: 2, R.SOLARIZE: 3}.get(op, -1)
                    assert list(d['cj_apply'][s, :, k]) == [int(c == cj) for c in range(4)], at
                    want = np.array([1.0 + sv if c == cj else 1.0 for c in range(3)] + [sv if cj == 3 else 256.0])
                    assert np.array_equal(d['cj_ratio'][s, :, k].view(np.uint64), want.view(np.uint64)), at
                    tone = {R.POSTERIZE: 0, R.AUTOCONTRAST: 1, R.EQUALIZE: 2}.get(op, -1)
                    assert list(d['tone_apply'][s, :, k]) == [int(c == tone) for c in range(3)], at
                    assert d['tone_bits'][s, k] == (table[R.POSTERIZE, b] if op == R.POSTERIZE else 8), at
                    geo = R.SHEAR_X <= op <= R.ROTATE
                    key = (op, neg, b, H, W) if geo else None
                    if key not in coefs:
                        coefs[key] = AR.quantise(AR.matrix_f64(H=H, W=W, **(R.affine_args(op, sv) if geo else dict(
                            angle=0, tx=0, ty=0, s=1, shx=0, shy=0))))
                    assert d['aff_apply'][s, k] == geo and np.array_equal(d['aff_coef'][s, k], coefs[key]), at
                    assert d['sharp_apply'][s, k] == (1 if op == R.SHARPNESS else 2), at
                    f = np.float32(np.float64(1.0) + sv) if op == R.SHARPNESS else np.float32(1)
                    assert d['sharp_factor'][s, k].view(np.uint32) == f.view(np.uint32), at
    assert seen - {R.IDENTITY} == set(AM.OPS_ALL if all_ops else AM.OPS_BASIC)


def test_host_mix_twin_matches_the_statement(hip_lib):
    from ffcv_amd import libffcv as L
    rng = np.random.default_rng(3)
    for width in (1, 3, 4):
        a = [rng.integers(0, 256, (6, 5, 7, 3), dtype=np.uint8) for _ in range(width + 1)]
        a[0][0] = a[1][0] = 255
        w = np.stack([AM.draw_weights(SEED, 0, k, width, 1.0) for k in range(6)], axis=1)
        w[:, 0] = 0.7
        want = np.stack([AM.mix(a[0][k], [r[k] for r in a[1:]], w[:, k]) for k in range(6)])
        assert np.array_equal(L.augmix_mix_batch_host(a[0], a[1:], w, np.empty_like(a[0]), 2), want)
    # half to even on ties, and an unchanged image stays: (0.5, 0.5) on 1 | 2 -> 2, 2 | 3 -> 2
    x, y = np.array([1, 2, 7], np.uint8).reshape(1, 1, 1, 3), np.array([2, 3, 7], np.uint8).reshape(1, 1, 1, 3)
    got = L.augmix_mix_batch_host(x, [y], np.full((2, 1), 0.5, np.float32), np.empty_like(x))
    assert got.ravel().tolist() == [2, 2, 7]


@pytest.mark.parametrize('kw,mode', ((dict(), AR.NEAREST),
                                     (dict(severity=10, mixture_width=2, chain_depth=3, alpha=0.5, all_ops=False,
                                           interpolation='bilinear', fill=(9, 200, 31)), AR.BILINEAR)))
def test_cpu_loader_matches_the_statement(tmp_path, hip_lib, kw, mode):
    from ffcv_amd.loader import Loader
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
    from ffcv_amd.transforms import ToTensor, AugMix
    n = 64
    ds = NaturalDS(n, hw=(32, 32), seed=3)
    fn = write(str(tmp_path / 'am.beton'), ds, {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    op = AugMix(**kw)
    loader = Loader(fn, batch_size=32, device='cpu', seed=SEED, pipelines={
        'image': [SimpleRGBImageDecoder(), op, ToTensor()]})
    table = AM.values(32, 32)
    for epoch in range(2):
        got = np.concatenate([im.numpy().copy() for im, _ in loader])
        for sid in range(n):
            chains = AM.draw_chains(SEED, epoch, sid, op.severity, op.mixture_width, op.chain_depth, op.all_ops)
            w = AM.draw_weights(SEED, epoch, sid, op.mixture_width, op.alpha)
            want = AM.expected(ds.imgs[sid], chains, w, table, mode, tuple(int(x) for x in np.broadcast_to(op.fill, 3)))
            assert np.array_equal(got[sid], want), (epoch, sid, chains)


def test_entries_reject_bad_arguments(hip_lib):
    from ffcv_amd import libffcv as L
    from ffcv_amd.transforms.auto_augment import augmix_table
    lib = L.lib()
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    ids, table = np.arange(2, dtype=np.uint64), augmix_table(8, 8)
    out = [np.full(shape(2), 9, dt) for _, dt, shape in L.augmix_arrays(4)]

    def draw(sev=3, width=3, depth=-1, alpha=1.0, h=8, w=8, batch=2, ids_p=ptr(ids), table_p=ptr(table), drop=None,
             host=True):
        outs = [None if i == drop else ptr(a) for i, a in enumerate(out)]
        args = (ids_p, batch, 0, 0, sev, width, depth, ctypes.c_double(alpha), 1, table_p, h, w, *outs)
        return lib.ffcv_augmix_draw_batch_host(*args) if host else lib.ffcv_augmix_draw_batch(None, *args, None)
    for host in (True, False):
        for kw in [dict(sev=0), dict(sev=11), dict(width=0), dict(width=5), dict(depth=0), dict(depth=4), dict(depth=-2),
                   dict(alpha=0.009), dict(alpha=101.0), dict(alpha=float('nan')), dict(h=0), dict(w=32768),
                   dict(batch=-1), dict(ids_p=None), dict(table_p=None)] + [dict(drop=i) for i in range(len(out))]:
            assert draw(host=host, **kw) == -1, kw
            assert b'ffcv_augmix_draw_batch' in lib.ffcv_last_error()
    assert all((a == 9).all() for a in out) and draw(batch=0) == 0 and draw(batch=0, host=False) == 0
    assert draw(sev=10, width=4, depth=3, alpha=100.0) == 0

    img, fill = np.zeros((2, 8, 8, 3), np.uint8), np.zeros(3, np.uint8)
    dst = np.zeros_like(img)
    d = [np.zeros(shape(2), dt) for _, dt, shape in L.augmix_arrays(2)]

    def pix(src_p=ptr(img), dst_p=ptr(dst), batch=2, h=8, w=8, width=2, mode=1, fill_p=ptr(fill), drop=None):
        arrs = [None if i == drop else ptr(a) for i, a in enumerate(d)]
        return lib.ffcv_augmix_batch(None, src_p, dst_p, batch, h, w, width, mode, fill_p, *arrs)
    assert L.augmix_lds_bytes() == 9 * 64 * 64
    for kw in [dict(src_p=None), dict(dst_p=None), dict(fill_p=None), dict(batch=-1), dict(h=0), dict(width=0),
               dict(width=5), dict(mode=2), dict(dst_p=ptr(img)), dict(h=64, w=65), dict(h=1, w=4097)] + \
            [dict(drop=i) for i in range(len(d))]:
        assert pix(**kw) == -1, kw
        assert b'ffcv_augmix_batch' in lib.ffcv_last_error()
    assert pix(batch=0) == 0 and pix(batch=0, h=64, w=64) == 0 and not dst.any()

    w = np.zeros((2, 2), np.float32)

    def mix(orig=ptr(img), r0=ptr(img), out=ptr(dst), width=1, batch=2, h=8, weights=ptr(w), host=True):
        args = (orig, r0, None, None, None, width, weights, out, batch, h, 8)
        return lib.ffcv_augmix_mix_batch_host(*args, 1) if host else lib.ffcv_augmix_mix_batch(None, *args)
    for host in (True, False):
        for kw in (dict(orig=None), dict(r0=None), dict(out=None), dict(weights=None), dict(width=0), dict(width=2),
                   dict(width=5), dict(batch=-1), dict(h=0), dict(out=ptr(img))):
            assert mix(host=host, **kw) == -1, kw
            assert b'ffcv_augmix_mix_batch' in lib.ffcv_last_error()
    assert mix(batch=0) == 0 and mix(batch=0, host=False) == 0 and mix() == 0
