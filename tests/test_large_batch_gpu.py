"""Every covered device entry on batches whose byte offsets pass 2^31 and 2^32
and whose image count passes 65,535 (tests/large_batch.py): the
default Loader hands the kernels groups of 12,288 images, 2.4 GB at 256 x 256
uint8 and 4.8 GB in fp16, and nothing else in the suite goes there.

Each case prints its wall time; the entries' documented limits are asserted
without a launch at the end of the file."""
import time

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from tests import large_batch as LB

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    LB.need_device()


def _timed(what, t0):
    ch.cuda.synchronize()
    print(f'\n[large_batch] {what}: {time.perf_counter() - t0:.2f} s')


@pytest.mark.parametrize('name,regime,limit', LB.DENSE, ids=lambda v: str(v))
def test_dense_batch(hip_lib, name, regime, limit):
    """Source and destination offsets past the limit; with the 'many' shape the
    image count passes 65,535 (2^31) and 350,000 (2^32)."""
    t0 = time.perf_counter()
    LB.run_dense(LB.BY_NAME[name], LB.built(name, regime), LB.LIMITS[limit])
    _timed(f'{name} {regime} {limit}', t0)


@pytest.mark.parametrize('name,regime', LB.STRIDED, ids=lambda v: str(v))
def test_destination_stride_past_4g(hip_lib, name, regime):
    """80 images written 64 MiB apart: the last destination starts past 2^32."""
    t0 = time.perf_counter()
    LB.run_strided(LB.BY_NAME[name], LB.built(name, regime))
    _timed(f'{name} {regime} stride', t0)


# ------------------------------------------------ rows of labels, not images --
N_ROWS = 350_003


def test_mixup_onehot_rows_past_4g(hip_lib):
    """350,003 rows of 3,079 classes: 4.31 GB of float32 output."""
    t0 = time.perf_counter()
    classes = 3079
    assert N_ROWS * classes * 4 > 1 << 32 and (1 << 32) % (classes * 4) != 0
    a = ch.arange(N_ROWS, device='cuda:0') * 7 % classes
    b = (ch.arange(N_ROWS, device='cuda:0') * 13 + 5) % classes
    lam = (ch.arange(N_ROWS, device='cuda:0') % 97 + 1).float() / 128
    labels3 = ch.stack([a.float(), b.float(), lam], 1).contiguous()
    out = ch.full((N_ROWS, classes), -1.0, device='cuda:0')
    status = ch.full((N_ROWS,), -1, dtype=ch.int32, device='cuda:0')
    L.mixup_onehot_batch(labels3, out, status)
    ch.cuda.synchronize()
    assert bool((status == 0).all())
    rows = ch.arange(N_ROWS, device='cuda:0')
    assert ch.equal(out[rows, b], np.float32(1) - lam)
    ne = a != b
    assert ch.equal(out[rows[ne], a[ne]], lam[ne])
    want_sum = ch.where(ne, lam.double() + (np.float32(1) - lam).double(), (np.float32(1) - lam).double())
    got_sum = ch.zeros(N_ROWS, dtype=ch.float64, device='cuda:0')
    for r0 in range(0, N_ROWS, 20000):                       # every other entry is zero
        got_sum[r0:r0 + 20000] = out[r0:r0 + 20000].double().sum(1)
        assert int((out[r0:r0 + 20000] != 0).sum(1).max()) <= 2
    assert ch.equal(got_sum, want_sum)
    del out, labels3, status, got_sum, want_sum, a, b, lam, rows, ne
    ch.cuda.empty_cache()
    _timed('mixup_onehot_batch', t0)


def test_replace_label_rows_past_4g(hip_lib):
    """350,003 rows of 1,543 int64 labels (4.32 GB); every third sample's id is in the set."""
    t0 = time.perf_counter()
    row = 1543
    assert N_ROWS * row * 8 > 1 << 32
    labels = (ch.arange(N_ROWS * row, device='cuda:0', dtype=ch.int64) % 1009).view(N_ROWS, row)
    ids = ch.arange(N_ROWS, device='cuda:0', dtype=ch.int64) * 5 + 2
    poison = ids[::3].contiguous()
    L.replace_label_batch(labels, ids, poison, -7)
    ch.cuda.synchronize()
    hit = ch.zeros(N_ROWS, dtype=ch.bool, device='cuda:0')
    hit[::3] = True
    assert bool((labels[hit] == -7).all())
    keep = labels[~hit]
    idx = ch.arange(N_ROWS * row, device='cuda:0', dtype=ch.int64).view(N_ROWS, row)[~hit]
    assert ch.equal(keep, idx % 1009)
    del labels, keep, idx, ids, poison, hit
    ch.cuda.empty_cache()
    _timed('replace_label_batch', t0)


# ------------------------------------------------------------------ draws --
def test_draws_of_350000_ids_equal_the_host_draws(hip_lib):
    """Each draw kernel that takes ``batch``, once at 350,003 ids against its
    host twin (the draws whose values are pinned bit for bit)."""
    t0 = time.perf_counter()
    rng = np.random.default_rng(77)
    ids = rng.integers(0, 1 << 40, N_ROWS).astype(np.uint64)
    d_ids = LB.dev(ids.view(np.int64))
    B = N_ROWS

    def z(shape, dt):
        return ch.full(shape, -1 if dt not in (ch.uint8,) else 0xA5, dtype=dt, device='cuda:0')

    status = z((B,), ch.int32)
    yx = z((B, 2), ch.int32)
    L.translate_draw_batch(d_ids, 3, 2, 4, yx, status)
    assert np.array_equal(yx.cpu().numpy(), L.translate_draw_batch_host(ids, 3, 2, 4))
    crops = z((B, 4), ch.int32)
    L.crop_draw_batch(d_ids, 61, 67, (0.08, 1.0), (0.75, 4 / 3), 3, 2, crops, status)
    assert np.array_equal(crops.cpu().numpy(), L.crop_draw_batch_host(ids, 61, 67, (0.08, 1.0), (0.75, 4 / 3), 3, 2))
    apply, val = z((B,), ch.uint8), z((B,), ch.float64)
    L.color_jitter_draw_batch(d_ids, 3, 2, 6, 0.5, 0.4, apply, val, status)
    ha, hv = L.color_jitter_draw_batch_host(ids, 3, 2, 6, 0.5, 0.4)
    assert np.array_equal(apply.cpu().numpy(), ha) and np.array_equal(val.cpu().numpy(), hv)
    L.hue_draw_batch(d_ids, 3, 2, 0.5, 0.3, apply, val, status)
    ha, hv = L.hue_draw_batch_host(ids, 3, 2, 0.5, 0.3)
    assert np.array_equal(apply.cpu().numpy(), ha) and np.array_equal(val.cpu().numpy(), hv)
    fac = z((B,), ch.float32)
    L.sharpness_draw_batch(d_ids, 3, 2, 0.5, 1.75, apply, fac, status)
    ha, hf = L.sharpness_draw_batch_host(ids, 3, 2, 0.5, 1.75)
    assert np.array_equal(apply.cpu().numpy(), ha) and np.array_equal(fac.cpu().numpy(), hf)
    tone = z((3, B), ch.uint8)
    L.tone_draw_batch(d_ids, 3, 2, (15, 17, 18), (0.3, 0.5, 0.7), tone, status)
    assert np.array_equal(tone.cpu().numpy(), L.tone_draw_batch_host(ids, 3, 2, (15, 17, 18), (0.3, 0.5, 0.7)))
    boxes, keys = z((B, 4), ch.int32), z((B,), ch.int64)
    L.erase_draw_batch(d_ids, 3, 2, 0.5, (0.02, 0.33), (0.3, 3.3), 61, 67, boxes, keys, status)
    hb, hk = L.erase_draw_batch_host(ids, 3, 2, 0.5, (0.02, 0.33), (0.3, 3.3), 61, 67)
    assert np.array_equal(boxes.cpu().numpy(), hb) and np.array_equal(keys.cpu().numpy().view(np.uint64), hk)
    assert bool((status == 0).all())
    L.uniform_draw_batch(d_ids, 3, 2, 10, 0.5, 0.25, 0.75, apply, val, status)
    ha, hv = L.uniform_draw_batch_host(ids, 3, 2, 10, 0.5, 0.25, 0.75)
    assert np.array_equal(apply.cpu().numpy(), ha) and np.array_equal(val.cpu().numpy(), hv)
    # the decoders' own draw: crop windows of samples of mixed sizes, cutout origins and flips
    hs, ws = (40 + ids % 97).astype(np.uint32), (50 + ids % 89).astype(np.uint32)
    table = np.zeros(B, L.SAMPLE_DTYPE)
    table['height'], table['width'], table['mode'] = hs, ws, 1
    dp = L.DrawParams()
    dp.crop_kind, dp.out_h, dp.out_w, dp.cutout_size = 0, 32, 32, 8
    dp.scale[:], dp.ratio[:] = (0.08, 1.0), (0.75, 4 / 3)
    dp.center_ratio, dp.loader_seed, dp.epoch, dp.flip_prob = 0.875, 3, 2, 0.5
    cut, flips = z((B, 2), ch.int32), z((B,), ch.uint8)
    L.draw_batch(d_ids, LB.dev(table.view(np.uint8)), dp, crops, cut, flips, status)
    hc, hy, hf = np.empty((B, 4), np.int32), np.empty((B, 2), np.int32), np.empty(B, np.uint8)
    L.draw_batch_host(ids, hs, ws, dp, hc, hy, hf)
    assert np.array_equal(crops.cpu().numpy(), hc) and np.array_equal(cut.cpu().numpy(), hy)
    assert np.array_equal(flips.cpu().numpy(), hf)
    assert bool((status == 0).all())
    del d_ids, status, yx, crops, apply, val, fac, tone, boxes, keys, cut, flips
    ch.cuda.empty_cache()
    _timed('draws', t0)


def _same(dev_arrays, host_arrays, what):
    for name, h in host_arrays.items():
        got = dev_arrays[name].cpu().numpy()
        assert got.shape == h.shape and np.array_equal(got.view(np.uint8), h.view(np.uint8)), (what, name)


def test_policy_draws_of_350000_ids_equal_the_host_draws(hip_lib):
    """The draws with per-sample rows of coefficients, weights and slots (blur,
    affine, the joint colour jitter, TrivialAugmentWide, RandAugment, AugMix)
    at 350,003 ids, bit for bit against their host twins, as the small-batch
    tests of each compare them."""
    from tests import augmix_ref as AM
    from tests import randaugment_ref as RA
    t0 = time.perf_counter()
    ids = np.random.default_rng(78).integers(0, 1 << 40, N_ROWS).astype(np.uint64)
    d_ids = LB.dev(ids.view(np.int64))
    B, H, W = N_ROWS, 61, 67

    def z(shape, dt):
        return ch.full(shape, 77, dtype=getattr(ch, np.dtype(dt).name), device='cuda:0')

    def arrays(spec):
        return {name: z(shape(B), dt) for name, dt, shape in spec}

    status = z((B,), np.int32)
    d = {'apply': z((B,), np.uint8), 'sigma': z((B,), np.float64), 'weights': z((B, 32), np.float32)}
    L.blur_draw_batch(d_ids, 3, 2, 0.5, 0.1, 2.0, 5, d['apply'], d['sigma'], d['weights'], status)
    _same(d, dict(zip(('apply', 'sigma', 'weights'), L.blur_draw_batch_host(ids, 3, 2, 0.5, 0.1, 2.0, 5))), 'blur')
    assert bool((status == 0).all())
    ranges = (-30, 30, -4, 4, -4, 4, 0.8, 1.25, -10, 10, -10, 10)
    d = {'apply': z((B,), np.uint8), 'coef': z((B, 6), np.int64)}
    L.affine_draw_batch(d_ids, 3, 2, 0.5, ranges, H, W, d['apply'], d['coef'], status)
    _same(d, dict(zip(('apply', 'coef'), L.affine_draw_batch_host(ids, 3, 2, 0.5, ranges, H, W))), 'affine')
    assert bool((status == 0).all())
    mag = (0.4, 0.3, 0.2, 0.1)
    d = {'apply': z((4, B), np.uint8), 'ratio': z((4, B), np.float64)}
    L.color_jitter_joint_draw_batch(d_ids, 3, 2, 0.8, mag, d['apply'], d['ratio'], status)
    _same(d, dict(zip(('apply', 'ratio'), L.color_jitter_joint_draw_batch_host(ids, 3, 2, 0.8, mag))), 'joint')
    assert bool((status == 0).all())
    table = RA.values(31, H, W)
    d = arrays(L.POLICY_ARRAYS)
    L.policy_draw_batch(d_ids, 3, 2, 31, LB.dev(table), H, W, d, status)
    _same(d, L.policy_draw_batch_host(ids, 3, 2, 31, table, H, W), 'policy')
    assert bool((status == 0).all())
    d = arrays(L.randaugment_arrays(3))
    L.randaugment_draw_batch(d_ids, 3, 2, 3, 31, 9, LB.dev(table), H, W, d, status)
    _same(d, L.randaugment_draw_batch_host(ids, 3, 2, 3, 31, 9, table, H, W), 'randaugment')
    assert bool((status == 0).all())
    d = arrays(L.augmix_arrays(3))
    L.augmix_draw_batch(d_ids, 3, 2, 7, 3, -1, 1.0, True, LB.dev(AM.values(H, W)), H, W, d, status)
    _same(d, L.augmix_draw_batch_host(ids, 3, 2, 7, 3, -1, 1.0, True, AM.values(H, W), H, W), 'augmix')
    assert bool((status == 0).all())
    del d, d_ids, status
    ch.cuda.empty_cache()
    _timed('policy draws', t0)


# ------------------------------------------------- the entries' own limits --
def _refused(lib, rc, who, word=''):
    msg = lib.ffcv_last_error()
    assert rc == EINVAL and who.encode() in msg and word.encode() in msg, (rc, msg)


def test_limits_are_refused_and_empty_batches_accepted_without_a_launch(hip_lib):
    """The first size beyond each documented limit is FFCV_EINVAL with the
    entry's name in the message; batch == 0 is FFCV_OK.  Nothing is launched:
    the one small buffer every pointer names keeps its fill."""
    lib = hip_lib
    buf = ch.full((4096,), 0xA5, dtype=ch.uint8, device='cuda:0')
    p, s = buf.data_ptr(), L._stream(None)
    H = W = 26755                                            # 3 H W = 2^31 + 6,427: the first square past u8_images_ok
    assert 3 * H * W > 0x7fffffff >= 3 * H * (W - 1)
    cj, tone = L.color_jitter_params((1,)), L.tone_params((4,))
    import ctypes
    f3 = (ctypes.c_uint8 * 3)(1, 2, 3)
    _refused(lib, lib.ffcv_color_jitter_batch(s, p, 1, H, W, ctypes.byref(cj), p, p, None, 0), 'ffcv_color_jitter_batch')
    _refused(lib, lib.ffcv_hue_batch(s, p, 1, H, W, p, p), 'ffcv_hue_batch')
    _refused(lib, lib.ffcv_tone_batch(s, p, 1, H, W, ctypes.byref(tone), p, None, 0), 'ffcv_tone_batch')
    _refused(lib, lib.ffcv_affine_batch(s, p, p + 2048, 1, H, W, 0, f3, p, p, 0), 'ffcv_affine_batch')
    # 0x7fffffff workgroups: beyond the LDS regime an image is cut into tiles of 4,096 pixels (the kernels'
    # *_TILE_PX), and the first batch whose workgroups pass the limit is refused
    h2, w2 = 16384, 16385
    ntiles = -(-h2 * w2 // LB.TILE_PX)
    first = 0x7fffffff // ntiles + 1
    assert first * ntiles > 0x7fffffff >= (first - 1) * ntiles
    _refused(lib, lib.ffcv_color_jitter_batch(s, p, first, h2, w2, ctypes.byref(cj), p, p, None, 0),
             'ffcv_color_jitter_batch')
    _refused(lib, lib.ffcv_hue_batch(s, p, first, h2, w2, p, p), 'ffcv_hue_batch')
    _refused(lib, lib.ffcv_tone_batch(s, p, first, h2, w2, ctypes.byref(tone), p, None, 0), 'ffcv_tone_batch')
    # erase: 65,535 planes and 2^31 - 1 samples; cutmix and erase: a sample of 2^31 - 1 bytes
    _refused(lib, lib.ffcv_erase_batch(s, p, 1, 65536, 2, 2, 1, p, 0, 1, p, None), 'ffcv_erase_batch')
    _refused(lib, lib.ffcv_erase_batch(s, p, 1 << 31, 1, 2, 2, 1, p, 0, 1, p, None), 'ffcv_erase_batch')
    _refused(lib, lib.ffcv_erase_batch(s, p, 1, 1, 32768, 32768, 2, p, 0, 1, p, None), 'ffcv_erase_batch')
    _refused(lib, lib.ffcv_cutmix_batch(s, p, p + 2048, 1, 1, 32768, 32768, 2, 1, p, 0), 'ffcv_cutmix_batch')
    # sides: blur and sharpness up to 65,535, affine up to 32,767
    _refused(lib, lib.ffcv_gaussian_blur_batch(s, p, p + 2048, 1, 65536, 1, 1, p, p, 0), 'ffcv_gaussian_blur_batch')
    _refused(lib, lib.ffcv_sharpness_batch(s, p, p + 2048, 1, 1, 65536, p, p, 0), 'ffcv_sharpness_batch')
    _refused(lib, lib.ffcv_affine_batch(s, p, p + 2048, 1, 32768, 1, 0, f3, p, p, 0), 'ffcv_affine_batch')
    # the fused policies beyond their LDS regimes
    hr, wr = LB.odd_shape(L.randaugment_lds_bytes() // 2)
    assert 6 * hr * wr > L.randaugment_lds_bytes()
    _refused(lib, lib.ffcv_randaugment_batch(s, p, p + 2048, 1, hr, wr, 1, 0, f3, *([p] * 9)), 'ffcv_randaugment_batch')
    assert not L.randaugment_large_fits(225, 225)
    _refused(lib, lib.ffcv_randaugment_large_batch(s, p, p + 2048, 1, 225, 225, 1, 0, f3, *([p] * 9)),
             'ffcv_randaugment_large_batch')
    ha, wa = LB.odd_shape(L.augmix_lds_bytes() // 3)
    assert 9 * ha * wa > L.augmix_lds_bytes()
    _refused(lib, lib.ffcv_augmix_batch(s, p, p + 2048, 1, ha, wa, 1, 0, f3, *([p] * 11)), 'ffcv_augmix_batch')

    # mixup, cutmix, poison: chunk blocks x runs of at most 2^31 - 1 workgroups.  One chunk block a sample
    # (samples of 16 bytes) and runs of 4 samples: the first count beyond is 4 * (2^31 - 1) + 1 samples
    n_over = 4 * 0x7fffffff + 1
    _refused(lib, lib.ffcv_mixup_batch(s, p, p + (1 << 40), n_over, 16, 1, n_over, p, 1), 'ffcv_mixup_batch', 'workgroups')
    # sides of the draws: 32,767
    d2 = (ctypes.c_double * 2)(0.1, 0.5)
    d12 = (ctypes.c_double * 12)(*([0.0, 0.0] * 3 + [1.0, 1.0] + [0.0, 0.0] * 2))
    _refused(lib, lib.ffcv_affine_draw_batch(s, p, 1, 1, 1, 0.5, d12, 32768, 4, p, p, None), 'ffcv_affine_draw_batch')
    _refused(lib, lib.ffcv_erase_draw_batch(s, p, 1, 1, 1, 0.5, d2, d2, 4, 32768, p, None, None),
             'ffcv_erase_draw_batch')
    _refused(lib, lib.ffcv_policy_draw_batch(s, p, 1, 1, 1, 31, p, 32768, 4, *([p] * 9), None),
             'ffcv_policy_draw_batch')
    _refused(lib, lib.ffcv_randaugment_draw_batch(s, p, 1, 1, 1, 2, 31, 9, p, 4, 32768, *([p] * 9), None),
             'ffcv_randaugment_draw_batch')
    _refused(lib, lib.ffcv_augmix_draw_batch(s, p, 1, 1, 1, 7, 3, -1, 1.0, 1, p, 32768, 4, *([p] * 11), None),
             'ffcv_augmix_draw_batch')
    # blur, sharpness, affine: more than 2^31 - 1 workgroups.  Beyond the whole-image regime an image of
    # 32,767 x 32,767 is cut into at least 32,767 / 64 bands or tiles a side
    _refused(lib, lib.ffcv_sharpness_batch(s, p, p + (1 << 63), 0x7fffffff, 32767, 32767, p, p, 0),
             'ffcv_sharpness_batch', 'workgroups')

    # cutmix and poison, as mixup: one chunk block a sample, so the runs alone pass 2^31 - 1.  Their runs hold at
    # most 64 samples (poison's longest; cutmix's are shorter), so 64 * (2^31 - 1) + 1 samples are beyond either
    n64 = 64 * 0x7fffffff + 1
    _refused(lib, lib.ffcv_cutmix_batch(s, p, p + (1 << 44), n64, 1, 1, 16, 1, n64, p, 1), 'ffcv_cutmix_batch', 'workgroups')
    _refused(lib, lib.ffcv_poison_batch(s, p, n64, 16, p, p, 1, p, p, 0.0, 255.0), 'ffcv_poison_batch', 'workgroups')
    # blur and affine: at least 32,767 / 64 bands or tiles a side of a 32,767 x 32,767 image
    _refused(lib, lib.ffcv_gaussian_blur_batch(s, p, p + (1 << 63), 0x7fffffff, 32767, 32767, 3, p, p, 0),
             'ffcv_gaussian_blur_batch', 'workgroups')
    _refused(lib, lib.ffcv_affine_batch(s, p, p + (1 << 63), 0x7fffffff, 26754, 26754, 0, f3, p, p, 0),
             'ffcv_affine_batch', 'workgroups')
    # the JPEG decoder: 65,535 images a launch, in the context and in the Python class
    with pytest.raises(L.FFCVError, match='65535'):
        L.JpegDecoder(65536, 64, 64, 4096)

    # batch == 0: FFCV_OK, or for the entries that document a count > 0, the refusal
    assert lib.ffcv_cutout_batch(s, p, 0, 4, 5, p, 2, f3) == 0
    assert lib.ffcv_flip_batch(s, p, p + 2048, 0, 4, 5, 3, p) == 0
    assert lib.ffcv_translate_batch(s, p, p + 2048, 0, 4, 5, p, 1, f3) == 0
    assert lib.ffcv_lut_batch(s, p, 0, p, 2, p + 2048) == 0
    assert lib.ffcv_gather_rows(s, p, 4096, p, 1, p, 0, 8, p + 2048, 8, p) == 0
    assert lib.ffcv_color_jitter_batch(s, p, 0, 4, 5, ctypes.byref(cj), p, p, None, 0) == 0
    assert lib.ffcv_hue_batch(s, p, 0, 4, 5, p, p) == 0
    assert lib.ffcv_tone_batch(s, p, 0, 4, 5, ctypes.byref(tone), p, None, 0) == 0
    assert lib.ffcv_gaussian_blur_batch(s, p, p + 2048, 0, 4, 5, 3, p, p, 0) == 0, lib.ffcv_last_error()
    assert lib.ffcv_sharpness_batch(s, p, p + 2048, 0, 4, 5, p, p, 0) == 0, lib.ffcv_last_error()
    assert lib.ffcv_affine_batch(s, p, p + 2048, 0, 4, 5, 0, f3, p, p, 0) == 0, lib.ffcv_last_error()
    assert lib.ffcv_gather_raw_batch(s, p, p, 0, p + 2048, 64) == 0
    sa = L.SimpleAugParams()
    sa.n_steps, sa.steps[0] = 1, L.AUG_FLIP
    assert lib.ffcv_simple_aug_batch(s, p, p, 0, 4, 5, ctypes.byref(sa), p, None, None, None, p + 2048, 0) == 0, \
        lib.ffcv_last_error()
    rp = L.RRCParams()
    rp.out_h, rp.out_w = 2, 2
    assert lib.ffcv_rrc_images_batch(s, p, 60, 0, 4, 5, p, None, None, ctypes.byref(rp), p + 2048, None, None, 0) == 0, \
        lib.ffcv_last_error()
    assert lib.ffcv_rrc_raw_batch(s, p, p, 0, p, None, None, ctypes.byref(rp), p + 2048) == 0, lib.ffcv_last_error()
    assert lib.ffcv_randaugment_batch(s, p, p + 2048, 0, 4, 5, 1, 0, f3, *([p] * 9)) == 0, lib.ffcv_last_error()
    assert lib.ffcv_randaugment_large_batch(s, p, p + 2048, 0, 4, 5, 1, 0, f3, *([p] * 9)) == 0, lib.ffcv_last_error()
    assert lib.ffcv_augmix_batch(s, p, p + 2048, 0, 4, 5, 1, 0, f3, *([p] * 11)) == 0, lib.ffcv_last_error()
    assert lib.ffcv_augmix_mix_batch(s, p, p + 1024, None, None, None, 1, p, p + 2048, 0, 4, 5) == 0, \
        lib.ffcv_last_error()
    assert lib.ffcv_translate_draw_batch(s, p, 0, 1, 1, 4, p, None) == 0
    assert lib.ffcv_color_jitter_draw_batch(s, p, 0, 1, 1, 5, 0.5, 0.4, p, p, None) == 0
    assert lib.ffcv_hue_draw_batch(s, p, 0, 1, 1, 0.5, 0.3, p, p, None) == 0
    assert lib.ffcv_sharpness_draw_batch(s, p, 0, 1, 1, 0.5, 1.5, p, p, None) == 0
    assert lib.ffcv_blur_draw_batch(s, p, 0, 1, 1, 0.5, 0.1, 2.0, 5, p, p, p, None) == 0
    assert lib.ffcv_affine_draw_batch(s, p, 0, 1, 1, 0.5, d12, 4, 5, p, p, None) == 0
    assert lib.ffcv_erase_draw_batch(s, p, 0, 1, 1, 0.5, d2, d2, 4, 5, p, None, None) == 0
    assert lib.ffcv_tone_batch_bits(s, p, 0, 4, 5, ctypes.byref(tone), p, None, 0, p) == 0
    dsc, dra = (ctypes.c_double * 2)(0.08, 1.0), (ctypes.c_double * 2)(0.75, 1.33)
    assert lib.ffcv_crop_draw_batch(s, p, 0, 4, 5, dsc, dra, 1, 1, p, None) == 0, lib.ffcv_last_error()
    i3, p3 = (ctypes.c_int32 * 3)(15, 17, 18), (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    assert lib.ffcv_tone_draw_batch(s, p, 0, 1, 1, 3, i3, p3, p, None) == 0, lib.ffcv_last_error()
    m4 = (ctypes.c_double * 4)(0.4, 0.3, 0.2, 0.1)
    assert lib.ffcv_color_jitter_joint_draw_batch(s, p, 0, 1, 1, 0.5, m4, p, p, None) == 0, lib.ffcv_last_error()
    assert lib.ffcv_uniform_draw_batch(s, p, 0, 1, 1, 10, 0.5, 0.2, 0.8, p, p, None) == 0, lib.ffcv_last_error()
    assert lib.ffcv_policy_draw_batch(s, p, 0, 1, 1, 31, p, 4, 5, *([p] * 9), None) == 0, lib.ffcv_last_error()
    assert lib.ffcv_randaugment_draw_batch(s, p, 0, 1, 1, 2, 31, 9, p, 4, 5, *([p] * 9), None) == 0, \
        lib.ffcv_last_error()
    assert lib.ffcv_augmix_draw_batch(s, p, 0, 1, 1, 7, 3, -1, 1.0, 1, p, 4, 5, *([p] * 11), None) == 0, \
        lib.ffcv_last_error()
    ddp = L.DrawParams()
    ddp.out_h = ddp.out_w = 8
    assert lib.ffcv_draw_batch(s, p, p, 0, ctypes.byref(ddp), p, None, None, None) == 0, lib.ffcv_last_error()
    # these document a count > 0 (include/ffcv_hip.h): an empty batch is refused, not launched
    _refused(lib, lib.ffcv_mixup_batch(s, p, p + 2048, 0, 16, 1, 1, p, 0), 'ffcv_mixup_batch')
    _refused(lib, lib.ffcv_cutmix_batch(s, p, p + 2048, 0, 1, 4, 5, 3, 1, p, 0), 'ffcv_cutmix_batch')
    _refused(lib, lib.ffcv_erase_batch(s, p, 0, 1, 4, 5, 3, p, 0, 1, p, None), 'ffcv_erase_batch')
    _refused(lib, lib.ffcv_poison_batch(s, p, 0, 16, p, p, 1, p, p, 0.0, 255.0), 'ffcv_poison_batch')
    _refused(lib, lib.ffcv_mixup_onehot_batch(s, p, p + 2048, 0, 10, p), 'ffcv_mixup_onehot_batch')
    _refused(lib, lib.ffcv_replace_label_batch(s, p, 0, 1, p, p, 1, 5), 'ffcv_replace_label_batch')
    ch.cuda.synchronize()
    assert bool((buf == 0xA5).all())


def test_the_comparison_sees_one_changed_byte_past_4g(hip_lib):
    """The harness itself: one byte changed in the last image of a tiled batch
    past 2^32 bytes, and one image moved to its neighbour's place, are each
    reported with their image index."""
    b = LB.built('flip_batch[1]', 'many')
    batch = LB.batch_for(1 << 32, b.src_img)
    reps = batch // LB.M
    buf = LB.DevBuf(batch * b.src_img, 5)
    d_base = LB.dev(b.base)
    LB.tile_bytes(buf.flat, d_base, reps)
    assert LB.differing(buf.flat, d_base, reps) == (0, [])
    buf.flat[batch * b.src_img - 1] ^= 1
    assert LB.differing(buf.flat, d_base, reps) == (1, [batch - 1])
    k = (1 << 32) // b.src_img + 2
    buf.flat[k * b.src_img:(k + 1) * b.src_img] = buf.flat[(k - 1) * b.src_img:k * b.src_img].clone()
    assert LB.differing(buf.flat, d_base, reps) == (2, [k, batch - 1])
    buf.buf[buf.lo - 1] = 0
    assert not buf.guards_ok()
    del buf
    ch.cuda.empty_cache()


def test_jpeg_rrc_destination_stride_past_4g(hip_lib, oracle):
    """JpegDecoder.rrc on 80 copies of one 48 x 80 stream, fp16 output, the
    images 64 MiB apart: the last starts past 2^32.  Each image has a crop of
    its own, so no two neighbours are equal; the expected images are the
    oracle's decode and resize through the table."""
    from ffcv_amd.synthetic import natural_image, encode_jpeg, pack
    t0 = time.perf_counter()
    B, stride, (oh, ow) = LB.STRIDE_BATCH, LB.STRIDE_BYTES, (24, 40)
    img = natural_image(np.random.default_rng(5), 48, 80)
    blob = encode_jpeg(img, 90, '4:2:0')
    buf, offs, sizes = pack([blob])
    smp = np.zeros(B, L.SAMPLE_DTYPE)
    smp['offset'], smp['size'], smp['height'], smp['width'] = offs[0], sizes[0], 48, 80
    k = np.arange(B)
    crops = np.stack([k % 7, k % 11, 40 - k % 5, 64 - k % 9], 1).astype(np.int32)
    table = np.random.default_rng(6).permutation(65536)[:768].astype(np.uint16).reshape(256, 3)
    u8 = oracle.rrc_batch([(np.frombuffer(blob, np.uint8), 48, 80, 0)] * B, crops, oh, ow)
    want = LB.dev(np.stack([table[u8[i].reshape(-1), np.arange(oh * ow * 3) % 3] for i in range(B)]).view(np.uint8))
    assert all(not np.array_equal(u8[i], u8[i + 1]) for i in range(B - 1))
    n = oh * ow * 6
    dst = LB.DevBuf((B - 1) * stride + n, 10)
    d_table = LB.dev(table)
    p = L.RRCParams()
    p.out_h, p.out_w, p.out_stride, p.lut = oh, ow, stride, d_table.data_ptr()
    status = ch.full((B,), -1, dtype=ch.int32, device='cuda:0')
    dec = L.JpegDecoder(B, 48, 80, len(blob))
    dec.rrc(LB.dev(buf), LB.dev(smp.view(np.uint8)), B, LB.dev(crops), None, None, p, dst.flat, status)
    ch.cuda.synchronize()
    assert bool((status == 0).all()) and dst.guards_ok()
    bad = [i for i in range(B) if not ch.equal(dst.flat[i * stride:i * stride + n], want[i].reshape(-1))]
    assert not bad, f'{len(bad)} of {B} images differ, first {bad[:8]}'
    gaps = [i for i in range(B - 1) if not bool((dst.flat[i * stride + n:(i + 1) * stride] == 0xA5).all())]
    assert not gaps, gaps[:8]
    dec.close()
    del dst, want, status
    ch.cuda.empty_cache()
    _timed('JpegDecoder.rrc stride', t0)
