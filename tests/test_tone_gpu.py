"""RandomPosterize / RandomAutocontrast / RandomEqualize / RandomInvert on the
MI355X, bit for bit against the statement (tests/tone_ref.py, itself pinned to
Pillow in tests/test_tone.py): ffcv_tone_batch on shapes of both regimes and
at the border between them, every ordered program of one to three steps, every
byte alignment, images inside guarded buffers; a reused workspace; the device
draws against the host draws; rejections before a launch; and device Loaders
against the CPU Loader under the same seed."""
import ctypes
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, RandomHorizontalFlip, RandomBrightness,
                                 RandomContrast, RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert)
from tests import tone_ref as R
from tests.helpers import NaturalDS, write

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
# 1 x 1; 105 bytes (images straddle 16-byte chunks); the largest whole image (16,383 bytes); the first tiled
# one (16,386 bytes: a last tile of 1,366 pixels); 13 tiles, the last of 3,285 pixels
SHAPES = ((1, 1), (5, 7), (43, 127), (2, 2731), (231, 227))
BATCH_FAMILIES = ('noise', 'band', 'noise', 'two_valued', 'normal', 'flat', 'constant_channel')
PROGRAMS = {'one_two': [p for n in (1, 2) for p in itertools.permutations(R.KINDS, n)],
            'three_a': list(itertools.permutations(R.KINDS, 3))[:12],
            'three_b': list(itertools.permutations(R.KINDS, 3))[12:]}


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def tmpdir_m():
    return tempfile.mkdtemp()


def _batch(shape, seed=0):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + seed)
    return np.stack([R.family(rng, f, *shape) for f in BATCH_FAMILIES])


def _device_tone(imgs, steps, bits, apply, lead=0, ws='fresh'):
    """ffcv_tone_batch on a copy of imgs placed GUARD + lead bytes into a
    16-byte aligned device buffer with GUARD bytes behind it; returns the images
    and checks that the guard bytes on both sides came back as they were."""
    nb = imgs.size
    buf = ch.full((GUARD + lead + nb + GUARD + 16,), 0xA5, dtype=ch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + lead
    view = buf[lo:lo + nb].view(imgs.shape)
    view.copy_(ch.from_numpy(np.ascontiguousarray(imgs)))
    if isinstance(ws, str):
        ws = ch.full((L.tone_workspace_bytes(len(imgs)) // 4,), 0x5A5A5A5A, dtype=ch.int32, device=DEV)
    L.tone_batch(view, steps, bits, ch.from_numpy(np.ascontiguousarray(apply, np.uint8)).to(DEV), ws)
    out = buf.cpu().numpy()
    assert (out[:lo] == 0xA5).all() and (out[lo + nb:] == 0xA5).all()
    return out[lo:lo + nb].reshape(imgs.shape)


def test_the_shapes_track_the_staging_budget():
    assert L.tone_lds_bytes() == 16384
    whole = [h * w * 3 <= L.tone_lds_bytes() for h, w in SHAPES]
    assert whole == [True, True, True, False, False]
    assert 43 * 127 * 3 == 16383 and 2 * 2731 * 3 == 16386          # one pixel apart
    assert L.tone_workspace_bytes(7) == 7 * 3 * 256 * 4


@pytest.mark.parametrize('part', sorted(PROGRAMS))
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_program_on_every_shape(shape, part):
    """B = 7: image 0 and the flat image 5 run every step, image 2 none (it
    and the guards stay byte-identical), the others a mix."""
    imgs = _batch(shape)
    rng = np.random.default_rng(len(part) + shape[1])
    changed = 0
    for j, program in enumerate(PROGRAMS[part]):
        bits = 1 + (j + shape[0]) % 8
        apply = (rng.random((len(program), 7)) < 0.6).astype(np.uint8)
        apply[:, 0], apply[:, 2], apply[:, 5] = 1, 0, 1
        got = _device_tone(imgs, program, bits, apply, lead=(3 * j + 1) % 16)
        want = R.apply_program_batch(imgs, program, bits, apply)
        bad = [k for k in range(7) if not np.array_equal(got[k], want[k])]
        assert not bad, (shape, program, bits, bad)
        assert np.array_equal(got[2], imgs[2])
        changed += not np.array_equal(want, imgs)
    assert changed > 0


_ALIGN = {}


@pytest.mark.parametrize('lead', range(16))
@pytest.mark.parametrize('shape', ((5, 7), (61, 90)), ids=str)
def test_every_alignment(shape, lead):
    """[posterize, equalize, autocontrast] at byte leads 0..15: every channel
    phase of the word map, whole image (105 bytes) and tiles (61 x 90: 5,490
    pixels, a last tile of 1,394)."""
    program, bits = (R.POSTERIZE, R.EQUALIZE, R.AUTOCONTRAST), 5
    assert (shape[0] * shape[1] * 3 > L.tone_lds_bytes()) == (shape == (61, 90))
    if shape not in _ALIGN:                                  # the reference once per shape, then read only
        imgs = _batch(shape, seed=7)[:5]
        apply = np.array([[1, 1, 0, 1, 0], [1, 0, 1, 1, 0], [1, 1, 1, 0, 0]], np.uint8)
        want = R.apply_program_batch(imgs, program, bits, apply)
        want.setflags(write=False)
        _ALIGN[shape] = (imgs, apply, want)
    imgs, apply, want = _ALIGN[shape]
    got = _device_tone(imgs, program, bits, apply, lead)
    bad = [k for k in range(5) if not np.array_equal(got[k], want[k])]
    assert not bad, (shape, lead, bad)
    assert np.array_equal(got[4], imgs[4]) and not np.array_equal(got[0], imgs[0])


def test_a_reused_workspace_gives_the_same_result():
    """A tiled program with statistics twice on the same workspace (first full
    of garbage, then of the first run's counters)."""
    imgs = _batch((70, 83))
    program, bits = (R.INVERT, R.EQUALIZE, R.POSTERIZE, R.AUTOCONTRAST), 3
    apply = np.ones((4, 7), np.uint8)
    apply[:, 2] = 0
    apply[0, 1] = apply[3, 3] = 0
    want = R.apply_program_batch(imgs, program, bits, apply)
    ws = ch.full((L.tone_workspace_bytes(7) // 4 + 5,), -1, dtype=ch.int32, device=DEV)
    first = _device_tone(imgs, program, bits, apply, 5, ws)
    counters = ws.cpu().numpy()
    assert (counters[-5:] == -1).all() and counters[:-5].reshape(7, 3, 256)[[0, 1, 3, 4, 5, 6]].sum(-1).tolist() == \
        [[70 * 83] * 3] * 6 and not counters[:-5].reshape(7, 3, 256)[2].any()
    second = _device_tone(imgs, program, bits, apply, 5, ws)
    assert np.array_equal(first, want) and np.array_equal(second, want)


def test_device_draws_equal_host_draws_and_randomstate():
    rng = np.random.default_rng(8)
    n = 4096
    ids = rng.integers(0, 2 ** 40, n).astype(np.uint64)
    ids[:16] = np.arange(16)
    d_ids = ch.from_numpy(ids.view(np.int64)).to(DEV)
    for seed, epoch, ops, ps in ((0, 0, (15, 16, 17, 18), (0.5, 0.25, 1.0, 0.0)), (2 ** 63 + 5, 7, (18, 15), (0.7, 0.1)),
                                 (12345, 400, (17,), (0.5,))):
        rows = len(ops)
        apply = ch.full((rows + 1, n), 9, dtype=ch.uint8, device=DEV)
        status = ch.full((n,), -1, dtype=ch.int32, device=DEV)
        L.tone_draw_batch(d_ids, seed, epoch, ops, ps, apply, status)
        host = L.tone_draw_batch_host(ids, seed, epoch, ops, ps)
        got = apply.cpu().numpy()
        assert (status == 0).all() and np.array_equal(got[:rows], host) and (got[rows] == 9).all()
        for i, (op, p) in enumerate(zip(ops, ps)):
            kind = {v: k for k, v in R.OP_ID.items()}[op]
            assert got[i, :300].tolist() == [int(R.draw(seed, epoch, int(s), kind, p)) for s in ids[:300]]
            if p == 0.5:
                assert 1800 < int(got[i].sum()) < 2300


def test_abi_rejects_bad_arguments_before_a_launch():
    lib = L.lib()
    n = 4
    img = ch.full((n, 80, 80, 3), 77, dtype=ch.uint8, device=DEV)     # a launch of invert would change it
    before = img.clone()
    apply = ch.ones((4, n), dtype=ch.uint8, device=DEV)
    ws = ch.zeros((768 * n,), dtype=ch.int32, device=DEV)
    ids = ch.arange(n, dtype=ch.int64, device=DEV)
    ch.cuda.synchronize()
    i, a, w, d = img.data_ptr(), apply.data_ptr(), ws.data_ptr(), ids.data_ptr()
    inv = ctypes.byref(L.tone_params([R.INVERT, R.EQUALIZE], 8))
    for args in ((None, n, 80, 80, inv, a, w, 3072 * n), (i, n, 80, 80, None, a, w, 3072 * n),
                 (i, n, 80, 80, inv, None, w, 3072 * n), (i, -1, 80, 80, inv, a, w, 3072 * n),
                 (i, n, 0, 80, inv, a, w, 3072 * n), (i, n, 80, -3, inv, a, w, 3072 * n),
                 (i, n, 26755, 26755, inv, a, w, 3072 * n), (i, n, 80, 80, inv, a, None, 0),
                 (i, n, 80, 80, inv, a, w + 2, 3072 * n), (i, n, 80, 80, inv, a, w, 3072 * n - 1),
                 (i, n, 80, 80, ctypes.byref(L.tone_params([R.INVERT, R.INVERT], 8)), a, w, 3072 * n),
                 (i, n, 80, 80, ctypes.byref(L.tone_params([R.INVERT, 7], 8)), a, w, 3072 * n),
                 (i, n, 80, 80, ctypes.byref(L.tone_params([R.INVERT, R.POSTERIZE], 0)), a, w, 3072 * n),
                 (i, n, 80, 80, ctypes.byref(L.tone_params([], 8)), a, w, 3072 * n)):
        assert lib.ffcv_tone_batch(None, *args) == -1 and b'ffcv_tone_batch:' in lib.ffcv_last_error()
    ops, ps = np.array([18, 17], np.int32), np.array([0.5, 0.5])
    o, p = ops.ctypes.data, ps.ctypes.data
    bad_ops, bad_ps = np.array([18, 14], np.int32), np.array([0.5, 1.5])
    for args in ((None, n, 0, 0, 2, o, p, a, None), (d, n, 0, 0, 2, None, p, a, None), (d, n, 0, 0, 2, o, None, a, None),
                 (d, n, 0, 0, 2, o, p, None, None), (d, n, 0, 0, 0, o, p, a, None), (d, n, 0, 0, 5, o, p, a, None),
                 (d, n, 0, 0, 2, bad_ops.ctypes.data, p, a, None), (d, n, 0, 0, 2, o, bad_ps.ctypes.data, a, None)):
        assert lib.ffcv_tone_draw_batch(None, *args) == -1 and b'ffcv_tone_draw_batch:' in lib.ffcv_last_error()
    ch.cuda.synchronize()
    assert ch.equal(img, before) and (apply == 1).all() and not ws.any()          # nothing was launched
    assert lib.ffcv_tone_batch(None, i, 0, 80, 80, inv, a, None, 0) == 0            # an empty batch is fine
    with pytest.raises(TypeError):
        L.tone_batch(img.permute(0, 2, 1, 3), [R.INVERT], 8, apply[:1])


# ------------------------------------------------------------- Loaders --
def _chains():
    return {'four': lambda: [RandomPosterize(3, p=0.5), RandomAutocontrast(p=0.6), RandomEqualize(p=0.4),
                             RandomInvert(p=0.3)],
            'after_jitter': lambda: [RandomBrightness(0.4), RandomContrast(0.4), RandomEqualize(p=0.6),
                                     RandomPosterize(2, p=0.5)],
            'split_by_flip': lambda: [RandomEqualize(p=0.6), RandomInvert(p=0.5), RandomHorizontalFlip(),
                                      RandomAutocontrast(p=0.6), RandomInvert(p=0.5)]}


@pytest.mark.parametrize('hw', ((32, 32), (80, 72)), ids=str)
@pytest.mark.parametrize('case', sorted(_chains()))
def test_device_loader_matches_cpu_loader(tmpdir_m, case, hw):
    """[decoder, ToTensor, ToDevice, the new operations, ToTorchImage] on the
    device Loader against the CPU Loader ([decoder, the new operations,
    ToTensor]) under the same seed, over two epochs; 32 x 32 images (whole
    image regime) and 80 x 72 (tiles)."""
    assert (hw[0] * hw[1] * 3 > L.tone_lds_bytes()) == (hw == (80, 72))
    fn = os.path.join(tmpdir_m, f'tone_raw_{hw[0]}.beton')
    if not os.path.exists(fn):
        write(fn, NaturalDS(40, hw=hw, seed=4), {'image': RGBImageField(write_mode='raw'), 'label': IntField()})
    ops, seed = _chains()[case], 17
    cpu = Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder()] + ops() + [ToTensor()]})
    want = [np.concatenate([im.numpy() for im, _ in cpu]) for _ in range(2)]
    plain = np.concatenate([im.numpy() for im, _ in Loader(fn, batch_size=16, device='cpu', seed=seed, drop_last=False,
                                                           pipelines={'image': [SimpleRGBImageDecoder(), ToTensor()]})])
    changed = [(w != plain).any(axis=(1, 2, 3)) for w in want]
    assert not np.array_equal(want[0], want[1]) and 5 < changed[0].sum() <= 40
    loader = Loader(fn, batch_size=16, seed=seed, drop_last=False, pipelines={
        'image': [SimpleRGBImageDecoder(), ToTensor(), ToDevice(DEV)] + ops() + [ToTorchImage()],
        'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]})
    assert loader.graph.groupable()                          # launch groups are kept
    assert not any(type(n.operation).__name__ == '_ToHost' for n in loader.graph.exec_nodes)
    tone_ops = [n.operation for n in loader.graph.exec_nodes if type(n.operation).__module__.endswith('.tone')]
    assert sum(not o._absorbed for o in tone_ops) == (2 if case == 'split_by_flip' else 1)
    for want_u8 in want:
        got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in loader])
        assert got.dtype == np.uint8 and got.shape == want_u8.shape
        bad = [k for k in range(len(got)) if not np.array_equal(got[k], want_u8[k])]
        assert not bad, (case, hw, bad[:8])
