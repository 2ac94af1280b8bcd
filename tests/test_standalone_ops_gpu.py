"""The first-generation standalone device kernels on the MI355X, each entry
called directly and compared bit for bit with its numpy statement
(tests/standalone_ref.py, tests/translate_ref.py): ffcv_lut_batch /
ffcv_normalize_batch, ffcv_flip_batch, ffcv_translate_batch, ffcv_cutout_batch,
ffcv_gather_raw_batch and ffcv_gather_samples.

Inputs are random, never constant.  Every batch sits ``lead`` bytes (0..15)
past a 16-byte boundary of a 0xA5-filled device buffer, the output in a second
such buffer whose alignment runs against the input's; after each call the
guard bytes on both sides and the untouched source are compared with what was
uploaded.  Shapes are the kernels' own regime boundaries: the group of 12 and
the 8,192-workgroup cap of the table lookup, the 256-workgroup cap of flip and
translate (65,536 bytes an image), the 64-workgroup cap of the raw gather
(16,384 bytes a sample), the 256-thread pass of cutout, and the 65,535 rows of
a grid."""
import ctypes

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.transforms.lut import make_lut
from tests import standalone_ref as R
from tests.translate_ref import translate_np

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
LEADS = tuple(range(16))
SHAPES = ((1, 1), (1, 2), (5, 7), (20, 26), (147, 149), (150, 151))
FILL = (9, 8, 7)
EINVAL = -1
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


class Guarded:
    """``nbytes`` bytes that start ``lead`` bytes past a 16-byte boundary of a
    0xA5-filled device buffer, with at least GUARD such bytes on both sides."""

    def __init__(self, nbytes, lead, data=None):
        self.lo, self.n = GUARD + lead, int(nbytes)
        self.buf = ch.full((self.lo + self.n + GUARD + 16,), 0xA5, dtype=ch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        if data is not None:
            host = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert host.size == self.n
            if self.n:
                self.buf[self.lo:self.lo + self.n].copy_(ch.from_numpy(host))
        self.uploaded = self.buf.cpu().numpy() if data is not None else None
        self.ptr = self.buf.data_ptr() + self.lo

    def read(self):
        """The payload, after checking the guards on both sides."""
        host = self.buf.cpu().numpy()
        assert (host[:self.lo] == 0xA5).all(), 'bytes in front of the buffer were written'
        assert (host[self.lo + self.n:] == 0xA5).all(), 'bytes behind the buffer were written'
        return host[self.lo:self.lo + self.n]

    def assert_untouched(self):
        assert np.array_equal(self.buf.cpu().numpy(), self.uploaded), 'the source was written'


def _dev(a):
    """The bytes of a on the device (a flat uint8 tensor)."""
    return ch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(DEV)


def _stream():
    return L._stream(None)


def _fill3(fill=FILL):
    return (ctypes.c_uint8 * 3)(*fill)


# ------------------------------------------------------------ table lookup --
def _table(elem, seed=0):
    """A (256, 3) table of random bit patterns, all 768 distinct where the
    width allows (one byte: every column a different permutation of 0..255),
    so that a wrong channel or byte position cannot cancel."""
    rng = np.random.default_rng(100 + elem + seed)
    if elem == 1:
        t = np.stack([rng.permutation(256) for _ in range(3)], -1).astype(np.uint8)
        assert not (t[:, 0] == t[:, 1]).all() and not (t[:, 1] == t[:, 2]).all()
        return t
    if elem == 2:
        return rng.permutation(65536)[:768].astype(np.uint16).reshape(256, 3)
    dt = {4: np.uint32, 8: np.uint64}[elem]
    t = rng.integers(0, np.iinfo(dt).max, 768, dtype=dt, endpoint=True)
    assert np.unique(t).size == 768
    return t.reshape(256, 3)


LUT_NS = (1, 2, 3, 11, 12, 13, 35, 36, 37, 3 * 43 * 127)


def _lut_case(lib, elem, n, lead, table, d_table, flat, entry='lut'):
    """One call: in at ``lead`` (so every residue mod 4: the dword and the
    byte path), out at the multiple of the element size that runs against it."""
    out_lead = (15 - lead) // elem * elem
    src = Guarded(n, lead, flat[:n])
    dst = Guarded(n * elem, out_lead)
    assert src.ptr % 4 == lead % 4 and dst.ptr % elem == 0
    if entry == 'lut':
        rc = lib.ffcv_lut_batch(_stream(), src.ptr, n, d_table.data_ptr(), elem, dst.ptr)
    else:
        rc = lib.ffcv_normalize_batch(_stream(), src.ptr, n, d_table.data_ptr(), dst.ptr)
    assert rc == 0, lib.ffcv_last_error()
    got = dst.read().view(table.dtype)
    src.assert_untouched()
    want = R.lut_np(flat[:n], table)
    assert np.array_equal(got, want), (elem, n, lead, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize('elem', (1, 2, 4, 8))
def test_lut_every_size_length_and_alignment(hip_lib, elem):
    """Tail only (n < 12), exactly one, two, three groups, groups plus a tail,
    and 16,383 elements (several workgroups and a tail of 3), for element
    sizes 1, 2, 4 and 8 at every input residue and output alignment."""
    table = _table(elem)
    d_table = _dev(table)
    flat = np.random.default_rng(elem).integers(0, 256, max(LUT_NS), dtype=np.uint8)
    for n in LUT_NS:
        for lead in LEADS:
            _lut_case(hip_lib, elem, n, lead, table, d_table, flat)


def test_normalize_batch_with_the_fp16_table(hip_lib):
    """ffcv_normalize_batch with make_lut's fp16 table (normalize.py:42-49)."""
    table = make_lut(MEAN, STD, np.float16).view(np.uint16)
    d_table = _dev(table)
    flat = np.random.default_rng(5).integers(0, 256, max(LUT_NS), dtype=np.uint8)
    for n in LUT_NS:
        for lead in LEADS:
            _lut_case(hip_lib, 2, n, lead, table, d_table, flat, entry='normalize')


@pytest.mark.parametrize('elem,lead', ((2, 1), (8, 0)), ids=('u16_byte_path', 'u64_dword_path'))
def test_lut_grid_stride_wraps(hip_lib, elem, lead):
    """n = 12 * 256 * 8192 + 12 * 256 + 7: one full sweep of the capped grid,
    a second step of 256 groups, and a tail of 7.  Element size 2 reads its
    input bytewise (lead 1), element size 8 as dwords (201 MB of output);
    compared in chunks so the host copy stays small."""
    n = 12 * 256 * 8192 + 12 * 256 + 7
    table = _table(elem, seed=1)
    d_table = _dev(table)
    flat = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8)
    src = Guarded(n, lead, flat)
    dst = Guarded(n * elem, 16 - elem)
    assert hip_lib.ffcv_lut_batch(_stream(), src.ptr, n, d_table.data_ptr(), elem, dst.ptr) == 0
    ch.cuda.synchronize()
    assert (dst.buf[:dst.lo] == 0xA5).all() and (dst.buf[dst.lo + dst.n:] == 0xA5).all()
    assert ch.equal(src.buf, ch.from_numpy(src.uploaded).to(DEV))
    chunk = 3 * (1 << 21)                                    # a multiple of 3: i % 3 restarts with each chunk
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        got = dst.buf[dst.lo + lo * elem:dst.lo + hi * elem].cpu().numpy().view(table.dtype)
        want = R.lut_np(flat[lo:hi], table)
        assert np.array_equal(got, want), (lo, np.flatnonzero(got != want)[:8] + lo)


def test_lut_empty_and_rejected_calls_write_nothing(hip_lib):
    table = _table(2)
    d_table = _dev(table)
    src = Guarded(36, 0, np.arange(36, dtype=np.uint8))
    dst = Guarded(36 * 16, 0)
    s, i, t, o = _stream(), src.ptr, d_table.data_ptr(), dst.ptr
    assert hip_lib.ffcv_lut_batch(s, i, 0, t, 2, o) == 0           # n = 0: FFCV_OK
    assert hip_lib.ffcv_normalize_batch(s, i, 0, t, o) == 0
    for args in ((None, 36, t, 2, o), (i, 36, None, 2, o), (i, 36, t, 2, None), (i, 36, t, 0, o), (i, 36, t, 3, o),
                 (i, 36, t, 16, o)):
        assert hip_lib.ffcv_lut_batch(s, *args) == EINVAL and b'ffcv_lut_batch' in hip_lib.ffcv_last_error()
    assert hip_lib.ffcv_normalize_batch(s, None, 36, t, o) == EINVAL
    ch.cuda.synchronize()
    assert (dst.read() == 0xA5).all()
    src.assert_untouched()


# -------------------------------------------------------------------- flip --
FLAGS = np.array([0, 1, 255, 1, 0, 255, 0], np.uint8)     # the contract is != 0


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_flip_every_shape_pixel_size_and_alignment(hip_lib, shape):
    """(147, 149) and (150, 151) are 65,709 and 67,950 bytes of u8 RGB: the
    first size past the 256 x 256 bytes one sweep of the grid covers, and one
    more.  Pixels of 1, 3, 6 and 12 bytes: grey, u8 RGB, fp16 RGB, fp32 RGB."""
    H, W = shape
    d_flags = _dev(FLAGS)
    for cb in (1, 3, 6, 12):
        imgs = np.random.default_rng(H * 1000 + W * 10 + cb).integers(0, 256, (7, H, W, cb), dtype=np.uint8)
        want = np.stack([R.flip_np(imgs[k], FLAGS[k]) for k in range(7)])
        assert np.array_equal(want[[0, 4, 6]], imgs[[0, 4, 6]])
        for lead in LEADS:
            src, dst = Guarded(imgs.size, lead, imgs), Guarded(imgs.size, 15 - lead)
            rc = hip_lib.ffcv_flip_batch(_stream(), src.ptr, dst.ptr, 7, H, W, cb, d_flags.data_ptr())
            assert rc == 0, hip_lib.ffcv_last_error()
            got = dst.read().reshape(imgs.shape)
            src.assert_untouched()
            bad = [k for k in range(7) if not np.array_equal(got[k], want[k])]
            assert not bad, (shape, cb, lead, bad)


def test_flip_rejected_calls_write_nothing(hip_lib):
    imgs = np.random.default_rng(1).integers(0, 256, (2, 4, 5, 3), dtype=np.uint8)
    src, dst = Guarded(imgs.size, 0, imgs), Guarded(imgs.size, 0)
    flags = _dev(np.array([1, 1], np.uint8))
    s, i, o, f = _stream(), src.ptr, dst.ptr, flags.data_ptr()
    for args in ((i, i, 2, 4, 5, 3, f), (i, o, 2, 0, 5, 3, f), (i, o, 2, 4, -1, 3, f), (i, o, 2, 4, 5, 0, f),
                 (i, o, -1, 4, 5, 3, f), (None, o, 2, 4, 5, 3, f), (i, None, 2, 4, 5, 3, f), (i, o, 2, 4, 5, 3, None)):
        assert hip_lib.ffcv_flip_batch(s, *args) == EINVAL and b'ffcv_flip_batch' in hip_lib.ffcv_last_error()
    assert hip_lib.ffcv_flip_batch(s, i, o, 0, 4, 5, 3, f) == 0     # an empty batch is fine
    ch.cuda.synchronize()
    assert (dst.read() == 0xA5).all()
    src.assert_untouched()


# --------------------------------------------------------------- translate --
def _windows(p, rng):
    """(0, 0), (p, p) the identity, (2p, 2p), (0, 2p), (2p, 0): every corner
    of the canvas (all fill once p >= the image), and two random windows."""
    fixed = [(0, 0), (p, p), (2 * p, 2 * p), (0, 2 * p), (2 * p, 0)]
    return np.array(fixed + [tuple(rng.integers(0, 2 * p + 1, 2)) for _ in range(2)], np.int32)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_translate_every_shape_padding_and_alignment(hip_lib, shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    imgs = rng.integers(0, 256, (7, H, W, 3), dtype=np.uint8)
    for p in (0, 1, 5, max(H, W) + 3):
        yx = _windows(p, rng)
        d_yx = _dev(yx)
        want = np.stack([translate_np(imgs[k], int(yx[k, 0]), int(yx[k, 1]), p, FILL) for k in range(7)])
        assert np.array_equal(want[1], imgs[1])                                    # (p, p): the image itself
        if p > max(H, W):
            assert (want[[0, 2, 3, 4]] == np.array(FILL, np.uint8)).all()            # the corners: all fill
        for lead in LEADS:
            src, dst = Guarded(imgs.size, lead, imgs), Guarded(imgs.size, 15 - lead)
            rc = hip_lib.ffcv_translate_batch(_stream(), src.ptr, dst.ptr, 7, H, W, d_yx.data_ptr(), p, _fill3())
            assert rc == 0, hip_lib.ffcv_last_error()
            got = dst.read().reshape(imgs.shape)
            src.assert_untouched()
            bad = [k for k in range(7) if not np.array_equal(got[k], want[k])]
            assert not bad, (shape, p, lead, bad, yx[bad].tolist())


# ------------------------------------------------------------------ cutout --
def _origins(H, W, c, rng):
    """The four corners, origins whose square hangs over the bottom and / or
    the right edge (none when c == 1), and random ones: nine in all."""
    yx = [(0, 0), (H - c, W - c), (0, W - c), (H - c, 0)]
    if c > 1:
        yx += [(H - 1, W - 1), (int(rng.integers(H - c + 1, H)), int(rng.integers(0, W - c + 1))),
               (int(rng.integers(0, H - c + 1)), int(rng.integers(W - c + 1, W)))]
    while len(yx) < 9:
        yx.append((int(rng.integers(0, H - c + 1)), int(rng.integers(0, W - c + 1))))
    return np.array(yx, np.int32)


@pytest.mark.parametrize('shape', ((32, 32), (17, 40), (40, 17), (1, 1)), ids=str)
def test_cutout_every_shape_size_origin_and_alignment(hip_lib, shape):
    """crop_size 16 is exactly one pass of the kernel's 256 threads, 17 needs
    two; squares touch the last row and column, and hang over them (clipped as
    numpy slicing clips).  Nine images compared one by one inside guards, so a
    write into a neighbour shows.  No origin is negative."""
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    imgs = rng.integers(0, 256, (9, H, W, 3), dtype=np.uint8)
    for c in sorted({c for c in (1, 5, 16, 17, min(H, W)) if c <= min(H, W)}):
        yx = _origins(H, W, c, rng)
        assert (yx >= 0).all() and (yx[:, 0] < H).all() and (yx[:, 1] < W).all()
        d_yx = _dev(yx)
        want = np.stack([R.cutout_np(imgs[k], int(yx[k, 0]), int(yx[k, 1]), c, FILL) for k in range(9)])
        for lead in LEADS:
            buf = Guarded(imgs.size, lead, imgs)
            rc = hip_lib.ffcv_cutout_batch(_stream(), buf.ptr, 9, H, W, d_yx.data_ptr(), c, _fill3())
            assert rc == 0, hip_lib.ffcv_last_error()
            got = buf.read().reshape(imgs.shape)
            bad = [k for k in range(9) if not np.array_equal(got[k], want[k])]
            assert not bad, (shape, c, lead, bad, yx[bad].tolist())
        assert np.array_equal(d_yx.cpu().numpy().view(np.int32).reshape(9, 2), yx)


# -------------------------------------------------------------- raw gather --
def _raw_samples(residue, rng):
    """Samples of mixed sizes back to back from ``residue`` on: 1 x 1, 13 x 10,
    74 x 74 (16,428 bytes: past the 64 x 256 one sweep covers) and 75 x 73, a
    sample of size 0, and one of mode 0 (JPEG: the raw gather leaves its row
    alone)."""
    dims = [(13, 10), (1, 1), (74, 74), (0, 0), (75, 73), (5, 4), (1, 1), (13, 10)]
    modes = [1, 1, 1, 1, 1, 0, 1, 1]
    table = np.zeros(len(dims), L.SAMPLE_DTYPE)
    off = residue
    for k, ((h, w), m) in enumerate(zip(dims, modes)):
        table[k] = (off, h * w * 3, max(h, 1), max(w, 1), m, 0)
        off += h * w * 3
    base = np.full(off + 7, 0xA5, np.uint8)
    base[residue:off] = rng.integers(0, 256, off - residue, dtype=np.uint8)
    return base, table


def test_gather_raw_mixed_samples_at_every_residue(hip_lib):
    rng = np.random.default_rng(3)
    for residue in LEADS:
        base, table = _raw_samples(residue, rng)
        stride = int(table['size'].max()) + 5
        assert stride == 74 * 74 * 3 + 5
        src = Guarded(base.size, 0, base)
        dst = Guarded(len(table) * stride, 15 - residue)
        d_table = _dev(table)
        rc = hip_lib.ffcv_gather_raw_batch(_stream(), src.ptr, d_table.data_ptr(), len(table), dst.ptr, stride)
        assert rc == 0, hip_lib.ffcv_last_error()
        got = dst.read().reshape(len(table), stride)
        src.assert_untouched()
        want = R.gather_raw_np(base, table, stride)
        assert (want[5] == 0xA5).all() and (want[3] == 0xA5).all() and (want[:, -5:] == 0xA5).all()
        bad = [k for k in range(len(table)) if not np.array_equal(got[k], want[k])]
        assert not bad, (residue, bad)


# -------------------------------------------------------- descriptor gather --
def test_gather_samples_with_ids_out_of_range(hip_lib):
    """300 random descriptors; ids with repeats, and n_table, n_table + 1,
    2^32 + 5 and 2^63 + 1, which give the documented empty JPEG descriptor
    (offset 0, size 0, 1 x 1, mode 0).  Batches around the 256 threads of a
    workgroup, forwards and backwards, the output inside guards."""
    rng = np.random.default_rng(4)
    n_table = 300
    table = rng.integers(0, 256, n_table * 32, dtype=np.uint8).view(L.SAMPLE_DTYPE)
    d_table = _dev(table)
    ids = rng.integers(0, n_table, 257).astype(np.uint64)
    ids[[10, 11]] = ids[[20, 21]]
    for pos, v in ((0, 2 ** 63 + 1), (3, n_table), (100, n_table + 1), (255, 2 ** 32 + 5), (256, n_table)):
        ids[pos] = v
    empty = np.zeros(1, L.SAMPLE_DTYPE)
    empty['height'] = empty['width'] = 1
    for order in (ids, ids[::-1].copy()):
        for batch in (0, 1, 255, 256, 257):
            for lead in (0, 8):
                d_ids = _dev(order[:max(batch, 1)])
                dst = Guarded(batch * 32, lead)
                rc = hip_lib.ffcv_gather_samples(_stream(), d_table.data_ptr(), n_table, d_ids.data_ptr(), batch,
                                                 dst.ptr)
                assert rc == 0, hip_lib.ffcv_last_error()
                got = dst.read().view(L.SAMPLE_DTYPE)
                sel = order[:batch]
                want = table[np.minimum(sel, n_table - 1).astype(np.int64)]
                want[sel >= n_table] = empty[0]
                assert (sel >= n_table).sum() >= (batch > 0)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (batch, lead)
    assert np.array_equal(d_table.cpu().numpy(), table.view(np.uint8).reshape(-1))


def test_cutout_translate_and_gathers_reject_before_a_launch(hip_lib):
    """What the entries' own argument checks refuse (FFCV_EINVAL), with the
    entry's name in the message and nothing written; an empty batch is fine."""
    lib = hip_lib
    imgs = np.random.default_rng(2).integers(0, 256, (2, 4, 5, 3), dtype=np.uint8)
    src, dst = Guarded(imgs.size, 0, imgs), Guarded(imgs.size, 0)
    yx = _dev(np.zeros((2, 2), np.int32))
    table = np.zeros(2, L.SAMPLE_DTYPE)
    table['size'], table['height'], table['width'], table['mode'] = 60, 4, 5, 1
    d_table, d_ids = _dev(table), _dev(np.zeros(2, np.uint64))
    s, i, o, y, t, d, f = _stream(), src.ptr, dst.ptr, yx.data_ptr(), d_table.data_ptr(), d_ids.data_ptr(), _fill3()
    for args in ((None, 2, 4, 5, y, 2, f), (i, 2, 4, 5, None, 2, f), (i, 2, 4, 5, y, 0, f), (i, 2, 4, 5, y, 5, f),
                 (i, 2, 5, 4, y, 5, f), (i, -1, 4, 5, y, 2, f)):
        assert lib.ffcv_cutout_batch(s, *args) == EINVAL and b'ffcv_cutout_batch' in lib.ffcv_last_error()
    for args in ((i, i, 2, 4, 5, y, 1, f), (None, o, 2, 4, 5, y, 1, f), (i, None, 2, 4, 5, y, 1, f),
                 (i, o, 2, 4, 5, None, 1, f), (i, o, 2, 4, 5, y, 1, None), (i, o, 2, 0, 5, y, 1, f),
                 (i, o, 2, 4, -1, y, 1, f), (i, o, 2, 4, 5, y, -1, f), (i, o, 2, 4, 5, y, 1 << 30, f),
                 (i, o, -1, 4, 5, y, 1, f)):
        assert lib.ffcv_translate_batch(s, *args) == EINVAL and b'ffcv_translate_batch' in lib.ffcv_last_error()
    for args in ((None, t, 2, o, 60), (i, None, 2, o, 60), (i, t, 2, None, 60), (i, t, 2, o, 0), (i, t, -1, o, 60)):
        assert lib.ffcv_gather_raw_batch(s, *args) == EINVAL and b'ffcv_gather_raw_batch' in lib.ffcv_last_error()
    for args in ((None, 2, d, 2, o), (t, 2, None, 2, o), (t, 2, d, 2, None), (t, 2, d, -1, o)):
        assert lib.ffcv_gather_samples(s, *args) == EINVAL and b'ffcv_gather_samples' in lib.ffcv_last_error()
    assert lib.ffcv_cutout_batch(s, i, 0, 4, 5, y, 2, f) == 0
    assert lib.ffcv_translate_batch(s, i, o, 0, 4, 5, y, 1, f) == 0
    assert lib.ffcv_gather_raw_batch(s, i, t, 0, o, 60) == 0
    assert lib.ffcv_gather_samples(s, t, 2, d, 0, o) == 0
    ch.cuda.synchronize()
    assert (dst.read() == 0xA5).all()
    src.assert_untouched()


# ----------------------------------------------- more images than grid rows --
BIG = 65537


def _translate_np_batch(imgs, yx, p, fill):
    """translate_np for a whole batch at once: the filled canvases with the
    images at offset p, then each image's window."""
    B, H, W = imgs.shape[:3]
    canvas = np.empty((B, H + 2 * p, W + 2 * p, 3), np.uint8)
    canvas[:] = np.asarray(fill, np.uint8)
    canvas[:, p:p + H, p:p + W] = imgs
    k = np.arange(B)[:, None, None]
    rows = yx[:, 0, None, None] + np.arange(H)[None, :, None]
    cols = yx[:, 1, None, None] + np.arange(W)[None, None]
    return canvas[k, rows, cols]


def test_flip_of_more_images_than_a_grid_has_rows(hip_lib):
    """65,537 images of 1 x 2 pixels: the entry launches them in slices."""
    rng = np.random.default_rng(6)
    imgs = rng.integers(0, 256, (BIG, 1, 2, 3), dtype=np.uint8)
    flags = rng.choice(np.array([0, 1, 255], np.uint8), BIG)
    flags[-2:] = (1, 0)
    src, dst = Guarded(imgs.size, 3, imgs), Guarded(imgs.size, 12)
    d_flags = _dev(flags)
    rc = hip_lib.ffcv_flip_batch(_stream(), src.ptr, dst.ptr, BIG, 1, 2, 3, d_flags.data_ptr())
    assert rc == 0, hip_lib.ffcv_last_error()
    got = dst.read().reshape(imgs.shape)
    src.assert_untouched()
    want = np.where((flags != 0)[:, None, None, None], imgs[:, :, ::-1], imgs)
    for k in (0, 1, 65534, 65535, 65536):
        assert np.array_equal(want[k], R.flip_np(imgs[k], flags[k]))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2, 3)))[:8]


def test_translate_of_more_images_than_a_grid_has_rows(hip_lib):
    rng = np.random.default_rng(7)
    imgs = rng.integers(0, 256, (BIG, 1, 2, 3), dtype=np.uint8)
    yx = rng.integers(0, 3, (BIG, 2)).astype(np.int32)          # padding 1
    yx[-2:] = ((1, 1), (1, 0))
    src, dst = Guarded(imgs.size, 5, imgs), Guarded(imgs.size, 10)
    d_yx = _dev(yx)
    rc = hip_lib.ffcv_translate_batch(_stream(), src.ptr, dst.ptr, BIG, 1, 2, d_yx.data_ptr(), 1, _fill3())
    assert rc == 0, hip_lib.ffcv_last_error()
    got = dst.read().reshape(imgs.shape)
    src.assert_untouched()
    want = _translate_np_batch(imgs, yx, 1, FILL)
    for k in list(range(40)) + [65534, 65535, 65536]:
        assert np.array_equal(want[k], translate_np(imgs[k], int(yx[k, 0]), int(yx[k, 1]), 1, FILL))
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2, 3)))[:8]


def test_gather_raw_of_more_samples_than_a_grid_has_rows(hip_lib):
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, 1 + 6 * BIG, dtype=np.uint8)
    table = np.zeros(BIG, L.SAMPLE_DTYPE)
    table['offset'] = 1 + 6 * np.arange(BIG, dtype=np.uint64)
    table['size'], table['height'], table['width'] = 6, 1, 2
    table['mode'] = rng.random(BIG) > 0.01
    table['mode'][-2:] = 1
    assert 100 < (table['mode'] == 0).sum() < 2000
    stride = 6 + 5
    src, dst = Guarded(base.size, 0, base), Guarded(BIG * stride, 7)
    d_table = _dev(table)
    rc = hip_lib.ffcv_gather_raw_batch(_stream(), src.ptr, d_table.data_ptr(), BIG, dst.ptr, stride)
    assert rc == 0, hip_lib.ffcv_last_error()
    got = dst.read().reshape(BIG, stride)
    src.assert_untouched()
    want = np.full((BIG, stride), 0xA5, np.uint8)
    want[:, :6] = np.where((table['mode'] == 1)[:, None], base[1:].reshape(BIG, 6), 0xA5)
    for k in (0, 65534, 65535, 65536):
        assert np.array_equal(want[k], R.gather_raw_np(base, table[k:k + 1], stride)[0])
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
