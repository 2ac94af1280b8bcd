"""Harness of tests/test_large_batch*.py: a device entry on a batch whose byte
offsets pass 2^31 and 2^32 and whose image count passes 65,535.

The large batch is a small one, tiled.  A period holds M distinct images and M
distinct rows of per-image parameters; image k of the batch is base[k % M] with
params[k % M], built on the device by repetition, and must come out as
want[k % M], which the entry's ``*_host`` twin (or, for the entries without
one, its numpy statement) computes once on the M images.  The comparison runs
on the device in chunks; the batch is never copied to the host.

What keeps the tiling from hiding a wrapped offset (check_conditions, run
without a device over every case by tests/test_large_batch.py):
  - neither 2^31 mod (M * img) nor 2^32 mod (M * img) is a multiple of img, so
    an offset that lost bit 31 or 32 lands inside another image of the period,
    never on a copy of the right one;
  - every expected image differs from its input and from the 0xA5 fill, and
    every apply flag is set: an image that was skipped, or run twice in place,
    cannot pass;
  - no two consecutive rows of parameters are equal (cyclically).
Only ffcv_amd.libffcv and the numpy statements of tests/ are used."""
import numpy as np

from ffcv_amd import libffcv as L
from tests import standalone_ref as R
from tests.translate_ref import translate_np

M = 251                       # images and parameter rows of a period: a prime
FILL_BYTE = 0xA5
GUARD = 4096
LIMITS = {'past_2g': 1 << 31, 'past_4g': 1 << 32}
SMALL = (61, 67)              # 12,261 bytes of u8 RGB: the many-images shape
STRIDE_BATCH, STRIDE_BYTES = 80, 64 << 20     # 79 * 64 MiB > 2^32
FILL = (9, 8, 7)
MIN_DEVICE_BYTES = 64 << 30
HUE_LDS_BYTES, TILE_PX = 16384, 4096      # ffcv_hue.hip; the *_TILE_PX of colour jitter, hue and tone


# ------------------------------------------------------------ arithmetic --
def batch_for(limit, img):
    """The smallest multiple of M whose bytes, at img bytes an image, exceed limit."""
    return (limit // (M * img) + 1) * M


def wrapped(k, img, bits):
    """Where image k's offset lands when it is kept in ``bits`` bits: the byte
    offset, the image of the batch it falls into and the offset inside it."""
    off = (k * img) & ((1 << bits) - 1)
    return off, off // img, off % img


def wrap_ok(img):
    return all((lim % (M * img)) % img != 0 for lim in LIMITS.values())


def odd_shape(min_bytes, bpp=3, also=()):
    """The first odd H x W (W = H + 2, then wider) of more than min_bytes bytes
    at bpp bytes a pixel for which wrap_ok holds at bpp and at every pixel size
    of ``also``."""
    h = int(np.sqrt(min_bytes / bpp)) | 1
    w = h + 2
    while h * w * bpp <= min_bytes or not all(wrap_ok(h * w * b) for b in (bpp,) + tuple(also)):
        w += 2
    return h, w


def cyc(n, a, b=0, m=M):
    """(a * i + b) % n for i < m: a sequence whose cyclic neighbours differ (a % n != 0)."""
    assert a % n != 0 and ((a * (m - 1) + b) % n) != b % n
    return (a * np.arange(m) + b) % n


class Built:
    """A period: base (M, src_img) and want (M, dst_img) uint8, the per-image
    parameters {name: (array, axis of the image index)}, the names of those
    that are apply flags, and whether the entry works in place."""

    def __init__(self, base, want, params=None, flags=(), inplace=False, shape=None, vary=None, **extra):
        self.base = np.ascontiguousarray(base).reshape(M, -1).view(np.uint8)
        self.want = np.ascontiguousarray(want).reshape(M, -1).view(np.uint8)
        self.params, self.flags, self.inplace, self.shape = dict(params or {}), tuple(flags), inplace, shape
        self.src_img, self.dst_img = self.base.shape[1], self.want.shape[1]
        self.extra = extra            # what the launch needs besides: tables, fills, output shapes
        # the parameters whose consecutive rows must differ: all but the apply flags
        self.vary = tuple(vary if vary is not None else [n for n in self.params if n not in self.flags])


def check_conditions(b):
    """The three conditions of the module docstring on a period."""
    assert wrap_ok(b.src_img) and wrap_ok(b.dst_img), (b.src_img, b.dst_img)
    for bits, lim in ((31, 1 << 31), (32, 1 << 32)):
        for img in (b.src_img, b.dst_img):
            k = lim // img + 1                      # the first image wholly past the limit
            off, at, inside = wrapped(k, img, bits)
            assert inside != 0 and off < k * img, (bits, img, k)
    assert not (b.want == FILL_BYTE).all(axis=1).any(), 'an expected image equals the fill'
    if b.src_img == b.dst_img:
        same = (b.want == b.base).all(axis=1)
        assert not same.any(), ('expected images equal to their input', np.flatnonzero(same)[:8])
    for name in b.flags:
        assert (b.params[name][0] != 0).all(), name
    rows = [np.ascontiguousarray(np.moveaxis(a, ax, 0)).reshape(M, -1).view(np.uint8).reshape(M, -1)
            for name, (a, ax) in b.params.items() if name in b.vary]
    if rows:
        rows = np.concatenate(rows, axis=1)
        eq = (rows == np.roll(rows, -1, axis=0)).all(axis=1)
        assert not eq.any(), ('equal consecutive parameter rows', np.flatnonzero(eq)[:8])


# ----------------------------------------------------------- device side --
def need_device():
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    total = torch.cuda.get_device_properties(0).total_memory
    if total < MIN_DEVICE_BYTES:
        pytest.skip(f'the device has {total >> 30} GiB of memory, less than the 64 GiB these batches are sized for')


class DevBuf:
    """nbytes device bytes ``lead`` bytes past GUARD bytes of 0xA5, with GUARD
    more behind; the allocation starts at a multiple of 16."""

    def __init__(self, nbytes, lead):
        import torch
        self.lo, self.n = GUARD + lead, int(nbytes)
        self.buf = torch.full((self.lo + self.n + GUARD,), FILL_BYTE, dtype=torch.uint8, device='cuda:0')
        assert self.buf.data_ptr() % 16 == 0
        self.flat = self.buf[self.lo:self.lo + self.n]

    def guards_ok(self):
        return bool((self.buf[:self.lo] == FILL_BYTE).all()) and bool((self.buf[self.lo + self.n:] == FILL_BYTE).all())


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to('cuda:0')      # a copy: the periods are read-only


def tile_bytes(flat, period, reps):
    """flat = period repeated reps times."""
    flat.view(reps, period.numel()).copy_(period.reshape(1, -1).expand(reps, -1))


def tile_param(a, axis, reps, batch=None):
    """A parameter array with its image axis repeated reps times (then cut to batch)."""
    t = dev(a)
    rep = [1] * t.dim()
    rep[axis] = reps
    t = t.repeat(*rep)
    if batch is not None:
        t = t.narrow(axis, 0, batch)
    return t.contiguous()


def differing(flat, want, reps, chunk_bytes=1 << 28):
    """(number of images of flat that differ from want[k % M], the first few k)."""
    import torch
    m, img = want.shape
    v = flat.view(reps, m, img)
    step = max(1, chunk_bytes // (m * img))
    total = torch.zeros((), dtype=torch.int64, device=flat.device)
    for r0 in range(0, reps, step):
        total += (v[r0:r0 + step] != want).any(dim=2).sum()
    n = int(total)
    first = []
    if n:
        for r0 in range(0, reps, step):
            ne = (v[r0:r0 + step] != want).any(dim=2).reshape(-1).nonzero().reshape(-1)
            first += (ne[:8] + r0 * m).tolist()
            if len(first) >= 8:
                break
    return n, first[:8]


def run_dense(case, built, limit):
    """The case's entry on the smallest tiled batch whose source AND destination
    bytes exceed limit; every check on the device."""
    import torch
    b = built
    batch = batch_for(limit, case.size_of(b))
    reps = batch // M
    sreps = reps + case.extra_periods
    src = DevBuf(sreps * M * b.src_img, case.lead[0])
    d_base, d_want = dev(b.base), dev(b.want)
    tile_bytes(src.flat, d_base, sreps)
    dst = src if b.inplace else DevBuf(batch * b.dst_img, case.lead[1])
    P = {name: tile_param(a, ax, reps) for name, (a, ax) in b.params.items()}
    try:
        case.launch(src.flat, dst.flat, batch, b, P, 0)
        torch.cuda.synchronize()
        assert src.guards_ok() and dst.guards_ok(), 'bytes outside the batch were written'
        if not b.inplace:
            n, first = differing(src.flat, d_base, sreps)
            assert n == 0, f'{n} source images were written, first {first}'
        n, first = differing(dst.flat, d_want, reps)
        assert n == 0, f'{n} of {batch} images differ, first {first}'
        case.after(b, P, batch)
    finally:
        del src, dst, P, d_base, d_want
        torch.cuda.empty_cache()


def run_strided(case, built):
    """80 images, the destination's 64 MiB apart: the last starts past 2^32."""
    import torch
    b = built
    batch, stride = STRIDE_BATCH, STRIDE_BYTES
    assert (batch - 1) * stride > 1 << 32
    src = DevBuf(M * b.src_img, case.lead[0])          # the whole period: a gather reads any of it
    src.flat.copy_(dev(b.base).reshape(-1))
    dst = DevBuf((batch - 1) * stride + b.dst_img, case.lead[1])
    P = {name: tile_param(a, ax, 1, batch) for name, (a, ax) in b.params.items()}
    d_want = dev(b.want[:batch])
    try:
        case.launch(src.flat if case.whole_source else src.flat[:batch * b.src_img], dst.flat, batch, b, P, stride)
        torch.cuda.synchronize()
        assert src.guards_ok() and dst.guards_ok(), 'bytes outside the batch were written'
        assert torch.equal(src.flat, dev(b.base).reshape(-1)), 'the source was written'
        bad = [k for k in range(batch)
               if not torch.equal(dst.flat[k * stride:k * stride + b.dst_img], d_want[k])]
        assert not bad, f'{len(bad)} of {batch} images differ, first {bad[:8]}'
        gaps = [k for k in range(batch - 1)
                if not bool((dst.flat[k * stride + b.dst_img:(k + 1) * stride] == FILL_BYTE).all())]
        assert not gaps, f'bytes between the images were written, behind image {gaps[:8]}'
        case.after(b, P, batch)
    finally:
        del src, dst, P, d_want
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ cases --
def _images(seed, h, w, c=3):
    return np.random.default_rng(seed).integers(0, 256, (M, h, w, c), dtype=np.uint8)


def _u8(flat, batch, h, w, c=3):
    return flat.view(batch, h, w, c)


class Case:
    """An entry: shapes() -> {regime: (H, W)}, build(H, W) -> Built on the host,
    launch(...) on device bytes.  strided: the entry takes a dst stride."""
    name = ''
    strided = False
    whole_source = False
    extra_periods = 0         # periods of source behind the batch (an entry with several sources)
    regimes = ('many', 'wide')
    lead = (5, 11)            # of the source and of the destination: odd byte offsets

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(65536)}     # past the 256 x 256 bytes one grid sweep covers

    def size_of(self, b):
        return min(b.src_img, b.dst_img)

    def after(self, b, P, batch):
        pass


class Cutout(Case):
    name = 'cutout_batch'

    def build(self, h, w):
        base = _images(1, h, w)
        yx = np.stack([cyc(h - 4, 7), cyc(w - 4, 3, 1)], 1).astype(np.int32)
        want = np.stack([R.cutout_np(base[i], int(yx[i, 0]), int(yx[i, 1]), 5, FILL) for i in range(M)])
        return Built(base, want, {'yx': (yx, 0)}, inplace=True, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.cutout_batch(_u8(src, batch, *b.shape), P['yx'], 5, FILL)


class Flip(Case):
    def __init__(self, cb):
        self.cb, self.name = cb, f'flip_batch[{cb}]'

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(65536, self.cb)} if wrap_ok(SMALL[0] * SMALL[1] * self.cb) else \
            {'many': odd_shape(SMALL[0] * SMALL[1] * self.cb - 1, self.cb), 'wide': odd_shape(65536, self.cb)}

    def build(self, h, w):
        base = _images(2 + self.cb, h, w, self.cb)
        flags = np.array([1, 255, 2], np.uint8)[np.arange(M) % 3]
        return Built(base, base[:, :, ::-1], {'flips': (flags, 0)}, flags=('flips',), shape=(h, w), vary=('flips',))

    def launch(self, src, dst, batch, b, P, stride):
        L.flip_batch(_u8(src, batch, *b.shape, self.cb), _u8(dst, batch, *b.shape, self.cb), P['flips'])


class Translate(Case):
    name = 'translate_batch'

    def build(self, h, w):
        base = _images(9, h, w)
        yx = np.stack([cyc(11, 7), cyc(11, 3, 1)], 1).astype(np.int32)
        yx[(yx == 5).all(axis=1), 1] = 6                       # (p, p) is the identity
        want = np.stack([translate_np(base[i], int(yx[i, 0]), int(yx[i, 1]), 5, FILL) for i in range(M)])
        return Built(base, want, {'yx': (yx, 0)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.translate_batch(_u8(src, batch, *b.shape), _u8(dst, batch, *b.shape), P['yx'], 5, FILL)


class Lut(Case):
    """out[i] = table[in[i] * 3 + i % 3]; the batch is sized by its ELEMENTS
    (the source's bytes), so the 2-byte table's output passes 2^33 bytes."""

    def __init__(self, elem):
        self.elem, self.name, self.lead = elem, f'lut_batch[{elem}]', (5, 10 if elem == 2 else 11)
        rng = np.random.default_rng(100 + elem)
        self.table = (np.stack([rng.permutation(256) for _ in range(3)], -1).astype(np.uint8) if elem == 1 else
                      rng.permutation(65536)[:768].astype(np.uint16).reshape(256, 3))

    regimes = ('many',)

    def shapes(self):
        return {'many': SMALL}

    def size_of(self, b):
        return b.src_img

    def build(self, h, w):
        base = _images(20 + self.elem, h, w)
        want = np.stack([R.lut_np(base[i], self.table) for i in range(M)])
        return Built(base, want, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        out = dst if self.elem == 1 else dst.view(torch.int16)
        L.lut_batch(src, dev(self.table), out)


SIGMA = (np.arange(M) + 100) % M      # a permutation of the period without a fixed point
assert (SIGMA != np.arange(M)).all() and np.unique(SIGMA).size == M


class GatherRows(Case):
    """Row k of the output is image k - k % M + SIGMA[k % M] of the source."""
    strided = True
    whole_source = True

    def __init__(self, side):
        self.side, self.name = side, f'gather_rows[{side}]'
        self.regimes = ('many',) if side == 'below' else ('wide',)

    def shapes(self):
        cut = L.gather_rows_cutover()
        if self.side == 'below':
            h, w = odd_shape(cut // 2)
            assert h * w * 3 < cut
            return {'many': (h, w)}
        return {'wide': odd_shape(cut)}

    def build(self, h, w):
        base = _images(30, h, w)
        return Built(base, base[SIGMA], {'sigma': (SIGMA.astype(np.int64), 0)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        img = b.src_img
        k = torch.arange(batch, device=src.device, dtype=torch.int64)
        ids = k - k % M + P['sigma']
        residue = src.data_ptr() % 16                      # base must be 16-byte aligned: the rows are not
        row_off = torch.arange(src.numel() // img, device=src.device, dtype=torch.int64) * img + residue
        status = torch.full((batch,), -1, dtype=torch.int32, device=src.device)
        base_ptr = src.data_ptr() - residue
        L.gather_rows(base_ptr, residue + src.numel(), row_off, ids, img, dst, stride or img, status)
        P['_status'] = status

    def after(self, b, P, batch):
        assert bool((P['_status'] == 0).all())


# ---- in place, a run of pixels per workgroup (lds_stage.h) ----------------
class ColorJitter(Case):
    """brightness, contrast, saturation: beyond the LDS regime the contrast
    step takes the per-image workspace."""
    name = 'color_jitter_batch'
    steps = (1, 2, 3)

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(L.color_jitter_lds_bytes())}

    def build(self, h, w):
        base = _images(40, h, w)
        apply = np.ones((3, M), np.uint8)
        ratio = np.stack([0.4 + cyc(97, 13, s) / 80.0 for s in range(3)]).astype(np.float64)
        want = L.color_jitter_batch_host(base.copy(), self.steps, apply, ratio)
        return Built(base, want, {'apply': (apply, 1), 'ratio': (ratio, 1)}, flags=('apply',), inplace=True,
                     shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        ws = torch.full((L.color_jitter_workspace_bytes(batch) // 8,), -1, dtype=torch.int64, device=src.device)
        L.color_jitter_batch(_u8(src, batch, *b.shape), self.steps, P['apply'], P['ratio'], ws)


class Hue(Case):
    name = 'hue_batch'

    def shapes(self):
        # HUE_LDS_BYTES has no query; the limits test pins it through the workgroup count the entry refuses
        return {'many': SMALL, 'wide': odd_shape(HUE_LDS_BYTES)}

    def build(self, h, w):
        base = _images(41, h, w)
        apply = np.ones(M, np.uint8)
        shift = (0.05 + cyc(89, 11) / 200.0) * np.where(np.arange(M) % 2, -1.0, 1.0)
        want = L.hue_batch_host(base.copy(), apply, shift)
        return Built(base, want, {'apply': (apply, 0), 'shift': (shift, 0)}, flags=('apply',), inplace=True,
                     shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.hue_batch(_u8(src, batch, *b.shape), P['apply'], P['shift'])


class Tone(Case):
    """posterize (bits per image), equalize, invert: beyond the LDS regime the
    equalize step takes the per-image workspace of 768 counters."""
    steps = (1, 3, 4)

    def __init__(self, bits):
        self.per_image, self.name = bits, 'tone_batch_bits' if bits else 'tone_batch'

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(L.tone_lds_bytes())}

    def build(self, h, w):
        base = _images(42, h, w)
        apply = np.ones((3, M), np.uint8)
        bits = (1 + cyc(7, 3)).astype(np.uint8)
        if self.per_image:
            want = L.tone_batch_bits_host(base.copy(), self.steps, apply, bits)
            params = {'apply': (apply, 1), 'bits': (bits, 0)}
        else:
            want = L.tone_batch_host(base.copy(), self.steps, 3, apply)
            params = {'apply': (apply, 1)}
        return Built(base, want, params, flags=('apply',), inplace=True, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        ws = torch.full((L.tone_workspace_bytes(batch) // 4,), -1, dtype=torch.int32, device=src.device)
        if self.per_image:
            L.tone_batch_bits(_u8(src, batch, *b.shape), self.steps, P['apply'], P['bits'], ws)
        else:
            L.tone_batch(_u8(src, batch, *b.shape), self.steps, 3, P['apply'], ws)


# ---- out of place with a dst stride (band_tiles.h, the affine tiles) ------
class Blur(Case):
    name = 'gaussian_blur_batch'
    strided = True
    ksize = 5

    def shapes(self):
        lds = L.gaussian_blur_lds_bytes()
        return {'many': odd_shape(lds // 15 * 3 // 2), 'wide': odd_shape(lds // 15 * 3)}

    def build(self, h, w):
        base = _images(50, h, w)
        apply = np.ones(M, np.uint8)
        sigma = 0.6 + cyc(83, 9) / 50.0
        j = np.arange(self.ksize) - (self.ksize - 1) / 2
        e = np.exp(-0.5 * (j[None] / sigma[:, None]) ** 2)
        weights = np.zeros((M, 32), np.float32)
        weights[:, :self.ksize] = (e / e.sum(1, keepdims=True)).astype(np.float32)
        want = L.gaussian_blur_batch_host(base, np.empty_like(base), self.ksize, apply, weights, nthreads=8)
        return Built(base, want, {'apply': (apply, 0), 'weights': (weights, 0)}, flags=('apply',), shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.gaussian_blur_batch(_u8(src, batch, *b.shape), dst, self.ksize, P['apply'], P['weights'], stride)


class Sharpness(Case):
    name = 'sharpness_batch'
    strided = True

    def shapes(self):
        lds = L.sharpness_lds_bytes()
        return {'many': odd_shape(lds // 6 * 3 // 2), 'wide': odd_shape(lds // 6 * 3)}

    def build(self, h, w):
        base = _images(51, h, w)
        apply = np.ones(M, np.uint8)
        factor = (1.5 + cyc(79, 5) / 20.0).astype(np.float32)
        want = L.sharpness_batch_host(base, np.empty_like(base), apply, factor, nthreads=8)
        return Built(base, want, {'apply': (apply, 0), 'factor': (factor, 0)}, flags=('apply',), shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.sharpness_batch(_u8(src, batch, *b.shape), dst, P['apply'], P['factor'], stride)


class Affine(Case):
    strided = True

    def __init__(self, mode):
        self.mode, self.name = mode, f'affine_batch[{("bilinear", "nearest")[mode]}]'

    def shapes(self):
        whole = L.affine_whole_bytes()
        return {'many': odd_shape(whole // 2), 'wide': odd_shape(whole)}

    def build(self, h, w):
        base = _images(52 + self.mode, h, w)
        apply = np.ones(M, np.uint8)
        ranges = (-30, 30, -4, 4, -4, 4, 0.8, 1.25, -10, 10, -10, 10)
        _, coef = L.affine_draw_batch_host(np.arange(M) + 1000, 3, 1, 1.0, ranges, h, w)
        want = L.affine_batch_host(base, np.empty_like(base), self.mode, FILL, apply, coef, nthreads=8)
        return Built(base, want, {'apply': (apply, 0), 'coef': (coef, 0)}, flags=('apply',), shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.affine_batch(_u8(src, batch, *b.shape), dst, self.mode, FILL, P['apply'], P['coef'], stride)


# ---- samples with a neighbour, boxes, membership ---------------------------
class Mixup(Case):
    """Every period is one batch of M samples: sample i mixes with i - 1, the
    period's first with its last, as in the M samples of the host twin."""

    def __init__(self, dtype):
        self.dtype, self.name = np.dtype(dtype), f'mixup_batch[{np.dtype(dtype).name}]'
        self.lead = (12, 4) if self.dtype == np.float32 else (5, 11)

    def shapes(self):
        bpp = 3 * self.dtype.itemsize
        return {'many': odd_shape(SMALL[0] * SMALL[1] * bpp - 1, bpp), 'wide': odd_shape(65536 * self.dtype.itemsize, bpp)}

    def build(self, h, w):
        base = _images(60, h, w)
        if self.dtype == np.float32:
            base = (base.astype(np.float32) - 128) / 64
        lam = 0.2 + cyc(61, 9) / 100.0
        want = L.mixup_batch_host(base, np.empty_like(base), lam, M, False, nthreads=8)
        return Built(base, want, {'lam': (lam, 0)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        if self.dtype == np.float32:
            src, dst = src.view(torch.float32), dst.view(torch.float32)
        L.mixup_batch(src.view(batch, *b.shape, 3), dst.view(batch, *b.shape, 3), P['lam'], M, False)


def _boxes(h, w, second_is_size):
    y, x = cyc(h // 2, 5), cyc(w // 2, 3, 1)
    bh, bw = 3 + cyc(h // 3, 2), 3 + cyc(w // 3, 4)
    return np.stack([y, x, bh if second_is_size else y + bh, bw if second_is_size else x + bw], 1).astype(np.int32)


class CutMix(Case):
    """layout: 'u8' (NHWC, 3-byte pixels), 'f16' (NHWC fp16: 6-byte pixels, at
    an odd byte offset, since the bytes are only moved), 'chw' (3 planes)."""

    def __init__(self, layout):
        self.layout, self.name = layout, f'cutmix_batch[{layout}]'
        self.bpp = 6 if layout == 'f16' else 3

    def shapes(self):
        return {'many': odd_shape(SMALL[0] * SMALL[1] * self.bpp - 1, self.bpp), 'wide': odd_shape(65536, self.bpp)}

    def dims(self, h, w):
        return (3, h, w) if self.layout == 'chw' else (h, w, self.bpp)

    def build(self, h, w):
        base = np.random.default_rng(61).integers(0, 256, (M,) + self.dims(h, w), dtype=np.uint8)
        boxes = _boxes(h, w, False)
        lay = 'chw' if self.layout == 'chw' else 'hwc'
        want = L.cutmix_batch_host(base, np.empty_like(base), boxes, M, False, layout=lay, nthreads=8)
        return Built(base, want, {'boxes': (boxes, 0)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        d = (batch,) + self.dims(*b.shape)
        L.cutmix_batch(src.view(d), dst.view(d), P['boxes'], M, False, layout='chw' if self.layout == 'chw' else 'hwc')


class Erase(Case):
    """'u8' / 'f16' / 'chw': a constant fill in cutmix's layouts; 'pixel' /
    'pixel16': the per-element noise of 1- and 2-byte elements."""

    def __init__(self, kind):
        self.kind, self.name = kind, f'erase_batch[{kind}]'
        self.bpp = 6 if kind in ('f16', 'pixel16') else 3
        self.lead = (6, 6) if kind == 'pixel16' else (5, 11)
        self.table = np.random.default_rng(62).integers(
            0, 65536, L.ERASE_TABLE).astype(np.uint16 if kind == 'pixel16' else np.uint8)

    shapes = CutMix.shapes

    def dims(self, h, w):
        if self.kind == 'pixel16':
            return (h, w, 3)
        return (3, h, w) if self.kind == 'chw' else (h, w, self.bpp)

    def build(self, h, w):
        rng = np.random.default_rng(63)
        noise = self.kind.startswith('pixel')
        if self.kind == 'pixel16':
            base = rng.integers(0, 65536, (M, h, w, 3)).astype(np.uint16)
        else:
            base = rng.integers(0, 256, (M,) + self.dims(h, w), dtype=np.uint8)
        boxes = _boxes(h, w, True)
        keys = rng.integers(1, 1 << 62, M).astype(np.uint64)
        fill = self.table if noise else np.arange(1, 1 + self.bpp, dtype=np.uint8)   # planes x pixel_bytes
        lay = 'chw' if self.kind == 'chw' else 'hwc'
        want = L.erase_batch_host(base.copy(), boxes, fill, keys if noise else None, layout=lay, nthreads=8)
        params = {'boxes': (boxes, 0)}
        if noise:
            params['keys'] = (keys.view(np.int64), 0)
        return Built(base, want, params, inplace=True, shape=(h, w), fill=fill)

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        if self.kind == 'pixel16':
            src = src.view(torch.int16)
        L.erase_batch(src.view((batch,) + self.dims(*b.shape)), P['boxes'], dev(b.extra['fill']), P.get('keys'),
                      layout='chw' if self.kind == 'chw' else 'hwc')


class Poison(Case):
    """Every sample's id is in the set; the ids of a period are distinct."""
    name = 'poison_batch'

    def build(self, h, w):
        base = _images(64, h, w)
        rng = np.random.default_rng(65)
        ids = np.sort(rng.choice(1 << 40, M, replace=False)).astype(np.uint64)
        sample_ids = ids[SIGMA].astype(np.int64)
        alpha = rng.random(h * w * 3) * 0.8 + 0.1
        keep, add = 1.0 - alpha, rng.integers(0, 256, h * w * 3).astype(np.float64) * alpha
        want = L.poison_batch_host(base.copy(), sample_ids, ids, keep, add, nthreads=8)
        return Built(base, want, {'sample_ids': (sample_ids, 0)}, inplace=True, shape=(h, w), ids=ids, keep=keep,
                     add=add)

    def launch(self, src, dst, batch, b, P, stride):
        e = b.extra
        L.poison_batch(_u8(src, batch, *b.shape), P['sample_ids'], dev(e['ids'].view(np.int64)), dev(e['keep']),
                       dev(e['add']))


# ---- samples addressed through a table; the fused policies; the resize ----
def _sample_table(src, batch, b, P):
    """device ffcv_sample[batch]: sample k is image k - k % M + SIGMA[k % M] of src, raw."""
    import torch
    h, w = b.shape
    k = torch.arange(batch, device=src.device, dtype=torch.int64)
    t = torch.empty((batch, 4), dtype=torch.int64, device=src.device)
    t[:, 0] = (k - k % M + P['sigma']) * b.src_img
    t[:, 1] = b.src_img
    t[:, 2] = h | (w << 32)
    t[:, 3] = 1
    return t


class GatherRaw(Case):
    name = 'gather_raw_batch'
    strided = True
    whole_source = True

    def build(self, h, w):
        base = _images(31, h, w)
        return Built(base, base[SIGMA], {'sigma': (SIGMA.astype(np.int64), 0)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.gather_raw_batch(src, _sample_table(src, batch, b, P), batch, dst, stride or b.src_img)


class SimpleAug(Case):
    """flip, translate, cutout in one launch, to uint8 or through the fp16 table."""
    strided = True
    whole_source = True

    def __init__(self, lut):
        self.lut, self.name, self.lead = lut, f'simple_aug_batch[{"f16" if lut else "u8"}]', (5, 10 if lut else 11)
        self.table = np.random.default_rng(32).permutation(65536)[:768].astype(np.uint16).reshape(256, 3)

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(65536, 3, (6,))}

    def size_of(self, b):
        return b.src_img

    def build(self, h, w):
        base = _images(33, h, w)
        flips = np.array([1, 255, 2], np.uint8)[np.arange(M) % 3]
        tyx = np.stack([cyc(11, 7), cyc(11, 3, 1)], 1).astype(np.int32)
        cyx = np.stack([cyc(h - 4, 5), cyc(w - 4, 9, 2)], 1).astype(np.int32)
        want = []
        for i in range(M):
            x = R.flip_np(base[SIGMA[i]], 1)
            x = translate_np(x, int(tyx[i, 0]), int(tyx[i, 1]), 5, FILL)
            x = R.cutout_np(x, int(cyx[i, 0]), int(cyx[i, 1]), 5, (1, 2, 3))
            want.append(R.lut_np(x, self.table).reshape(h, w, 3) if self.lut else x)
        params = {'sigma': (SIGMA.astype(np.int64), 0), 'flips': (flips, 0), 'tyx': (tyx, 0), 'cyx': (cyx, 0)}
        return Built(base, np.stack(want), params, flags=('flips',), shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        p = L.SimpleAugParams()
        p.n_steps, p.padding, p.cutout_size = 3, 5, 5
        p.steps[:3] = (L.AUG_FLIP, L.AUG_TRANSLATE, L.AUG_CUTOUT)
        p.translate_fill[:3], p.cutout_fill[:3] = FILL, (1, 2, 3)
        L.simple_aug_batch(src, _sample_table(src, batch, b, P), batch, *b.shape, p, P['flips'], P['cyx'], P['tyx'],
                           dev(self.table) if self.lut else None, dst, stride)


class RrcImages(Case):
    """A crop of nearly the whole image, two pixels a side smaller at three
    origins, reduced by INTER_AREA to a slightly smaller output."""
    name = 'rrc_images_batch'
    strided = True

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(L.rrc_images_lds_bytes())}

    @staticmethod
    def out_shape(h, w):
        oh, ow = h - 4, w - 6
        while not wrap_ok(oh * ow * 3):
            ow -= 2
        return oh, ow

    def build(self, h, w):
        base = _images(34, h, w)
        crops = np.stack([cyc(3, 1), cyc(3, 2, 1), np.full(M, h - 2), np.full(M, w - 2)], 1).astype(np.int32)
        oh, ow = self.out_shape(h, w)
        want = L.rrc_images_batch_host(base, crops, np.empty((M, oh, ow, 3), np.uint8), nthreads=8)
        return Built(base, want, {'crops': (crops, 0)}, shape=(h, w), out=(oh, ow))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        h, w = b.shape
        p = L.RRCParams()
        p.out_h, p.out_w = b.extra['out']
        p.out_stride = stride
        nws = L.rrc_images_workspace_bytes(batch, h, w, p.out_h, p.out_w)
        ws = torch.empty((nws,), dtype=torch.uint8, device=src.device) if nws else None
        P['_status'] = torch.full((batch,), -1, dtype=torch.int32, device=src.device)
        L.rrc_images_batch(src, b.src_img, batch, h, w, P['crops'], None, None, p, dst, P['_status'], ws)

    def after(self, b, P, batch):
        assert bool((P['_status'] == 0).all())


class RrcRaw(RrcImages):
    """ffcv_rrc_raw_batch_ws on raw samples addressed through a table (sample k
    is image k - k % M + SIGMA[k % M]), to uint8 or through the fp16 table;
    the resize is rrc_images_batch_host's.  The 'many' batches hold more
    images than a grid has rows, which the entry launches in slices."""

    def __init__(self, lut):
        self.lut, self.name, self.lead = lut, f'rrc_raw_batch[{"f16" if lut else "u8"}]', (5, 10 if lut else 11)
        self.table = np.random.default_rng(38).permutation(65536)[:768].astype(np.uint16).reshape(256, 3)

    whole_source = True

    def shapes(self):
        return {'many': SMALL, 'wide': odd_shape(65536)}

    @staticmethod
    def out_shape(h, w):
        oh, ow = h - 4, w - 6
        while not (wrap_ok(oh * ow * 3) and wrap_ok(oh * ow * 6)):
            ow -= 2
        return oh, ow

    def build(self, h, w):
        base = _images(39, h, w)
        crops = np.stack([cyc(3, 1), cyc(3, 2, 1), np.full(M, h - 2), np.full(M, w - 2)], 1).astype(np.int32)
        oh, ow = self.out_shape(h, w)
        want = L.rrc_images_batch_host(np.ascontiguousarray(base[SIGMA]), crops, np.empty((M, oh, ow, 3), np.uint8),
                                       nthreads=8)
        if self.lut:
            want = np.stack([R.lut_np(x, self.table).reshape(oh, ow, 3) for x in want])
        return Built(base, want, {'crops': (crops, 0), 'sigma': (SIGMA.astype(np.int64), 0)}, shape=(h, w),
                     out=(oh, ow))

    def launch(self, src, dst, batch, b, P, stride):
        import torch
        p = L.RRCParams()
        p.out_h, p.out_w = b.extra['out']
        p.out_stride = stride
        d_table = dev(self.table) if self.lut else None
        p.lut = d_table.data_ptr() if self.lut else None
        ws = torch.empty((L.rrc_raw_workspace_bytes(batch, p.out_h, p.out_w),), dtype=torch.uint8, device=src.device)
        L.rrc_raw_batch(src, _sample_table(src, batch, b, P), batch, P['crops'], None, None, p, dst, workspace=ws)

    def after(self, b, P, batch):
        pass


CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)    # the programs of a policy slot


def _host_slots(imgs, d, slots, mode):
    """The slots' host twins one after the other, as the unfused transform runs them."""
    cur = imgs.copy()
    for s in slots:
        a, nxt = L.randaugment_slot(d, s), np.full_like(cur, FILL_BYTE)
        L.color_jitter_batch_host(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
        L.color_jitter_batch_host(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
        L.tone_batch_bits_host(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'])
        L.affine_batch_host(cur, nxt, mode, FILL, a['aff_apply'], a['aff_coef'], nthreads=8)
        L.sharpness_batch_host(cur, nxt, a['sharp_apply'], a['sharp_factor'], nthreads=8)
        cur = nxt
    return cur


def _pick(d, want, base):
    """M of the candidates, in order: each changes its image, and its row of
    draws differs from the one picked before it (and the last from the first)."""
    ax = {n: 2 if n in ('cj_apply', 'cj_ratio', 'tone_apply') else 1 for n in d}     # the image axis: [slot][row][k]
    rows = np.concatenate([np.ascontiguousarray(np.moveaxis(a, ax[n], 0)).reshape(len(base), -1).view(np.uint8)
                           for n, a in d.items()], axis=1)
    keep = []
    for i in range(len(base)):
        if (want[i] == base[i]).all() or (keep and (rows[i] == rows[keep[-1]]).all()):
            continue
        if len(keep) == M - 1 and (rows[i] == rows[keep[0]]).all():
            continue
        keep.append(i)
        if len(keep) == M:
            break
    assert len(keep) == M
    keep = np.array(keep)
    return {n: (np.ascontiguousarray(np.take(a, keep, axis=ax[n])), ax[n]) for n, a in d.items()}, want[keep], base[keep]


class RandAugment(Case):
    """Two slots a sample; the draws are the host draw's own, of 2 M candidate
    ids, from which _pick takes a period."""

    def __init__(self, large):
        self.large = large
        self.name = 'randaugment_large_batch' if large else 'randaugment_batch'
        self.regimes = ('wide',) if large else ('many',)

    def shapes(self):
        lds = L.randaugment_lds_bytes()
        assert 6 * SMALL[0] * SMALL[1] <= lds
        h, w = odd_shape(lds // 2)
        assert 6 * h * w > lds and L.randaugment_large_fits(h, w)
        return {'many': SMALL, 'wide': (h, w)}

    def build(self, h, w):
        from tests import randaugment_ref as RA
        cand = np.random.default_rng(35).integers(0, 256, (2 * M, h, w, 3), dtype=np.uint8)
        d = L.randaugment_draw_batch_host(np.arange(2 * M) + 500, 11, 1, 2, 31, 9, RA.values(31, h, w), h, w)
        params, want, base = _pick(d, _host_slots(cand, d, range(2), 0), cand)
        return Built(base, want, params, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        fn = L.randaugment_large_batch if self.large else L.randaugment_batch
        fn(_u8(src, batch, *b.shape), _u8(dst, batch, *b.shape), 2, 0, FILL, P)


def _augmix_draws(h, w, n):
    from tests import augmix_ref as AM
    return L.augmix_draw_batch_host(np.arange(n) + 900, 11, 1, 7, 3, -1, 1.0, True, AM.values(h, w), h, w)


class AugMix(Case):
    """Three chains and the mix in one launch."""
    name = 'augmix_batch'
    regimes = ('many',)

    def shapes(self):
        lds = L.augmix_lds_bytes()
        many = SMALL if 9 * SMALL[0] * SMALL[1] <= lds else odd_shape(lds // 9 * 3 // 2)
        assert 9 * many[0] * many[1] <= lds
        return {'many': many}

    def build(self, h, w):
        cand = np.random.default_rng(36).integers(0, 256, (2 * M, h, w, 3), dtype=np.uint8)
        d = _augmix_draws(h, w, 2 * M)
        results = [_host_slots(cand, d, range(3 * i, 3 * i + 3), 0) for i in range(3)]
        want = L.augmix_mix_batch_host(cand, results, d['weights'], np.empty_like(cand), nthreads=8)
        params, want, base = _pick(d, want, cand)
        return Built(base, want, params, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        L.augmix_batch(_u8(src, batch, *b.shape), _u8(dst, batch, *b.shape), 3, 0, FILL, P)


class AugMixMix(Case):
    """The mix alone, width 3: result i of image k is image k + i + 1 of the
    source, which holds one period more than the batch."""
    name = 'augmix_mix_batch'
    extra_periods = 1

    def build(self, h, w):
        base = _images(37, h, w)
        weights = np.ascontiguousarray(_augmix_draws(h, w, 2 * M)['weights'][:, ::2])
        results = [np.ascontiguousarray(np.roll(base, -(i + 1), axis=0)) for i in range(3)]
        want = L.augmix_mix_batch_host(base, results, weights, np.empty_like(base), nthreads=8)
        return Built(base, want, {'weights': (weights, 1)}, shape=(h, w))

    def launch(self, src, dst, batch, b, P, stride):
        img = b.src_img
        view = lambda i: _u8(src[i * img:(i + batch) * img], batch, *b.shape)     # noqa: E731
        L.augmix_mix_batch(view(0), [view(1), view(2), view(3)], P['weights'], _u8(dst, batch, *b.shape))


CASES = [Cutout(), Flip(1), Flip(2), Flip(6), Translate(), Lut(1), Lut(2), GatherRows('below'), GatherRows('above'),
         ColorJitter(), Hue(), Tone(False), Tone(True), Blur(), Sharpness(), Affine(0), Affine(1),
         Mixup(np.uint8), Mixup(np.float32), CutMix('u8'), CutMix('f16'), CutMix('chw'),
         Erase('u8'), Erase('f16'), Erase('chw'), Erase('pixel'), Erase('pixel16'), Poison(),
         GatherRaw(), SimpleAug(False), SimpleAug(True), RrcImages(), RrcRaw(False), RrcRaw(True), RandAugment(False), RandAugment(True),
         AugMix(), AugMixMix()]


BY_NAME = {c.name: c for c in CASES}
DENSE = [(c.name, regime, lim) for c in CASES for regime in c.regimes for lim in LIMITS]
STRIDED = [(c.name, c.regimes[-1]) for c in CASES if c.strided]

_built = {}


def built(name, regime):
    """The period of a case at a regime's shape, computed once and left unchanged."""
    if (name, regime) not in _built:
        c = BY_NAME[name]
        b = c.build(*c.shapes()[regime])
        b.base.setflags(write=False)
        b.want.setflags(write=False)
        _built[name, regime] = b
    return _built[name, regime]
