"""K1's decode extent (entropy_passes): the entropy decode stops at the linear
estimate of where the crop window's last MCU row ends, plus a margin, and
runs again over the whole stream when that prefix falls short.  Every crop
here is bit-exact against libjpeg-turbo's pixels (resize_crop of the whole
decode, as test_jpeg_container_gpu.py::test_rrc does it).

The extent the kernel used and whether the full-extent pass had to follow are
read from the debug words (slot 13: lanes | fell back << 8 | extent << 32);
what they must be comes from the host model (tools/sync_sim.c mode 13: the
stream's bits and the true end of every MCU row) and the margin constants of
jpeg_defs.h.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ffcv_amd.synthetic import natural_image, encode_jpeg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, CORRUPT = 0, 4  # FFCV_SAMPLE_* (include/ffcv_hip.h)
OUTS = [(32, 32), (17, 40)]
MAXB = 128


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch


def _margin():
    src = open(os.path.join(ROOT, 'ffcv_amd', 'csrc', 'jpeg_defs.h')).read()
    return tuple(int(re.search(r'^#define %s (\d+)' % n, src, re.M).group(1)) for n in ('K1_EXT_REL', 'K1_EXT_ABS'))


def _enc(img, q, sub):
    if sub == 'gray':
        return encode_jpeg(np.ascontiguousarray(img[:, :, 1]), q, '4:4:4')
    return encode_jpeg(img, q, sub)


def _mcu_h(sub):
    return {'4:2:0': 16, '4:2:2': 8, '4:4:4': 8, 'gray': 8}[sub]


def need_rows(sub, H, y, h):
    """MCU rows up to the last one that holds a block of the window of crop
    rows [y, y + h): parse_header's window (chroma of a vertically subsampled
    image takes one sample of fancy-upsampling context on each side)."""
    last = y + h - 1
    if sub != '4:2:0':
        return (last >> 3) + 1
    chroma = min((last >> 1) + 1, (H + 1) // 2 - 1)
    return max((last >> 3) >> 1, chroma >> 3) + 1


def extent(bits, mcuy, rows):
    """The extent entropy_passes lays its lane ranges over."""
    if rows == mcuy:
        return bits
    rel, ab = _margin()
    return min(bits, bits // mcuy * rows + (bits >> 8) * rel + ab)


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    """tools/sync_sim.c mode 13: (bits, mcuy, [bit where MCU row r ends])."""
    d = tmp_path_factory.mktemp('sim')
    exe = str(d / 'sync_sim')
    subprocess.run([os.environ.get('CC', 'cc'), '-O1', '-o', exe, os.path.join(ROOT, 'tools', 'sync_sim.c')], check=True)

    def rows(blob):
        f = str(d / 'x.jpg')
        np.asarray(blob).tofile(f)
        out = subprocess.run([exe, f, '64', '13'], check=True, capture_output=True, text=True).stdout
        head, tail = [l for l in out.splitlines() if l.startswith('rows:')][0].split('|')
        h = head.split()
        return int(h[2]), int(h[6]), [int(p.split(':')[1]) for p in tail.split()]
    return rows


@pytest.fixture(scope='module')
def ref(oracle):
    """libjpeg-turbo's pixels of a stream, decoded once."""
    cache = {}

    def get(blob):
        key = bytes(blob)
        if key not in cache:
            cache[key] = oracle.ljt_decode(blob)
        return cache[key]
    return get


def _run(items, crops, out_hw, dec=None, draw=None):
    """One RRC launch of items[k] = (name, blob, h, w) cropped to crops[k] =
    (y, x, h, w), or with draw = DrawParams the fused launch that draws them
    (sample ids 0..B-1): (status, pixels, debug words, crops)."""
    torch = _torch()
    from ffcv_amd import libffcv as L
    from ffcv_amd.libffcv import SAMPLE_DTYPE
    from ffcv_amd.synthetic import pack
    B = len(items)
    buf, offs, sizes = pack([it[1] for it in items])
    a = np.zeros(B, SAMPLE_DTYPE)
    a['offset'], a['size'] = offs, sizes
    a['height'], a['width'] = [it[2] for it in items], [it[3] for it in items]
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros(4096, np.uint8)])).to('cuda:0')
    d_smp = torch.from_numpy(a.view(np.uint8)).to('cuda:0')
    own = dec is None
    if own:
        dec = L.JpegDecoder(B, max(it[2] for it in items), max(it[3] for it in items), max(len(it[1]) for it in items))
    lib = L.lib()
    lib.ffcv_jpeg_set_debug.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    dbg = torch.zeros((B, 16), dtype=torch.int64, device='cuda:0')
    lib.ffcv_jpeg_set_debug(dec.handle, ctypes.c_void_p(dbg.data_ptr()))
    p = L.RRCParams()
    p.out_h, p.out_w = out_hw
    out = torch.full((B, out_hw[0], out_hw[1], 3), 7, dtype=torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    flips = torch.zeros(B, dtype=torch.uint8, device='cuda:0')
    if draw is None:
        d_crops = torch.from_numpy(np.ascontiguousarray(crops, np.int32)).to('cuda:0')
        dec.rrc(d_buf, d_smp, B, d_crops, None, flips, p, out, status)
    else:
        d_crops = torch.empty((B, 4), dtype=torch.int32, device='cuda:0')
        ids = torch.arange(B, dtype=torch.int64, device='cuda:0')
        dec.rrc_fused(d_buf, d_smp, ids, draw, d_crops, None, None, p, out, status)
    torch.cuda.synchronize()
    lib.ffcv_jpeg_set_debug(dec.handle, None)
    res = status.cpu().numpy(), out.cpu().numpy(), dbg.cpu().numpy().view(np.uint64), d_crops.cpu().numpy()
    if own:
        dec.close()
    return res


def _want(oracle, ref, items, crops, out_hw):
    return np.stack([oracle.resize_crop(ref(it[1]), y, y + h, x, x + w, *out_hw) for it, (y, x, h, w) in zip(items, crops)])


def _lanes(d):
    return d[:, 13] & 0xff


def _fell_back(d):
    return (d[:, 13] >> 8) & 1


def _ext(d):
    return d[:, 13] >> 32


def _check(oracle, ref, items, crops, out_hw):
    """Every crop OK and pixel-exact, in launches of MAXB; the debug words."""
    dbg = []
    bad = []
    for i in range(0, len(items), MAXB):
        its, cr = items[i:i + MAXB], crops[i:i + MAXB]
        st, got, d, _ = _run(its, cr, out_hw)
        want = _want(oracle, ref, its, cr, out_hw)
        for k, (it, c) in enumerate(zip(its, cr)):
            if st[k] != OK or not np.array_equal(got[k], want[k]):
                bad.append((it[0], c, int(st[k])))
        dbg.append(d)
    assert not bad, (len(bad), bad[:8])
    return np.concatenate(dbg)


# ---------------------------------------------------------------- boundary crops
def _boundary_rows(sub, H):
    """(y, h) row ranges around every MCU-row boundary of an image of H rows."""
    m = _mcu_h(sub)
    out = [(0, min(m, H)), (0, 1)]
    for r in range((H + m - 1) // m):
        top, last = r * m, min(r * m + m, H) - 1
        out += [(last, 1), (top, 1)]                      # one row: the MCU row's last, its first
        for end in (last - 1, last, last + 1):            # crops ending just before / on / after the boundary
            if 0 <= end < H:
                out.append((max(0, end - 19), end - max(0, end - 19) + 1))
                out.append((0, end + 1))
    out.append((H // 3, H - H // 3))                      # reaches the image's last row
    out.append((H - 1, 1))
    return sorted(set(out))


@pytest.fixture(scope='module')
def images():
    """[(name, blob, h, w, sub)]"""
    rng = np.random.default_rng(2110)
    out = []
    for h, w in [(48, 80), (56, 72)]:
        for sub in ('4:2:0', '4:4:4', 'gray'):
            out.append((f'nat {sub} {h}x{w}', _enc(natural_image(rng, h, w), 90, sub), h, w, sub))
    out.append(('nat 4:2:2 48x80', _enc(natural_image(rng, 48, 80), 90, '4:2:2'), 48, 80, '4:2:2'))
    out.append(('nat 4:2:0 200x256', _enc(natural_image(rng, 200, 256), 90, '4:2:0'), 200, 256, '4:2:0'))
    return out


@pytest.mark.parametrize('out_hw', OUTS, ids=['32x32', '17x40'])
def test_boundary_crops(hip_lib, oracle, ref, model, images, out_hw):
    items, crops, meta = [], [], []
    for name, blob, H, W, sub in images:
        bits, mcuy, ends = model(blob)
        assert mcuy == (H + _mcu_h(sub) - 1) // _mcu_h(sub)
        for n, (y, h) in enumerate(_boundary_rows(sub, H)):
            assert ends[need_rows(sub, H, y, h) - 1] <= extent(bits, mcuy, need_rows(sub, H, y, h)), (name, y, h)
            x, w = ((0, W), (W // 3, W // 2), (W - 9, 9))[n % 3]
            items.append((name, blob, H, W))
            crops.append((y, x, h, w))
            meta.append((bits, mcuy, need_rows(sub, H, y, h)))
    d = _check(oracle, ref, items, crops, out_hw)
    assert not _fell_back(d).any()  # natural content: the margin covers every prefix
    # the extent used: the whole stream exactly when no MCU row below the window is left unused
    big = [k for k, it in enumerate(items) if it[0] == 'nat 4:2:0 200x256']
    assert len(big) > 40 and (_lanes(d)[big] == 64).all()
    short = 0
    for k in range(len(items)):
        bits, mcuy, rows = meta[k]
        assert int(_ext(d)[k]) == extent(bits, mcuy, rows), (items[k][0], crops[k], int(_ext(d)[k]), bits, mcuy, rows)
        if k in big:
            assert (int(_ext(d)[k]) < bits) == (rows < mcuy), (crops[k], int(_ext(d)[k]), bits, rows, mcuy)
            short += rows < mcuy
    assert short > 20


# ---------------------------------------------------------------- fall-back
def _two_level(rng, h, w):
    return rng.choice(np.array([16, 239], np.uint8), size=(h, w, 3))


@pytest.fixture(scope='module')
def halves():
    """96 x 64, 4:2:0: noise over flat, and the same image upside down."""
    rng = np.random.default_rng(77)
    img = np.full((96, 64, 3), (90, 140, 60), np.uint8)
    img[:48] = _two_level(rng, 48, 64)
    return [('noise over flat', encode_jpeg(img, 90, '4:2:0'), 96, 64),
            ('flat over noise', encode_jpeg(np.ascontiguousarray(img[::-1]), 90, '4:2:0'), 96, 64)]


def test_fall_back_model(halves, model):
    """Host side: for the crops of test_fall_back the needed rows of the
    noise-over-flat image end far past estimate + margin (more than a symbol,
    at most 31 bits, so the kernel cannot complete them inside the extent),
    and those of its mirror image end inside it."""
    for (name, blob, H, W), short in zip(halves, (True, False)):
        bits, mcuy, ends = model(blob)
        assert mcuy == 6
        for h in (48, 58):
            rows = need_rows('4:2:0', H, 0, h)
            assert rows == 4
            e = extent(bits, mcuy, rows)
            print(name, 'bits', bits, 'rows', rows, 'true end', ends[rows - 1], 'extent', e)
            assert e < bits
            assert (ends[rows - 1] > e + 31) if short else (ends[rows - 1] <= e)


@pytest.mark.parametrize('out_hw', OUTS, ids=['32x32', '17x40'])
def test_fall_back(hip_lib, oracle, ref, halves, out_hw):
    items = [halves[0], halves[0], halves[1], halves[1]]
    crops = [(0, 0, 48, 64), (0, 0, 58, 64)] * 2
    d = _check(oracle, ref, items, crops, out_hw)
    assert list(_fell_back(d)) == [1, 1, 0, 0]
    assert _ext(d)[0] == _ext(d)[1] and _ext(d)[2] < _ext(d)[0]  # the whole stream after the fall-back


# ---------------------------------------------------------------- small streams
def test_small_streams(hip_lib, oracle, ref, model):
    rng = np.random.default_rng(8)
    items, crops = [], []
    for n in (8, 16):
        for sub in ('4:2:0', '4:4:4', 'gray'):
            for what, img in (('flat', np.full((n, n, 3), (200, 60, 120), np.uint8)), ('nat', natural_image(rng, n, n)),
                              ('noise', _two_level(rng, n, n))):
                for c in ((0, 0, min(n, 7), n), (1, 2, 3, 5)):
                    items.append((f'{what} {sub} {n}', _enc(img, 90, sub), n, n))
                    crops.append(c)
    bits = np.array([model(it[1])[0] for it in items])
    assert (bits <= 192).any() and ((bits > 300) & (bits < 192 * 64)).any()
    # what the kernel must lay its lanes over (the absolute margin covers most of these streams whole)
    ext = []
    for it, (y, x, h, w) in zip(items, crops):
        b, mcuy, ends = model(it[1])
        rows = need_rows(it[0].split()[1], it[2], y, h)
        e = extent(b, mcuy, rows)
        assert ends[rows - 1] <= e, it[0]  # none of them needs the fall-back
        ext.append(e)
    ext = np.array(ext)
    assert (ext == bits).sum() > len(items) // 2 and (ext < bits).any()
    for out_hw in OUTS:
        d = _check(oracle, ref, items, crops, out_hw)
        assert (_ext(d) == ext).all() and not _fell_back(d).any()
        assert (_lanes(d) == np.clip((ext + 191) // 192, 1, 64)).all()
        assert (_lanes(d) == 1).any() and ((_lanes(d) > 1) & (_lanes(d) < 64)).any()


# ---------------------------------------------------------------- entropy index
def test_entropy_index_keeps_full_extent(hip_lib, oracle, ref, model, images):
    """With an index attached a sample is decoded in full (the record holds
    the lane states of the full partition): the first epoch publishes, the
    second starts from the records; both are pixel-exact.  The same crops
    without an index stop early."""
    torch = _torch()
    from ffcv_amd import libffcv as L
    its = [(n, b, h, w) for n, b, h, w, _ in images]
    bits = [model(it[1])[0] for it in its]
    B = len(its)
    dp = L.DrawParams()
    dp.out_h, dp.out_w = OUTS[0]
    dp.scale[0], dp.scale[1] = 0.08, 0.3  # small crops: most windows end above the last MCU row
    dp.ratio[0], dp.ratio[1] = 0.75, 4 / 3
    dp.loader_seed = 11
    dp.epoch = 3
    index = torch.zeros((B, L.EIDX_LANES, L.EIDX_WORDS), dtype=torch.int32, device='cuda:0')
    dec = L.JpegDecoder(B, max(it[2] for it in its), max(it[3] for it in its), max(len(it[1]) for it in its))
    dec.set_entropy_index(index)
    want = crops = None
    for rnd in range(2):
        st, got, d, cr = _run(its, None, OUTS[0], dec=dec, draw=dp)
        if want is None:
            crops = [tuple(int(v) for v in c) for c in cr]
            want = _want(oracle, ref, its, crops, OUTS[0])
        assert (st == OK).all() and np.array_equal(got, want), rnd
        hit = d[:, 12] == np.uint64(0xFFFFFFFFFFFFFFFF)
        if rnd == 0:
            assert not hit.any() and index.cpu().numpy().any(axis=(1, 2)).all()  # published
            assert [int(e) for e in _ext(d)] == bits and not _fell_back(d).any()
        else:
            assert hit.all()
    dec.close()
    st, got, d, _ = _run(its, crops, OUTS[0])
    assert (st == OK).all() and np.array_equal(got, want)
    rows = [need_rows(im[4], im[2], c[0], c[2]) for im, c in zip(images, crops)]
    assert [int(e) for e in _ext(d)] == [extent(b, model(it[1])[1], r) for b, it, r in zip(bits, its, rows)]
    assert (_ext(d) < bits).sum() >= 2


# ---------------------------------------------------------------- damaged tail
def test_damaged_tail(hip_lib, oracle, ref, model):
    """A 64 x 80 stream cut in the middle of its last MCU row: a crop whose
    window ends above the damage is OK with libjpeg-turbo's pixels (it pads
    and goes on too); one that reaches the cut is OK with those pixels or
    CORRUPT with a zero row, as test_jpeg_container_gpu.py::test_alignment_sweep allows."""
    rng = np.random.default_rng(31)
    blob = encode_jpeg(natural_image(rng, 64, 80), 90, '4:2:0')
    bits, mcuy, ends = model(blob)
    assert mcuy == 4
    raw = bytes(blob)
    sos = raw.index(b'\xff\xda')
    scan = sos + 2 + ((raw[sos + 2] << 8) | raw[sos + 3])  # first entropy-coded byte
    # half-way into the last MCU row (stuffed bytes scale the de-stuffed position; checked below)
    cut = scan + (ends[2] + ends[3]) // 16 * (len(raw) - 2 - scan) // (bits // 8)
    short = blob[:cut]
    sbits, _, sends = model(short)
    assert len(sends) == 3 and sends == ends[:3] and ends[2] < sbits < ends[3]  # rows 0-2 whole, row 3 cut
    items = [('cut', short, 64, 80)] * 3
    crops = [(0, 0, 30, 80), (3, 5, 20, 40), (20, 0, 44, 80)]
    assert need_rows('4:2:0', 64, 0, 30) == 2 and need_rows('4:2:0', 64, 20, 44) == 4
    for out_hw in OUTS:
        st, got, d, _ = _run(items, crops, out_hw)
        want = _want(oracle, ref, items, crops, out_hw)
        assert st[0] == OK and st[1] == OK and st[2] in (OK, CORRUPT), st
        for k in range(3):
            if st[k] == OK:
                assert np.array_equal(got[k], want[k]), k
            else:
                assert not got[k].any(), k
