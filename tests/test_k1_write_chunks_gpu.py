"""K1's chunked write pass (write_range: a per-chunk part for block boundaries,
then K1_WCHUNK AC-only steps) on content built to stress it, bit for bit.

One image set serves every test: flat images (a chunk per block, most inner
steps idle, many blocks per lane), two-level noise at q100 (up to 63 AC steps
a block, coefficients staged below zigzag 24 and stored directly above),
checkerboards of flat and noise blocks / MCUs (1-step blocks beside 60-step
ones, lane boundaries inside long blocks), blocks with exactly C - 1, C, C + 1
and 2C AC steps (found with the host model, tools/sync_sim.c mode 12), and a
lone coefficient at zigzag 63 (ZRL runs).  Each at 4:2:0, 4:2:2, 4:4:4 and
greyscale, with streams below and above 1.5 KB (fewer than 64 lanes, and 64).

Pixels are compared with the project's oracle (libjpeg-turbo when present,
else the C restatement), coefficients with the CPU decoder.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from ffcv_amd.synthetic import natural_image, encode_jpeg, pack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBS = ['4:2:0', '4:2:2', '4:4:4', 'gray']
OUT = 32  # RRC output side


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch


def _chunk():
    src = open(os.path.join(ROOT, 'ffcv_amd', 'csrc', 'jpeg_defs.h')).read()
    return int(re.search(r'^#define K1_WCHUNK (\d+)', src, re.M).group(1))


def _enc(img, q, sub):
    if sub == 'gray':
        return encode_jpeg(np.ascontiguousarray(img[:, :, 1]), q, '4:4:4')
    return encode_jpeg(img, q, sub)


def _noise(rng, h, w):
    """Two-level noise at 16 / 239.  The full 0 / 255 swing is left out: on a
    few of its pixels libjpeg-turbo's 16-bit SIMD IDCT wraps where its own C
    form does not (9 of 36 such 56x72 images on the host), so the two forms of
    the oracle disagree there; test_content_is_what_it_claims holds them equal
    on every image used here."""
    return rng.choice(np.array([16, 239], np.uint8), size=(h, w, 3))


def _checker(rng, h, w, cell):
    img = np.full((h, w, 3), 90, np.uint8)
    n = _noise(rng, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((yy // cell + xx // cell) % 2).astype(bool)
    img[m] = n[m]
    return img


def _zz63(h, w):
    """Every 8x8 block is the (7, 7) DCT basis function: one coefficient at
    zigzag 63 after three ZRL symbols."""
    t = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    b = 128 + 100 * np.outer(t, t)
    img = np.tile(b, (h // 8, w // 8))
    return np.repeat(np.clip(np.rint(img), 0, 255).astype(np.uint8)[:, :, None], 3, 2)


@pytest.fixture(scope='module')
def model(tmp_path_factory):
    """tools/sync_sim.c mode 12: histogram of AC steps per block of a file."""
    d = tmp_path_factory.mktemp('sim')
    exe = str(d / 'sync_sim')
    subprocess.run([os.environ.get('CC', 'cc'), '-O1', '-o', exe, os.path.join(ROOT, 'tools', 'sync_sim.c')], check=True)

    def acsteps(blob):
        f = str(d / 'x.jpg')
        blob.tofile(f)
        out = subprocess.run([exe, f, '64', '12'], check=True, capture_output=True, text=True).stdout
        line = [l for l in out.splitlines() if l.startswith('acsteps:')][0]
        return {int(k): int(v) for k, v in (p.split(':') for p in line.split()[1:])}
    return acsteps


@pytest.fixture(scope='module')
def cases(model):
    """[(name, blob, h, w)], the same for every test."""
    rng = np.random.default_rng(1207)
    out = []
    C = _chunk()
    for sub in SUBS:
        for h, w in [(16, 16), (24, 40), (48, 40)]:
            out.append((f'flat {sub} {h}x{w}', _enc(np.full((h, w, 3), (200, 60, 120), np.uint8), 90, sub), h, w))
        for h, w in [(8, 8), (16, 16), (56, 72)]:
            out.append((f'noise {sub} {h}x{w}', _enc(_noise(rng, h, w), 100, sub), h, w))
        for cell in (8, 16):
            out.append((f'checker{cell} {sub}', _enc(_checker(rng, 64, 80, cell), 100, sub), 64, 80))
        out.append((f'zz63 {sub}', _enc(_zz63(48, 48), 90, sub), 48, 48))
        # blocks of exactly C - 1, C, C + 1 and 2C AC steps: natural content at
        # falling quality until the model has seen each count (asserted below)
        need = {C - 1, C, C + 1, 2 * C} - {0}
        for q in (90, 75, 60, 45, 30, 20, 12):
            if not need:
                break
            blob = _enc(natural_image(rng, 48, 64), q, sub)
            hist = model(blob)
            if need & set(hist):
                need -= set(hist)
                out.append((f'steps q{q} {sub}', blob, 48, 64))
        assert not need, f'{sub}: no block with {sorted(need)} AC steps'
    return out


def _dev_set(cases, reps=None):
    from ffcv_amd.libffcv import SAMPLE_DTYPE
    torch = _torch()
    blobs = [c[1] for c in cases]
    buf, offs, sizes = pack(blobs)
    idx = np.arange(len(cases)) if reps is None else np.asarray(reps)
    a = np.zeros(len(idx), SAMPLE_DTYPE)
    a['offset'] = offs[idx]
    a['size'] = sizes[idx]
    a['height'] = [cases[i][2] for i in idx]
    a['width'] = [cases[i][3] for i in idx]
    d_smp = torch.from_numpy(a.view(np.uint8)).to('cuda:0')
    return torch.from_numpy(buf).to('cuda:0'), d_smp


def _decoder(cases, batch):
    from ffcv_amd import libffcv as L
    return L.JpegDecoder(batch, max(c[2] for c in cases), max(c[3] for c in cases), max(len(c[1]) for c in cases))


def _pixels(oracle, blob):
    return oracle.ljt_decode(blob) if oracle.ljt() is not None else oracle.jpeg_decode(blob)


def test_content_is_what_it_claims(hip_lib, oracle, cases):
    """Host-side: stream sizes on both sides of 64 lanes, flat blocks of one AC
    step, noise blocks with staged and directly stored coefficients, the
    zigzag-63 blocks."""
    from ffcv_amd import libffcv as L
    stats = L.jpeg_scan_stats([c[1] for c in cases])
    ecs = stats[:, 2].astype(np.int64)
    assert (ecs > 0).all()
    for sub in SUBS:
        sel = np.array([sub in c[0] for c in cases])
        assert (ecs[sel] < 1536).any() and (ecs[sel] > 1536).any(), sub  # nthr = ceil(bits / 192) < 64 and = 64
    for (name, blob, h, w), st in zip(cases, stats):
        if oracle.ljt() is not None:  # one reference, whichever form of the oracle is present
            assert np.array_equal(oracle.ljt_decode(blob), oracle.jpeg_decode(blob)), name
        co = L.cpu_jpeg_coefficients(blob)
        assert len(co) == st[1]
        nz = (co[:, 1:] != 0).sum(1)
        if name.startswith('flat'):
            assert (nz == 0).all() and st[0] == 2 * st[1], name  # DC + EOB
        # 56 of 63 non-zero: more than the 23 staged positions, so some are stored directly
        if name.startswith('noise'):
            assert nz.max() >= 56, name
        if name.startswith('checker'):
            assert (nz == 0).any() and nz.max() >= 56, name
        if name.startswith('zz63'):
            one = (nz == 1) & (co[:, 63] != 0)
            assert one.any(), name


def test_full_decode(hip_lib, oracle, cases):
    torch = _torch()
    B = len(cases)
    d_buf, d_smp = _dev_set(cases)
    dec = _decoder(cases, B)
    stride = max(c[2] for c in cases) * max(c[3] for c in cases) * 3
    out = torch.zeros(B * stride, dtype=torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.decode(d_buf, d_smp, B, out, stride, status)
    torch.cuda.synchronize()
    st, o = status.cpu().numpy(), out.cpu().numpy()
    for k, (name, blob, h, w) in enumerate(cases):
        assert st[k] == 0, (name, st[k])
        got = o[k * stride:k * stride + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got, _pixels(oracle, blob)), name


def test_coefficients(hip_lib, oracle, cases):
    torch = _torch()
    from ffcv_amd import libffcv as L
    B = len(cases)
    d_buf, d_smp = _dev_set(cases)
    dec = _decoder(cases, B)
    want = [L.cpu_jpeg_coefficients(c[1]) for c in cases]
    maxb = max(len(x) for x in want) + 8
    out = torch.zeros((B, maxb, 64), dtype=torch.int16, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.coefficients(d_buf, d_smp, B, out, maxb, status)
    torch.cuda.synchronize()
    st, o = status.cpu().numpy(), out.cpu().numpy()
    for k, c in enumerate(cases):
        assert st[k] == 0, (c[0], st[k])
        assert np.array_equal(o[k, :len(want[k])], want[k]), c[0]
        assert not o[k, len(want[k]):].any(), c[0]


def _windows(h, w):
    """(y, x, h, w): the whole image, one MCU, windows on each edge, and one
    without the first and the last MCU row (lanes wholly outside it only carry
    DC sums) where the image has three 16-row bands."""
    ws = [(0, 0, h, w), (0, 0, min(16, h), min(16, w)), (0, 0, max(1, h // 2), w), (h - max(1, h // 3), 0, max(1, h // 3), w),
          (0, 0, h, max(1, w // 3)), (0, w - max(1, w // 2), h, max(1, w // 2))]
    if h >= 48:
        ws.append((16, 3, h - 32, w - 5))
    return ws


def test_rrc_windows(hip_lib, oracle, cases):
    torch = _torch()
    from ffcv_amd import libffcv as L
    reps, crops = [], []
    for i, (name, blob, h, w) in enumerate(cases):
        for win in _windows(h, w):
            reps.append(i)
            crops.append(win)
    assert any(c[0] == 16 for c in crops)
    crops = np.array(crops, np.int32)
    B = len(reps)
    d_buf, d_smp = _dev_set(cases, reps)
    dec = _decoder(cases, B)
    p = L.RRCParams()
    p.out_h, p.out_w = OUT, OUT
    out = torch.zeros((B, OUT, OUT, 3), dtype=torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    flips = torch.zeros(B, dtype=torch.uint8, device='cuda:0')
    dec.rrc(d_buf, d_smp, B, torch.from_numpy(crops).to('cuda:0'), None, flips, p, out, status)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all(), np.nonzero(status.cpu().numpy())
    want = oracle.rrc_batch([(cases[i][1], cases[i][2], cases[i][3], 0) for i in reps], crops, OUT, OUT)
    got = out.cpu().numpy()
    bad = np.argwhere((got != want).reshape(B, -1).any(1)).ravel()
    assert bad.size == 0, [(cases[reps[b]][0], tuple(crops[b])) for b in bad[:6]]


def test_rrc_entropy_index_twice(hip_lib, oracle, cases):
    """The fused RRC with the entropy index attached, twice: the second launch
    starts every lane from its record and runs the same write pass."""
    torch = _torch()
    import ctypes
    from ffcv_amd import libffcv as L
    n = len(cases)
    d_buf, d_table = _dev_set(cases)
    ids = torch.arange(n, dtype=torch.int64, device='cuda:0')
    dp = L.DrawParams()
    dp.out_h = dp.out_w = OUT
    dp.scale[0], dp.scale[1] = 0.08, 1.0
    dp.ratio[0], dp.ratio[1] = 0.75, 4 / 3
    dp.loader_seed = 11
    dp.epoch = 3
    rp = L.RRCParams()
    rp.out_h = rp.out_w = OUT
    dec = _decoder(cases, n)
    index = torch.zeros((n, L.EIDX_LANES, L.EIDX_WORDS), dtype=torch.int32, device='cuda:0')
    dec.set_entropy_index(index)
    lib = L.lib()
    lib.ffcv_jpeg_set_debug.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    dbg = torch.zeros((n, 16), dtype=torch.int64, device='cuda:0')
    lib.ffcv_jpeg_set_debug(dec.handle, ctypes.c_void_p(dbg.data_ptr()))
    want = None
    for rnd in range(2):
        crops = torch.empty((n, 4), dtype=torch.int32, device='cuda:0')
        out = torch.zeros((n, OUT, OUT, 3), dtype=torch.uint8, device='cuda:0')
        status = torch.full((n,), -1, dtype=torch.int32, device='cuda:0')
        dec.rrc_fused(d_buf, d_table, ids, dp, crops, None, None, rp, out, status)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all(), (rnd, np.nonzero(status.cpu().numpy()))
        hit = dbg[:, 12].cpu().numpy() == -1
        assert hit.all() if rnd else not hit.any(), rnd  # the index path on the second launch only
        if want is None:
            want = oracle.rrc_batch([(c[1], c[2], c[3], 0) for c in cases], crops.cpu().numpy(), OUT, OUT)
        got = out.cpu().numpy()
        bad = np.argwhere((got != want).reshape(n, -1).any(1)).ravel()
        assert bad.size == 0, (rnd, [cases[b][0] for b in bad[:6]])
    lib.ffcv_jpeg_set_debug(dec.handle, None)
