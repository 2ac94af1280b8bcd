"""K1, K1b and K2 on JPEG container layouts Pillow never writes, bit for bit
against libjpeg-turbo (tests/jpeg_surgery.py builds them; the CPU side is
tests/test_jpeg_container.py).

What the suite's Pillow streams never reach: header bytes past the 2048 K1
stages in LDS (tables, SOS and DQT read from global memory, also as the
workgroup's shared tables), every alignment of the sample and of the scan in
the de-stuffing pass, LUT-less table slots (a third AC table, six slots),
table ids 2 / 3 and tables defined twice or unused, 16-bit and merged DQT /
DHT segments, fill bytes, COM / APPn, SOF1, DRI 0, RGB colour spaces (Adobe
transform 0, ids R G B), grey with sampling factors, and the 4:4:0, 4:1:1
and 1x4 layouts with dimensions off the MCU grid; then the streams
libjpeg-turbo rejects, beside good ones.

Samples lie at chosen byte offsets, back to back as in a .beton (no
alignment between them), and the buffer ends with 4 KB of zeros, so that no
header read of a malformed sample can leave the allocation.
"""
import numpy as np
import pytest

from tests import jpeg_surgery as J
from tests.test_kernels_gpu import _oracle_post

pytestmark = pytest.mark.gpu

OK, BAD_MARKER, UNSUPPORTED, CORRUPT = 0, 1, 2, 4  # FFCV_SAMPLE_* (include/ffcv_hip.h)
MAXB = 96                   # images per launch
OUTS = [(32, 32), (17, 40)]  # RRC outputs
CUT, FILL = 8, (124, 116, 103)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch


# ---------------------------------------------------------------- packing
def _place(blobs, residues, tail=4096):
    """One buffer with sample k at the next offset that is residues[k] mod 8,
    and `tail` zero bytes after the last one."""
    offs, pos = [], 0
    for b, r in zip(blobs, residues):
        pos += (r - pos) % 8
        offs.append(pos)
        pos += len(b)
    buf = np.zeros(pos + tail, np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = b
    return buf, np.array(offs, np.uint64)


def _dev_set(items, residues=None):
    """items: [(name, blob, h, w)].  Device buffer and ffcv_sample array."""
    from ffcv_amd.libffcv import SAMPLE_DTYPE
    torch = _torch()
    if residues is None:
        residues = [(3 * k + 1) % 8 for k in range(len(items))]
    buf, offs = _place([it[1] for it in items], residues)
    assert not buf[-4096:].any()
    a = np.zeros(len(items), SAMPLE_DTYPE)
    a['offset'] = offs
    a['size'] = [len(it[1]) for it in items]
    a['height'] = [it[2] for it in items]
    a['width'] = [it[3] for it in items]
    return torch.from_numpy(buf).to('cuda:0'), torch.from_numpy(a.view(np.uint8)).to('cuda:0')


def _decoder(items, batch):
    from ffcv_amd import libffcv as L
    return L.JpegDecoder(batch, max(it[2] for it in items), max(it[3] for it in items), max(len(it[1]) for it in items))


def _chunks(seq, n=MAXB):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


# ---------------------------------------------------------------- launches
def _decode(items, residues=None):
    """(status, [pixels (h, w, 3) of every image]) of one full-decode launch."""
    torch = _torch()
    B = len(items)
    assert B <= MAXB
    d_buf, d_smp = _dev_set(items, residues)
    dec = _decoder(items, B)
    stride = max(it[2] * it[3] for it in items) * 3
    out = torch.full((B * stride,), 7, dtype=torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.decode(d_buf, d_smp, B, out, stride, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    dec.close()
    return status.cpu().numpy(), [o[k * stride:k * stride + it[2] * it[3] * 3].reshape(it[2], it[3], 3)
                                  for k, it in enumerate(items)]


def _coefficients(items, nblocks, residues=None):
    """(status, int16 (B, maxb, 64)) of one coefficient launch."""
    torch = _torch()
    B = len(items)
    assert B <= MAXB
    d_buf, d_smp = _dev_set(items, residues)
    dec = _decoder(items, B)
    maxb = max(nblocks) + 8
    out = torch.full((B, maxb, 64), 7, dtype=torch.int16, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.coefficients(d_buf, d_smp, B, out, maxb, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    dec.close()
    return status.cpu().numpy(), o


def _lut(oracle):
    return oracle.normalize_lut(np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255)


def _rrc(oracle, items, crops, out_hw, post):
    """(status, output, flips, cut) of one RRC launch of items[k] cropped to
    crops[k] = (y, x, h, w); post: with the fp16 LUT, cutout and flips."""
    torch = _torch()
    from ffcv_amd import libffcv as L
    B = len(items)
    assert B <= MAXB
    OH, OW = out_hw
    d_buf, d_smp = _dev_set(items)
    dec = _decoder(items, B)
    p = L.RRCParams()
    p.out_h, p.out_w = OH, OW
    flips = cut = d_cut = d_lut = None
    d_flips = torch.zeros(B, dtype=torch.uint8, device='cuda:0')
    if post:
        flips = (np.arange(B) % 2).astype(np.uint8)
        cut = np.stack([(np.arange(B) * 5) % (OH - CUT + 1), (np.arange(B) * 7) % (OW - CUT + 1)], 1).astype(np.int32)
        d_flips = torch.from_numpy(flips).to('cuda:0')
        d_cut = torch.from_numpy(cut).to('cuda:0')
        d_lut = torch.from_numpy(_lut(oracle).view(np.int16)).to('cuda:0')
        p.cutout_size = CUT
        for i, f in enumerate(FILL):
            p.cutout_fill[i] = f
        p.lut = d_lut.data_ptr()
    out = torch.full((B, OH, OW, 3), 7, dtype=torch.float16 if post else torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.rrc(d_buf, d_smp, B, torch.from_numpy(np.ascontiguousarray(crops, np.int32)).to('cuda:0'), d_cut, d_flips,
            p, out, status)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    dec.close()
    return status.cpu().numpy(), o, flips, cut


def _rrc_want(oracle, pixels, crops, out_hw, post, flips, cut):
    """resize_crop of libjpeg-turbo's pixels, then test_kernels_gpu's post-processing."""
    u8 = np.stack([oracle.resize_crop(px, y, y + h, x, x + w, *out_hw) for px, (y, x, h, w) in zip(pixels, crops)])
    if not post:
        return u8
    return _oracle_post(u8, flips, cut, CUT, FILL, _lut(oracle))


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope='module')
def sets(oracle):
    """name -> (base, accepted variants, rejected variants); ref(blob) is
    libjpeg-turbo's decode, computed once per stream."""
    from ffcv_amd import libffcv as L
    out = {b.name: (b, J.accepted(b), J.rejected(b)) for b in J.bases()}
    cache = {}

    def ref(blob):
        key = bytes(blob)
        if key not in cache:
            cache[key] = (oracle.ljt_decode(blob), L.cpu_jpeg_coefficients(blob))
        return cache[key]
    out['ref'] = ref
    return out


def _items(base, variants):
    return [(base.name, base.blob, base.h, base.w)] + [(v.name, v.blob, v.h, v.w) for v in variants]


def _check_decode(sets, items, residues=None, expect=None):
    """One full-decode launch: status and pixels of every image (expect[k]: a
    non-zero status whose row must be zero)."""
    st, px = _decode(items, residues)
    for k, it in enumerate(items):
        e = 0 if expect is None else expect[k]
        assert st[k] == e, (it[0], st[k], e)
        if e:
            assert not px[k].any(), it[0]
        else:
            assert np.array_equal(px[k], sets['ref'](it[1])[0]), it[0]


def _check_coefficients(sets, items, residues=None, expect=None):
    good = [sets['ref'](it[1])[1] for k, it in enumerate(items) if expect is None or not expect[k]]
    st, o = _coefficients(items, [len(c) for c in good], residues)
    g = iter(good)
    for k, it in enumerate(items):
        e = 0 if expect is None else expect[k]
        assert st[k] == e, (it[0], st[k], e)
        if e:
            assert not o[k].any(), it[0]
        else:
            want = next(g)
            assert np.array_equal(o[k, :len(want)], want), it[0]


# ---------------------------------------------------------------- accepted variants
@pytest.mark.parametrize('name', J.BASE_NAMES)
def test_full_decode(hip_lib, oracle, sets, name):
    base, acc, _ = sets[name]
    _check_decode(sets, _items(base, acc))


@pytest.mark.parametrize('name', J.BASE_NAMES)
def test_coefficients(hip_lib, oracle, sets, name):
    base, acc, _ = sets[name]
    _check_coefficients(sets, _items(base, acc))


def _crops(h, w, out_hw):
    """(y, x, h, w): the full image, an odd-offset interior crop, each corner,
    one row, one column, a crop larger than the output on both axes where the
    image allows one (area resize) and one smaller than it (linear)."""
    OH, OW = out_hw
    ch, cw = max(1, h // 3), max(1, w // 3)
    y1, x1 = min(1, h - 1), min(3, w - 1)
    area = (h - min(h, max(OH + 1, h - 3)), w - min(w, max(OW + 1, w - 2)), min(h, max(OH + 1, h - 3)),
            min(w, max(OW + 1, w - 2)))
    lh, lw = min(h, max(1, OH // 2)), min(w, max(1, OW // 2))
    return [(0, 0, h, w), (y1, x1, max(1, h - y1 - 1), max(1, w - x1 - 2)),
            (0, 0, ch, cw), (0, w - cw, ch, cw), (h - ch, 0, ch, cw), (h - ch, w - cw, ch, cw),
            (h // 2, 0, 1, w), (0, w // 2, h, 1), area, ((h - lh) // 2, (w - lw) // 2, lh, lw)]


@pytest.mark.parametrize('post', [False, True], ids=['plain', 'lut_cutout_flip'])
@pytest.mark.parametrize('out_hw', OUTS, ids=['32x32', '17x40'])
@pytest.mark.parametrize('name', J.BASE_NAMES + ['small'])
def test_rrc(hip_lib, oracle, sets, name, out_hw, post):
    """Explicit crops of every accepted variant through K1, K1b and K2; the
    layout, colour-space and grey variants take K2's general selector with
    expansion factors 1, 2 and 4 and with RGB input."""
    if name == 'small':
        items = [(v.name, v.blob, v.h, v.w) for v in J.small_layouts()]
    else:
        base, acc, _ = sets[name]
        items = _items(base, acc)
    work = [(it, c) for it in items for c in _crops(it[2], it[3], out_hw)]
    for y, x, h, w in (c for _, c in work):
        assert h >= 1 and w >= 1 and y >= 0 and x >= 0
    if name in ('nat420', 'nat420opt', 'nat444', 'noise420big', 'natgray', 'noisegray'):  # 48 x 80 and 56 x 72
        assert sum(c[2] > out_hw[0] and c[3] > out_hw[1] for _, c in work) >= len(items)  # area crops
    bad = []
    for chunk in _chunks(work):
        its, crops = [w[0] for w in chunk], [w[1] for w in chunk]
        st, got, flips, cut = _rrc(oracle, its, crops, out_hw, post)
        want = _rrc_want(oracle, [sets['ref'](it[1])[0] for it in its], crops, out_hw, post, flips, cut)
        for k, (it, c) in enumerate(chunk):
            if st[k] != OK or not _same(got[k], want[k]):
                bad.append((it[0], c, int(st[k])))
    assert not bad, (len(bad), bad[:8])


# ---------------------------------------------------------------- workgroup composition
def _compositions(sets):
    """Batches of 4 and 8 (K1 decodes four images per workgroup, which share
    the tables of the first valid one): [(what, items, expected status)]."""
    std = [sets[n][0] for n in ('nat420', 'nat422', 'nat444', 'noise420')]
    s = [(b.name, b.blob, b.h, b.w) for b in std]

    def var(base, name):
        v, = [x for x in sets[base][1] + sets[base][2] if x.name == f'{base}/{name}']
        return (v.name, v.blob, v.h, v.w)
    opt = sets['nat420opt'][0]
    opt = (opt.name, opt.blob, opt.h, opt.w)
    out = [
        ('relabelled first', [var('nat420', 'ids23'), s[1], s[2], s[3]]),
        ('six slots first', [var('nat420', 'six_slots'), s[0], s[1], s[2], var('nat422', 'ids23'), s[3], s[0], s[2]]),
        ('standard first', [s[0], var('nat422', 'ids23'), var('nat420', 'six_slots'), var('nat444', 'unused_id3')]),
        ('standard first', [s[1], var('nat420', 'dc0_twice'), var('nat444', 'dht_merged'), var('nat420', 'adobe0'),
                            s[2], var('nat444', 'six_slots'), var('noise420', 'ids23'), var('nat422', 'rgb_ids')]),
        ('reject first', [var('nat420', 'dht_overrun'), s[1], s[2], var('nat444', 'ids23')]),
        ('reject first', [var('nat422', 'no_dht'), s[0], s[2], s[3], var('nat420', 'dri4'), var('nat420', 'app1_first'),
                          s[1], s[0]]),
        ('past the staged header first', [var('nat420', 'app1_first'), s[0], s[1], s[2]]),
        ('past the staged header first', [var('nat422', 'app1_before_sos'), s[0], s[1], s[3],
                                          var('nat444', 'app2_straddle'), s[2], s[0], s[1]]),
        ('past the staged header last', [s[0], var('nat420', 'app1_first'), var('nat422', 'app2_straddle'),
                                         var('nat444', 'app1_before_sos')]),
        ('past the staged header last', [s[3], s[2], var('nat420', 'app1_first'), var('nat420', 'app2_straddle'),
                                         s[1], var('nat422', 'app1_first'), s[0], var('noise420', 'app1_before_sos')]),
        ('optimised between standard', [s[0], opt, s[1], s[2]]),
        ('optimised between standard', [s[0], opt, s[1], s[2], opt, s[3], var('nat420opt', 'app1_first'), s[0]]),
    ]
    status = {f'{b}/{r.name.split("/")[1]}': r.gpu_status for b in J.BASE_NAMES for r in sets[b][2]}
    return [(what, items, [status.get(it[0], 0) for it in items]) for what, items in out]


def test_workgroup_composition(hip_lib, oracle, sets, monkeypatch):
    """Every image's status and output in each order, on all three paths.  The
    RRC launches run in batch order (FFCV_K1_ORDER=0: no size sort), so the
    workgroups hold the images listed."""
    monkeypatch.setenv('FFCV_K1_ORDER', '0')
    comps = _compositions(sets)
    assert sorted({len(c[1]) for c in comps}) == [4, 8]
    for what, items, expect in comps:
        assert items[-1][0] not in [r.name for b in J.BASE_NAMES for r in sets[b][2]], what
        _check_decode(sets, items, None, expect)
        _check_coefficients(sets, items, None, expect)
        crops = [(0, 0, it[2], it[3]) for it in items]
        st, got, _, _ = _rrc(oracle, items, crops, (32, 32), False)
        good = [k for k in range(len(items)) if not expect[k]]
        want = _rrc_want(oracle, [sets['ref'](items[k][1])[0] for k in good], [crops[k] for k in good], (32, 32),
                         False, None, None)
        assert st.tolist() == expect, (what, st)
        for k in range(len(items)):
            if expect[k]:
                assert not got[k].any(), (what, k)
            else:
                assert np.array_equal(got[k], want[good.index(k)]), (what, items[k][0])


# ---------------------------------------------------------------- alignment sweep
@pytest.mark.parametrize('name', ['noise420', 'noise420big', 'flat420'])
def test_alignment_sweep(hip_lib, oracle, sets, name):
    """Every sample offset mod 8 against a COM of 0..3 bytes in front of SOS:
    the header staging and the de-stuffing pass at every alignment of the
    sample and of the scan, on streams dense in FF 00.  Then the stream cut in
    mid-scan at each scan length mod 4: libjpeg-turbo pads such a stream with
    zero bits and leaves the rest grey; the device either equals that or
    reports CORRUPT with a zero row."""
    base, acc, _ = sets[name]
    com = [v for v in acc if v.name.split('/')[1] in ('com0', 'com1', 'com2', 'com3')]
    assert len(com) == 4
    items = [(f'{v.name}@{r}', v.blob, v.h, v.w) for v in com for r in range(8)]
    residues = [r for _ in com for r in range(8)]
    scan_offs = {(r + J.offsets(J.split(v.blob)[0])[1]) % 4 for v in com for r in range(8)}
    assert scan_offs == {0, 1, 2, 3} and len(items) == 32
    off = J.offsets(J.split(base.blob)[0])[1]
    cuts = [off + (len(base.blob) - off) // 2 + j for j in range(4)]
    assert {(c - off) % 4 for c in cuts} == {0, 1, 2, 3}
    short = [(f'{name}/cut{c}', base.blob[:c], base.h, base.w) for c in cuts]
    residues += [5, 2, 7, 4]
    items += short
    n = len(items)
    st, px = _decode(items, residues)
    cst, co = _coefficients(items, [len(sets['ref'](base.blob)[1])] * n, residues)
    for k, it in enumerate(items):
        wpx, wco = sets['ref'](it[1])
        if k >= 32:
            assert st[k] in (OK, CORRUPT) and cst[k] in (OK, CORRUPT), (it[0], st[k], cst[k])
        else:
            assert st[k] == OK and cst[k] == OK, (it[0], st[k], cst[k])
        if st[k] == OK:
            assert np.array_equal(px[k], wpx), it[0]
        else:
            assert not px[k].any(), it[0]
        if cst[k] == OK:
            assert np.array_equal(co[k, :len(wco)], wco), it[0]
        else:
            assert not co[k].any(), it[0]


# ---------------------------------------------------------------- arena
@pytest.mark.parametrize('mode', ['decode', 'coefficients', 'rrc'])
def test_arena_small_layouts(hip_lib, oracle, mode):
    """1x1, 9x33 and 33x9 images at 4x1, 1x4 and 4:4:0: the launch's scratch
    stays within the sum of the per-image bounds (ffcv_jpeg_scratch_bound
    assumes sampling factors up to 4), and the output is libjpeg-turbo's."""
    torch = _torch()
    from ffcv_amd import libffcv as L
    items = [(v.name, v.blob, v.h, v.w) for v in J.small_layouts()]
    B = len(items)
    assert B == 9
    d_buf, d_smp = _dev_set(items)
    dec = _decoder(items, B)
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    want = [oracle.ljt_decode(it[1]) for it in items]
    if mode == 'decode':
        stride = 33 * 33 * 3
        out = torch.zeros(B * stride, dtype=torch.uint8, device='cuda:0')
        dec.decode(d_buf, d_smp, B, out, stride, status)
    elif mode == 'coefficients':
        wco = [L.cpu_jpeg_coefficients(it[1]) for it in items]
        maxb = max(len(c) for c in wco) + 8
        out = torch.zeros((B, maxb, 64), dtype=torch.int16, device='cuda:0')
        dec.coefficients(d_buf, d_smp, B, out, maxb, status)
    else:
        p = L.RRCParams()
        p.out_h, p.out_w = 32, 32
        crops = np.array([(0, 0, it[2], it[3]) for it in items], np.int32)
        out = torch.zeros((B, 32, 32, 3), dtype=torch.uint8, device='cuda:0')
        dec.rrc(d_buf, d_smp, B, torch.from_numpy(crops).to('cuda:0'), None,
                torch.zeros(B, dtype=torch.uint8, device='cuda:0'), p, out, status)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all(), status.cpu().numpy()
    used, cap = dec.arena_used()
    bound = int(L.scratch_bound([it[2] for it in items], [it[3] for it in items], [len(it[1]) for it in items]).sum())
    assert 0 < used <= bound, (used, bound, cap)
    o = out.cpu().numpy()
    for k, it in enumerate(items):
        if mode == 'decode':
            assert np.array_equal(o[k * stride:k * stride + it[2] * it[3] * 3].reshape(it[2], it[3], 3), want[k]), it[0]
        elif mode == 'coefficients':
            assert np.array_equal(o[k, :len(wco[k])], wco[k]), it[0]
        else:
            assert np.array_equal(o[k], oracle.resize_crop(want[k], 0, it[2], 0, it[3], 32, 32)), it[0]
    dec.close()


# ---------------------------------------------------------------- reject set
@pytest.mark.parametrize('name', J.BASE_NAMES)
def test_reject_set(hip_lib, oracle, sets, name):
    """Every stream libjpeg-turbo rejects (and DRI 4, which this path does not
    decode) gets its documented status and a zero row on all three paths,
    between good images that stay exact.  A table running past its DQT / DHT
    segment is BAD_MARKER: without the segment-bounds check K1 builds the
    table from the next segment's bytes and dht_overrun decodes with status
    0."""
    base, acc, rej = sets[name]
    good = _items(base, [v for v in acc if v.name.split('/')[1] in ('ids23', 'app1_first', 'com1')])
    items, expect = [], []
    for k, r in enumerate(rej):
        items += [good[k % len(good)], (r.name, r.blob, r.h, r.w)]
        expect += [0, r.gpu_status]
        if r.name.endswith(('dht_overrun', 'dht_overrun_std', 'dqt_short')):
            assert r.gpu_status == BAD_MARKER
    items.append(good[0])  # a reject-set sample is never the last one
    expect.append(0)
    assert len(rej) >= 8 and set(expect) == {OK, BAD_MARKER, UNSUPPORTED}
    _check_decode(sets, items, None, expect)
    _check_coefficients(sets, items, None, expect)
    crops = [(0, 0, it[2], it[3]) for it in items]
    st, got, _, _ = _rrc(oracle, items, crops, (32, 32), False)
    assert st.tolist() == expect, st
    for k, it in enumerate(items):
        if expect[k]:
            assert not got[k].any(), it[0]
        else:
            want = oracle.resize_crop(sets['ref'](it[1])[0], 0, it[2], 0, it[3], 32, 32)
            assert np.array_equal(got[k], want), it[0]
