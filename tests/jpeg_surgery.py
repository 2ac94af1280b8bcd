"""Container surgery on baseline JPEG streams (test helper, numpy only).

A baseline stream is taken apart into its marker segments and its scan bytes
and put back together with a different container around the same
entropy-coded data: other segment orders, lengths and table ids, segments
Pillow never writes, other colour-space signalling, and SOF sampling factors
that reinterpret the same blocks as another layout.  No encoder is involved.

    split(blob)  -> ([(marker, payload), ...] up to and including SOS, scan bytes)
    join(segments, scan, fill=0) -> blob

accepted(base) and rejected(base) build the named variants of one base
stream; bases() is the set of Pillow streams they are built from.
"""
from collections import namedtuple

import numpy as np

from ffcv_amd.synthetic import natural_image, encode_jpeg

SOF0, SOF1, DHT, SOS, DQT, DRI, APP0, APP1, APP2, APP14, COM = \
    0xC0, 0xC1, 0xC4, 0xDA, 0xDB, 0xDD, 0xE0, 0xE1, 0xE2, 0xEE, 0xFE
HDR_BYTES = 2048  # header bytes K1 stages in LDS (jpeg_defs.h)

Base = namedtuple('Base', 'name blob h w sub')          # sub: '4:2:0', '4:2:2', '4:4:4' or 'gray'
Variant = namedtuple('Variant', 'name blob h w group')  # group: 'container', 'colour' or 'layout'
Reject = namedtuple('Reject', 'name blob h w gpu_status cpu_decodes')


# ---------------------------------------------------------------- split / join
def split(blob):
    b = bytes(blob)
    assert b[:2] == b'\xff\xd8', 'no SOI'
    p, segs = 2, []
    while True:
        assert b[p] == 0xFF, f'no marker at {p}'
        while b[p] == 0xFF:
            p += 1
        m = b[p]
        n = (b[p + 1] << 8) | b[p + 2]
        segs.append((m, b[p + 3:p + 1 + n]))
        p += 1 + n
        if m == SOS:
            return segs, b[p:]


def _seg(m, payload, length=None, fill=0):
    n = len(payload) + 2 if length is None else length
    return b'\xff' * fill + bytes([0xFF, m, n >> 8, n & 255]) + bytes(payload)


def join(segments, scan, fill=0):
    out = b'\xff\xd8' + b''.join(_seg(m, pl, fill=fill) for m, pl in segments) + bytes(scan)
    return np.frombuffer(out, np.uint8).copy()


def offsets(segments, fill=0):
    """Byte offset of each segment's marker (its 0xFF) in join(segments, ...)."""
    out, p = [], 2
    for m, pl in segments:
        out.append(p + fill)
        p += fill + 4 + len(pl)
    return out, p  # p: scan offset


# ---------------------------------------------------------------- tables
def dqt_tables(segs):
    """[(precision, id, 64 values in zigzag order)] of every DQT segment, in order."""
    out = []
    for m, pl in segs:
        if m != DQT:
            continue
        p = 0
        while p < len(pl):
            pq, tq = pl[p] >> 4, pl[p] & 15
            n = 128 if pq else 64
            v = pl[p + 1:p + 1 + n]
            vals = [(v[2 * i] << 8) | v[2 * i + 1] for i in range(64)] if pq else list(v)
            out.append((pq, tq, vals))
            p += 1 + n
    return out


def dqt_payload(pq, tq, vals):
    if pq:
        return bytes([0x10 | tq]) + b''.join(bytes([v >> 8, v & 255]) for v in vals)
    return bytes([tq]) + bytes(vals)


def dht_tables(segs):
    """[(class, id, 16 counts, symbols)] of every DHT segment, in order."""
    out = []
    for m, pl in segs:
        if m != DHT:
            continue
        p = 0
        while p < len(pl):
            tc, th = pl[p] >> 4, pl[p] & 15
            counts = list(pl[p + 1:p + 17])
            n = sum(counts)
            out.append((tc, th, counts, bytes(pl[p + 17:p + 17 + n])))
            p += 17 + n
    return out


def dht_payload(tc, th, counts, vals):
    return bytes([(tc << 4) | th]) + bytes(counts) + bytes(vals)


def _index(segs, m, nth=0):
    return [i for i, s in enumerate(segs) if s[0] == m][nth]


def _sof_index(segs):
    return [i for i, s in enumerate(segs) if s[0] in (SOF0, SOF1)][0]


def _ncomp(segs):
    return segs[_sof_index(segs)][1][5]


def _edit(segs, i, fn):
    out = list(segs)
    pl = bytearray(out[i][1])
    m = fn(pl)
    out[i] = (out[i][0] if m is None else m, bytes(pl))
    return out


def _insert_before(segs, m, new):
    i = _index(segs, m)
    return segs[:i] + list(new) + segs[i:]


def _without(segs, m):
    return [s for s in segs if s[0] != m]


def _one_per_segment(segs):
    """Every DQT / DHT table in a segment of its own (Pillow's layout already;
    kept so that the builders below do not depend on it)."""
    out = []
    for m, pl in segs:
        if m == DQT:
            out += [(DQT, dqt_payload(*t)) for t in dqt_tables([(m, pl)])]
        elif m == DHT:
            out += [(DHT, dht_payload(*t)) for t in dht_tables([(m, pl)])]
        else:
            out.append((m, pl))
    return out


# ---------------------------------------------------------------- container-only variants
def _com(segs, n):
    return _insert_before(segs, SOS, [(COM, b'c' * n)])


def _pad_seg(m, n):
    """An APPn segment of n bytes in all (marker and length included)."""
    return (m, bytes((7 * i + 1) & 255 for i in range(n - 4)))


def _app1_first(segs):
    return [_pad_seg(APP1, 3000)] + segs


def _app1_before_sos(segs):
    return _insert_before(segs, SOS, [_pad_seg(APP1, 3000)])


def _app2_straddle(segs):
    """An APP2 in front of the largest DHT, sized so that this table's counts
    and the first half of its symbols lie inside the staged header and the
    rest of its symbols past HDR_BYTES."""
    i = max((k for k, s in enumerate(segs) if s[0] == DHT), key=lambda k: len(segs[k][1]))
    offs, _ = offsets(segs)
    nsym = len(segs[i][1]) - 17
    assert nsym >= 2
    pad = HDR_BYTES - (4 + 17 + nsym // 2) - offs[i]
    out = segs[:i] + [_pad_seg(APP2, pad)] + segs[i:]
    o2, _ = offsets(out)
    assert o2[i + 1] + 4 + 17 < HDR_BYTES < o2[i + 1] + 4 + len(segs[i][1])
    return out


def _merge(segs, m):
    idx = [i for i, s in enumerate(segs) if s[0] == m]
    merged = (m, b''.join(segs[i][1] for i in idx))
    return [merged if i == idx[0] else s for i, s in enumerate(segs) if i == idx[0] or i not in idx]


def _dqt16(segs):
    return [(DQT, b''.join(dqt_payload(1, tq, v) for _, tq, v in dqt_tables([s]))) if s[0] == DQT else s
            for s in segs]


def _sof1(segs):
    return _edit(segs, _sof_index(segs), lambda pl: SOF1)


def _dri(segs, n):
    return _insert_before(segs, SOS, [(DRI, bytes([n >> 8, n & 255]))])


def _map_ids(segs, qmap, hmap):
    """DQT ids through qmap (DQT segments and SOF), DHT ids through hmap (DHT
    segments and SOS)."""
    out = []
    for m, pl in _one_per_segment(segs):
        pl = bytearray(pl)
        if m == DQT:
            pl[0] = (pl[0] & 0xF0) | qmap[pl[0] & 15]
        elif m == DHT:
            pl[0] = (pl[0] & 0xF0) | hmap[pl[0] & 15]
        elif m in (SOF0, SOF1):
            for c in range(pl[5]):
                pl[8 + 3 * c] = qmap[pl[8 + 3 * c]]
        elif m == SOS:
            for c in range(pl[0]):
                t = pl[2 + 2 * c]
                pl[2 + 2 * c] = (hmap[t >> 4] << 4) | hmap[t & 15]
        out.append((m, bytes(pl)))
    return out


def _ids23(segs):
    return _map_ids(segs, {0: 2, 1: 3}, {0: 2, 1: 3})


def _table(segs, tc, th):
    return [t for t in dht_tables(segs) if t[0] == tc and t[1] == th][-1]


def _six_slots(segs):
    """The chroma DC and AC tables again as id 2, Cr pointed at them: three DC
    and three AC tables in one scan."""
    assert _ncomp(segs) == 3
    dc, ac = _table(segs, 0, 1), _table(segs, 1, 1)
    out = _insert_before(segs, SOS, [(DHT, dht_payload(0, 2, dc[2], dc[3])), (DHT, dht_payload(1, 2, ac[2], ac[3]))])

    def cr(pl):
        pl[6] = 0x22
    return _edit(out, _index(out, SOS), cr)


def _unused_id3(segs):
    dc, ac = _table(segs, 0, 0), _table(segs, 1, 0)
    q = dqt_tables(segs)[0]
    return _insert_before(segs, SOS, [(DQT, dqt_payload(0, 3, q[2])), (DHT, dht_payload(0, 3, dc[2], dc[3])),
                                      (DHT, dht_payload(1, 3, ac[2], ac[3]))])


# a valid DC table that is none of the stream's own: one code of each length 2..13
_OTHER_DC = (0, 0, [0] + [1] * 12 + [0] * 3, bytes(range(12)))


def _dc0_twice(segs):
    first = _OTHER_DC if _ncomp(segs) == 1 else _table(segs, 0, 1)
    assert (first[2], first[3]) != _table(segs, 0, 0)[2:]
    return _insert_before(segs, DHT, [(DHT, dht_payload(0, 0, first[2], first[3]))])


def _gray_factors(segs, hv):
    assert _ncomp(segs) == 1

    def f(pl):
        pl[7] = hv
    return _edit(segs, _sof_index(segs), f)


# ---------------------------------------------------------------- colour-space variants
def _comp_ids(segs, ids):
    def sof(pl):
        for c in range(3):
            pl[6 + 3 * c] = ids[c]

    def sos(pl):
        for c in range(3):
            pl[1 + 2 * c] = ids[c]
    return _edit(_edit(segs, _sof_index(segs), sof), _index(segs, SOS), sos)


def _rgb_ids(segs):
    return _comp_ids(_without(segs, APP0), b'RGB')


def _adobe(segs, transform):
    pl = b'Adobe' + bytes([0, 100, 0, 0, 0, 0, transform])
    return [(APP14, pl)] + _without(segs, APP0)


# ---------------------------------------------------------------- layout variants
def _geometry(segs):
    pl = segs[_sof_index(segs)][1]
    h, w, nc = (pl[1] << 8) | pl[2], (pl[3] << 8) | pl[4], pl[5]
    hs, vs = pl[7] >> 4, pl[7] & 15
    if nc == 1:
        return h, w, 1, -(-w // 8) * -(-h // 8)
    return h, w, hs * vs + 2, -(-w // (8 * hs)) * -(-h // (8 * vs))


def _relayout(segs, yfac, h, w):
    """The same blocks as luma factors yfac (chroma 1x1) at h x w: the blocks
    per MCU and the MCU count must be those of the stream."""
    def f(pl):
        pl[1:5] = bytes([h >> 8, h & 255, w >> 8, w & 255])
        pl[7] = yfac
    out = _edit(segs, _sof_index(segs), f)
    assert _geometry(out)[2:] == _geometry(segs)[2:], (_geometry(out), _geometry(segs))
    return out


def relayout(blob, yfac, h, w):
    segs, scan = split(blob)
    return join(_relayout(segs, yfac, h, w), scan)


# layout variants by base name: (variant, luma factors, height, width)
_LAYOUTS = {
    'nat422': [('l440', 0x12, 41, 21), ('dims', 0x21, 17, 33)],
    'nat420': [('l411', 0x41, 39, 87), ('l1x4', 0x14, 91, 37), ('dims', 0x22, 33, 65)],
    'nat420opt': [('l411', 0x41, 39, 87), ('l1x4', 0x14, 91, 37), ('dims', 0x22, 33, 65)],
    'noise420big': [('l411', 0x41, 75, 61), ('l1x4', 0x14, 61, 75), ('dims', 0x22, 49, 65)],
    'noise420': [('l411', 0x41, 1, 1), ('l1x4', 0x14, 1, 1), ('dims', 0x22, 1, 1)],
    'flat420': [('l411', 0x41, 7, 31), ('l1x4', 0x14, 31, 7), ('dims', 0x22, 3, 5)],
    'nat444': [('dims', 0x11, 41, 73)],
}

CONTAINER = ['com0', 'com1', 'com2', 'com3', 'app1_first', 'app1_before_sos', 'app2_straddle', 'fill3',
             'dqt_merged', 'dht_merged', 'dqt16', 'sof1', 'dri0', 'trailing', 'no_eoi', 'ids23', 'six_slots',
             'unused_id3', 'dc0_twice', 'gray22', 'gray41']
COLOUR = ['rgb_ids', 'adobe0', 'adobe1']
LAYOUT = ['l440', 'l411', 'l1x4', 'dims']
ACCEPT = CONTAINER + COLOUR + LAYOUT
REJECT = ['dht_overrun', 'dht_overrun_std', 'dqt_short', 'sos_first', 'no_dqt', 'no_dht', 'nonintegral',
          'prec12', 'four_comp', 'dri4']


def accepted(base):
    """Every accept-set variant that applies to this base stream."""
    segs, scan = split(base.blob)
    gray = base.sub == 'gray'
    out = []

    def add(name, group, s=segs, sc=scan, fill=0, h=base.h, w=base.w):
        out.append(Variant(f'{base.name}/{name}', join(s, sc, fill), h, w, group))
    for n in range(4):
        add(f'com{n}', 'container', _com(segs, n))
    add('app1_first', 'container', _app1_first(segs))
    add('app1_before_sos', 'container', _app1_before_sos(segs))
    add('app2_straddle', 'container', _app2_straddle(segs))
    add('fill3', 'container', fill=3)
    add('dqt_merged', 'container', _merge(segs, DQT))
    add('dht_merged', 'container', _merge(segs, DHT))
    add('dqt16', 'container', _dqt16(segs))
    add('sof1', 'container', _sof1(segs))
    add('dri0', 'container', _dri(segs, 0))
    add('trailing', 'container', sc=scan + bytes((37 * i + 11) & 255 for i in range(256)))
    assert scan[-2:] == b'\xff\xd9'
    add('no_eoi', 'container', sc=scan[:-2])
    add('ids23', 'container', _ids23(segs))
    add('unused_id3', 'container', _unused_id3(segs))
    add('dc0_twice', 'container', _dc0_twice(segs))
    if gray:
        add('gray22', 'container', _gray_factors(segs, 0x22))
        add('gray41', 'container', _gray_factors(segs, 0x41))
    else:
        add('six_slots', 'container', _six_slots(segs))
        add('rgb_ids', 'colour', _rgb_ids(segs))
        add('adobe0', 'colour', _adobe(segs, 0))
        add('adobe1', 'colour', _adobe(segs, 1))
    for name, yfac, h, w in _LAYOUTS.get(base.name, []):
        add(name, 'layout', _relayout(segs, yfac, h, w), h=h, w=w)
    return out


# ---------------------------------------------------------------- reject set
BAD_MARKER, UNSUPPORTED = 1, 2  # FFCV_SAMPLE_* (include/ffcv_hip.h)


def trim_ac_table(segs, drop=6):
    """The luma AC table without its last `drop` 16-bit codes.  Canonical codes
    are assigned in order, so every other code keeps its bits; the stream
    still decodes as long as it uses none of the dropped symbols (the caller
    checks that it does)."""
    i = [k for k, s in enumerate(segs) if s[0] == DHT and s[1][0] == 0x10][0]
    (tc, th, counts, vals), = dht_tables([segs[i]])
    if counts[15] <= drop:  # an optimised table: every symbol is in use
        return None, i
    counts = counts[:15] + [counts[15] - drop]
    out = list(segs)
    out[i] = (DHT, dht_payload(tc, th, counts, vals[:-drop]))
    return out, i


def _dht_overrun(segs):
    """One count of the trimmed luma AC table (see trim_ac_table) raised by 5:
    the counts stay a valid code, and the last five symbols lie in the next
    segment."""
    out, i = trim_ac_table(_one_per_segment(segs))
    if out is None:
        return None

    def f(pl):
        pl[16] += 5
    return _edit(out, i, f)


def trimmed(base):
    """The accepted stream dht_overrun is made from (None for optimised tables)."""
    segs, scan = split(base.blob)
    out, _ = trim_ac_table(_one_per_segment(segs))
    return None if out is None else join(out, scan)


def _dht_overrun_std(segs):
    """The same on the table as written (a complete code: over-subscribed too)."""
    segs = _one_per_segment(segs)
    i = [k for k, s in enumerate(segs) if s[0] == DHT and s[1][0] == 0x10][0]

    def f(pl):
        pl[16] += 5
    return _edit(segs, i, f)


def rejected(base):
    segs, scan = split(base.blob)
    gray = base.sub == 'gray'
    out = []

    def add(name, s, status=BAD_MARKER, cpu_decodes=False):
        blob = s if isinstance(s, np.ndarray) else join(s, scan)
        out.append(Reject(f'{base.name}/{name}', blob, base.h, base.w, status, cpu_decodes))
    if _dht_overrun(segs) is not None:
        add('dht_overrun', _dht_overrun(segs))
    add('dht_overrun_std', _dht_overrun_std(segs))
    # a DQT segment whose length field is 10 short: the table runs past it
    i = _index(segs, DQT)
    raw = b'\xff\xd8' + b''.join(_seg(m, pl, length=len(pl) + 2 - 10 if k == i else None)
                                 for k, (m, pl) in enumerate(segs)) + scan
    add('dqt_short', np.frombuffer(raw, np.uint8).copy())
    k = _sof_index(segs)
    add('sos_first', [s for s in segs[:k] if s[0] != SOS] + [segs[-1]] + segs[k:-1])

    def undefined_q(pl):
        pl[8] = 2
    add('no_dqt', _edit(segs, k, undefined_q))

    def undefined_h(pl):
        pl[2] = 0x23
    add('no_dht', _edit(segs, _index(segs, SOS), undefined_h))

    def prec12(pl):
        pl[0] = 12
    add('prec12', _edit(segs, k, prec12), UNSUPPORTED)
    add('dri4', _dri(segs, 4), UNSUPPORTED, True)
    if not gray:
        def nonint(pl):
            pl[7], pl[10] = 0x32, 0x21
        add('nonintegral', _edit(segs, k, nonint), UNSUPPORTED)

        def four(pl):
            pl[5] = 4
            pl += bytes([4, 0x11, 1])
        add('four_comp', _edit(segs, k, four), UNSUPPORTED)
    return out


# ---------------------------------------------------------------- base streams
BASE_NAMES = ['nat420', 'nat420opt', 'nat422', 'nat444', 'noise420', 'noise420big', 'flat420', 'natgray',
              'noisegray']


def _noise(rng, h, w):
    """Two-level noise at 16 / 239 (dense in FF 00 stuffing at q100); not 0 / 255,
    where libjpeg-turbo's SIMD IDCT wraps on a few pixels and its C form does
    not (see tests/test_k1_write_chunks_gpu.py)."""
    return rng.choice(np.array([16, 239], np.uint8), size=(h, w, 3))


def bases():
    rng = np.random.default_rng(2048)
    nat = natural_image(rng, 48, 80)
    small = natural_image(rng, 24, 40)
    big, tiny = _noise(rng, 56, 72), _noise(rng, 16, 16)
    flat = np.full((8, 8, 3), (200, 60, 120), np.uint8)

    def b(name, img, q, sub, **kw):
        g = sub == 'gray'
        blob = encode_jpeg(np.ascontiguousarray(img[:, :, 1]) if g else img, q, '4:4:4' if g else sub, **kw)
        return Base(name, blob, img.shape[0], img.shape[1], sub)
    out = [b('nat420', nat, 75, '4:2:0'), b('nat420opt', nat, 90, '4:2:0', optimize=True),
            b('nat422', small, 90, '4:2:2'), b('nat444', nat, 90, '4:4:4'),
            b('noise420', tiny, 100, '4:2:0'), b('noise420big', big, 100, '4:2:0'),
            b('flat420', flat, 90, '4:2:0'), b('natgray', nat, 90, 'gray'), b('noisegray', big, 100, 'gray')]
    assert [x.name for x in out] == BASE_NAMES
    return out


def small_layout_bases():
    """Streams of 1, 4, 5 and 6 MCUs for the smallest images of each layout:
    {(blocks per MCU - 2, MCUs): blob} with 4:2:0 (4 luma blocks) and 4:2:2 (2)."""
    rng = np.random.default_rng(99)
    out = {}
    for sub, shapes in (('4:2:0', [(16, 16), (32, 32), (16, 80)]), ('4:2:2', [(8, 16), (8, 80), (8, 96)])):
        for h, w in shapes:
            blob = encode_jpeg(natural_image(rng, h, w), 90, sub)
            out[(_geometry(split(blob)[0])[2] - 2, _geometry(split(blob)[0])[3])] = blob
    return out


def small_layouts():
    """1x1, 9x33 and 33x9 images at 4x1, 1x4 and 4:4:0 (1 to 6 MCUs each)."""
    src = small_layout_bases()
    out = []
    for name, yfac in (('l411', 0x41), ('l1x4', 0x14), ('l440', 0x12)):
        hs, vs = yfac >> 4, yfac & 15
        for h, w in ((1, 1), (9, 33), (33, 9)):
            n = -(-w // (8 * hs)) * -(-h // (8 * vs))
            out.append(Variant(f'{name}/{h}x{w}', relayout(src[(hs * vs, n)], yfac, h, w), h, w, 'layout'))
    return out
