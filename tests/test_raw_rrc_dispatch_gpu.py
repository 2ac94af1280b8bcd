"""The raw crop+resize kernel's dispatch, swept (GPU, bit-exact + exact pin).

rrc_band (ffcv_rrc.hip) picks between a four-column "quad" walk (linear,
area-walk, general area) and a per-pixel path, over LDS-staged or global
rows, by predicates on the output width, the stride, the crop's kind and the
staged size.  The other tests enter it at output widths that are all
multiples of 4 with dense strides.  Here every predicate is taken on both
sides.  Every group of crops (one output size) runs four ways, u8 and fp16
LUT, each with and without the per-image tap workspace, into a buffer
pre-filled with a sentinel, and is compared

* bit for bit with oracle.rrc_batch (+ the epilogue in numpy), pad bytes and
  non-raw samples' rows keeping the sentinel;
* for the u8 run without epilogue, directly with tests/resize_ref.py (exact
  rationals) under the bounds derived there (area kinds 0.5 + eps < 0.75,
  linear kind 1.0066 < 1.5), so the kernel is pinned to exact arithmetic
  itself and not only through the oracle.  Observed over these cases (the
  oracle, hence the kernel): area kinds 0.6543 (at 1024 / 1028 output
  columns, where the 1e-3 sliver rule drops weight and the bound is
  0.5 + eps_f32 + eps_sliver; 0.5000 below 1000 columns), linear kind 0.7652.

Staged or not is documented by hand arithmetic from RRC_LDS_BYTES = 30464
beside each case: a band's source rows are staged when
nrows * nch * 16 <= 30464 with nch = (3 * sw + 30) >> 4 chunks per row, and
a row takes one more pass of the staging loop per 128 chunks.
"""
import numpy as np
import pytest

from ffcv_amd.synthetic import natural_image
from tests import resize_ref as R
from tests.test_kernels_gpu import _torch, _samples, _dev, _oracle_post

gpu = pytest.mark.gpu
SENT = 0xA5
FILL = (124, 116, 103)


class Item:
    def __init__(self, ih, iw, crop, flip=0, cut=(0, 0), mode=1, lead=None):
        self.ih, self.iw, self.crop, self.flip, self.cut, self.mode, self.lead = ih, iw, tuple(crop), flip, cut, mode, lead


class Group:
    def __init__(self, out, items, cs=0, cbf=False, flips=False, pads=(0, 0), tail=64, what=''):
        self.out, self.items, self.cs, self.cbf, self.flips, self.pads, self.tail, self.what = \
            out, items, cs, cbf, flips, pads, tail, what


def _item(n, h, w, **kw):
    """A crop of h x w inside an image a little larger, at offsets that vary."""
    i, j = n % 3, n % 5
    return Item(h + i + (n % 2), w + j + (n % 4), (i, j, h, w), **kw)


def _cands(oh, ow):
    c = [(oh, ow), (2 * oh, 3 * ow), (2 * oh + 1, ow + max(1, ow // 3)), (3 * oh + 1, 2 * ow), (oh + 1, ow + 1),
         (max(1, oh - 1), ow + 2), (oh + 5, max(1, ow - 1)), (max(1, oh // 2), max(1, ow // 2)), (1, ow + 1),
         (oh + 2, 1)]
    return list(dict.fromkeys(c))


# ---- 1. width classes: out_w not a multiple of 4 (and < 4), every kind
def groups_widths():
    return [Group((oh, ow), [_item(n, h, w) for n, (h, w) in enumerate(_cands(oh, ow))], what='width')
            for oh in (1, 3, 16, 17) for ow in (1, 2, 3, 5, 17, 18, 19)]


# ---- 2. out_w % 4 == 0: 3 * out_w % 16 = 12, 8, 4, 0, 12, 8, 0; only remainder 0 (vec_end == 3 * out_w, no
# scalar tail) takes the quad walk for kind 3, every width takes it for kind 2
def groups_quads():
    return [Group((17, ow), [_item(n, h, w) for n, (h, w) in enumerate(_cands(17, ow) + [(20, ow + 1)])], what='quad')
            for ow in (4, 8, 12, 16, 20, 24, 32)]


# ---- 3. thread groups: tpg = 64 for nq <= 64, 128 for out_w 260..512, 256 for 516..1024; nq > 256 at 1028
# (per-pixel).  The kind 3 crops (9 x 40; 17 x out_w / 2, at most 17 rows of 98 chunks = 26656 B) are staged
# everywhere.  The area-walk crop 30 x 1.5 out_w has 29 rows in its first band: staged only while nch <= 65
# (sw <= 341), so at these widths it runs per pixel from global memory.  The narrow area-walk crops reach the
# quad walk: 17 x (out_w + 1) reads 16 rows per band, staged while nch <= 119 (sw <= 629), and 18 x (out_w + 3)
# reads 17, staged while nch <= 112 (sw <= 587): both are staged at 252..528, tpg 256 included.  From 630 px
# on a kind 2 band (>= 16 rows) is never staged, so kind 2 at 1024 is per-pixel by arithmetic, not by choice.
def groups_thread_groups():
    out = []
    for ow in (252, 256, 260, 512, 516, 528, 1024, 1028):
        items = [_item(0, 9, 40), _item(1, 30, ow + ow // 2), _item(2, 17, ow + 1), _item(3, 18, ow + 3),
                 _item(4, 17, ow // 2)]
        out.append(Group((17, ow), items, what='tpg'))
    return out


# ---- 4. staging
def groups_staging():
    out = []
    # chunk-loop passes: nch = (3 w + 30) >> 4 is 128 at w = 676 and 677 (2058 >> 4, 2061 >> 4: one pass), 129
    # at 678 (2064 >> 4: second pass), 131 at 690, 189 at 1000, 256 at 1360 (4110 >> 4: still two passes) and 257
    # at 1361 (4113 >> 4: third pass), 258 at 1368.  10 crop rows into 33: a band reads at most 6 rows,
    # 6 * 258 * 16 = 24768 <= 30464: staged.  out_w 64 takes the quad walk, 60 the per-pixel path (staged).
    ws = (676, 677, 678, 690, 1000, 1360, 1361, 1368)
    out.append(Group((33, 64), [Item(12, w + 5, (1, n % 5, 10, w)) for n, w in enumerate(ws)], what='passes'))
    out.append(Group((33, 60), [Item(12, w + 5, (2, n % 3, 10, w)) for n, w in enumerate((678, 1361))], what='passes'))
    # staged / unstaged flip, out 16 x 176 (one band).  Area, 30 source rows (scale_y 1.875): 30 * nch * 16 <=
    # 30464 while nch <= 63, 3 w + 30 < 1024, w <= 331: widths 300..328 staged, 332..340 not.
    # Kind 3, 170 px wide (x up, nch = 540 >> 4 = 33, 528 B per row, 57 rows fit): a band of 16 rows reads
    # rows 0 .. floor(15 sh / 16) + 1: 57 rows at sh = 59, 58 at sh = 60: heights 52..59 staged, 60..66 not.
    lad = [_item(n, 30, w) for n, w in enumerate(range(300, 344, 4))]
    lad += [_item(n, sh, 170) for n, sh in enumerate((52, 54, 56, 58, 59, 60, 62, 64, 66))]
    out.append(Group((16, 176), lad, what='flip'))
    # row alignments: image widths 56..71 (stepmod = 3 w mod 16 takes every value), crop columns 0..15, sample
    # offsets at every value mod 16; a kind 3 (quad walk at 32) and an area-walk crop for each combination
    for ow in (32, 30):
        items = []
        for m in range(16):
            for j in range(16 if ow == 32 else 4):
                jj = j if ow == 32 else (5 * j + m) % 16
                for crop in ((1 + j % 3, jj, 7, 20), (j % 4, jj, 20, 36)):
                    # the sample's offset puts the crop's first byte at (m + j) mod 16
                    items.append(Item(24, 56 + m, crop, lead=(m + j - 3 * (crop[0] * (56 + m) + crop[1])) % 16))
        out.append(Group((16, ow), items, what='align'))
    return out


# ---- 5. the linear quad walk's rows: the same source row over many outputs (ra == rb at height 1), rows that
# skip (y downscaled inside kind 3: both register sets reload), and rows advancing by exactly one (role swap)
def groups_row_walk():
    hs = (1, 2, 15, 16, 17, 31, 33, 34, 40, 64, 100, 129)
    return [Group((oh, 32), [_item(n, h, 20) for n, h in enumerate(hs)], what='rows') for oh in (32, 33)]


# ---- 6. area: scales 1.03, 1.5, 1.97, 2, 2.03, 3.3 on either axis (walk / non-walk mixes, integer x fraction)
def groups_area():
    return [Group((33, 100), [_item(n, h, w) for n, (h, w) in enumerate(
        (h, w) for h in (34, 50, 65, 66, 67, 109) for w in (101, 150, 199, 200, 201, 330))], what='area')]


# ---- 7. epilogue on the quad (32; 20 for kind 2) and per-pixel (19; 20 for kind 3) paths
def groups_epilogue():
    out = []
    for N in (32, 19, 20):
        crops = [(N, N), (2 * N, 2 * N), (N + 5, N + 3), (2 * N + 3, N + 1), (N - 3, N + 4), (N // 2, N // 2)]
        plain = [_item(n, h, w, flip=f) for n, (h, w) in enumerate(crops) for f in (0, 1)]
        out.append(Group((N, N), plain, flips=True, what='epilogue'))
        # a cutout edge inside a quad: origins with x % 4 in 1..3 (and x + 6 at 3, 0, 1 mod 4)
        for cs, origins in ((1, [(0, 0), (N - 1, N - 1), (5, 6)]), (N, [(0, 0)]),
                            (6, [(0, 0), (N - 6, N - 6), (3, 1), (1, 2), (2, 3)])):
            items = [_item(n, h, w, flip=f, cut=o) for n, (h, w) in enumerate(crops) for f in (0, 1) for o in origins]
            for cbf in (False, True):
                out.append(Group((N, N), items, cs=cs, cbf=cbf, flips=True, what='epilogue'))
    return out


# ---- 8. out_stride: dense, padded to a multiple of 4, and (u8) stride % 4 in 1..3, where the kernel must
# leave the quad walk (aligned4 false); fp16 also with stride % 4 == 2 and stride % 8 == 4
def _pad_to(dense, mod, r):
    return (r - dense) % mod or mod


def groups_stride():
    out = []
    for ow in (32, 19):
        items = [_item(n, h, w) for n, (h, w) in enumerate(_cands(17, ow) + [(20, ow + 1)])]
        d8, d16 = 17 * ow * 3, 17 * ow * 6
        p8 = [0, _pad_to(d8, 4, 0), _pad_to(d8, 4, 1), _pad_to(d8, 4, 2), _pad_to(d8, 4, 3), _pad_to(d8, 16, 0)]
        p16 = [0, _pad_to(d16, 8, 4), _pad_to(d16, 4, 2), _pad_to(d16, 8, 0), _pad_to(d16, 8, 4) + 8, _pad_to(d16, 16, 0)]
        out += [Group((17, ow), items, pads=pads, what='stride') for pads in zip(p8, p16)]
    return out


# ---- 9. a non-raw (mode 0) sample inside a raw batch: its rows keep the sentinel
def groups_mixed():
    out = []
    for ow in (32, 19):
        items = [_item(n, h, w) for n, (h, w) in enumerate(_cands(17, ow)[:5])]
        items[2] = Item(8, 8, (0, 0, 8, 8), mode=0)
        out.append(Group((17, ow), items, what='mixed'))
    return out


# ---- 10. the crop ends on the buffer's last byte (no tail): the aligned-chunk staging returns the right
# bytes there.  Kind 3 quad, area walk, per-pixel staged, and an unstaged crop (40 rows of 123 chunks).
def groups_last_byte():
    first = [_item(0, 9, 40), _item(1, 20, 36)]
    return [Group((17, 32), first + [Item(12, 37, (5, 17, 7, 20))], tail=0, what='last'),
            Group((17, 32), first + [Item(25, 50, (5, 14, 20, 36))], tail=0, what='last'),
            Group((17, 19), first + [Item(13, 38, (6, 18, 7, 20))], tail=0, what='last'),
            Group((17, 32), first + [Item(60, 700, (20, 50, 40, 650))], tail=0, what='last')]


# ---- 11. one cutout across each quad walk: out 20 x 16 (3 * 16 % 16 == 0: the linear quad walk; 20 rows: two
# bands), a square of 5 at (y 13, x 6): rows 13..17 span the band boundary at row 16, columns 6..10 the quad
# boundary at column 8 (flipped with cut-before-flip: columns 5..9).  Crop 10 x 9 is kind 3 (the linear walk),
# 30 x 24 has both scales 1.5 (the area walk), 50 x 40 both 2.5 (the general-area quads: a band reads 40
# source rows of (3 * 40 + 30) >> 4 = 9 chunks, 5,760 bytes: staged).
def groups_cutout_across_walks():
    items = [_item(n, h, w, flip=f, cut=(13, 6)) for n, (h, w) in enumerate(((10, 9), (30, 24), (50, 40)))
             for f in (0, 1)]
    return [Group((20, 16), items, cs=5, cbf=cbf, flips=True, what='cutwalk') for cbf in (False, True)]


ALL = [groups_widths, groups_quads, groups_thread_groups, groups_staging, groups_row_walk, groups_area,
       groups_epilogue, groups_stride, groups_mixed, groups_last_byte, groups_cutout_across_walks]


def _tpg(ow):
    t = 64
    while t < (ow >> 2):
        t <<= 1
    return t


def _classes():
    """One record per (group, item), computed from the sizes alone."""
    rec = []
    for fn in ALL:
        for g in fn():
            oh, ow = g.out
            dense = oh * ow * 3
            for it in g.items:
                _, _, sh, sw = it.crop
                k = R.kind_of(sh, sw, oh, ow)
                rec.append(dict(what=g.what, kind=k, ow=ow, oh=oh, w4=ow % 4, v16=3 * ow % 16, tpg=_tpg(ow),
                                nq=ow >> 2, walk=k == 2 and sw < 2 * ow and sh < 2 * oh, sh=sh, sw=sw,
                                one_axis=k == 2 and ((sw >= 2 * ow) != (sh >= 2 * oh)), mode=it.mode, flip=it.flip,
                                cs=g.cs, cbf=g.cbf, cut=it.cut, s8=(dense + g.pads[0]) % 4, pad8=g.pads[0],
                                pad16=g.pads[1], s16=(2 * dense + g.pads[1]) % 8, tail=g.tail))
    return rec


def test_coverage_table():
    rec = _classes()

    def has(**kw):
        return any(all((v(r[k]) if callable(v) else r[k] == v) for k, v in kw.items()) for r in rec)
    for k in (0, 1, 2, 3):
        for w4 in (0, 1, 2, 3):
            assert has(kind=k, w4=w4), (k, w4)
        assert has(kind=k, ow=lambda w: w < 4), k
    for v16 in (0, 4, 8, 12):
        assert has(kind=3, w4=0, v16=v16) and has(kind=2, w4=0, v16=v16, walk=True), v16
    for tpg in (64, 128, 256):
        assert has(kind=3, v16=0, tpg=tpg, nq=lambda n: n <= 256), tpg
        assert has(kind=2, w4=0, walk=True, tpg=tpg, nq=lambda n: n <= 256), tpg
    assert has(kind=3, nq=lambda n: n > 256) and has(kind=2, nq=lambda n: n > 256)
    assert has(kind=3, w4=0, sw=lambda w: 677 < w <= 1360) and has(kind=3, w4=0, sw=lambda w: w > 1360)
    assert has(kind=2, w4=0, walk=False) and has(kind=2, w4=0, one_axis=True)
    assert has(kind=3, sh=1) and has(kind=3, sw=1) and has(kind=2, sh=1) and has(kind=2, sw=1)
    for s8 in (0, 1, 2, 3):
        assert has(what='stride', s8=s8, pad8=lambda p: p > 0, w4=0) and has(what='stride', s8=s8, pad8=lambda p: p > 0, w4=3)
    assert has(what='stride', pad8=0, pad16=0)
    for w4 in (0, 3):
        for n, s16 in enumerate((0, 4, lambda s: s % 4 == 2)):  # fp16 stride mod 8
            assert has(what='stride', w4=w4, s16=s16, pad16=lambda p: p > 0), (w4, n)
    assert has(mode=0, w4=0) and has(mode=0, w4=3)
    assert has(tail=0, kind=3, w4=0) and has(tail=0, kind=2, walk=True) and has(tail=0, w4=3)
    for w4 in (0, 3):
        for cbf in (False, True):
            for flip in (0, 1):
                assert has(w4=w4, cbf=cbf, flip=flip, cs=1) and has(w4=w4, cbf=cbf, flip=flip, cs=lambda c: c > 6)
                assert has(w4=w4, cbf=cbf, flip=flip, cs=6, cut=lambda c: c[1] % 4 in (1, 2, 3))
    # each quad walk with a cutout that crosses a band and a quad boundary
    for cbf in (False, True):
        for flip in (0, 1):
            for walk in (dict(kind=3), dict(kind=2, walk=True), dict(kind=2, walk=False)):
                assert has(what='cutwalk', cbf=cbf, flip=flip, v16=0, oh=lambda h: h > 16, cs=5,
                           cut=lambda c: c[0] < 16 < c[0] + 5 and c[1] < 8 < c[1] + 5, **walk), (cbf, flip, walk)
    # every source is small
    assert max(r['sh'] * r['sw'] * 3 for r in rec) <= 160_000
    # the alignment groups: every row lead (first crop byte's address mod 16, the buffer being 16-byte
    # aligned) and every row step mod 16, for the linear and the area-walk crops alike
    for g in groups_staging():
        if g.what != 'align':
            continue
        _, offs, _ = _concat([np.zeros(it.ih * it.iw * 3, np.uint8) for it in g.items], [it.lead for it in g.items], 0)
        for lin in (True, False):
            its = [(it, int(o)) for it, o in zip(g.items, offs) if (R.kind_of(*it.crop[2:], *g.out) == 3) == lin]
            assert {(o + (it.crop[0] * it.iw + it.crop[1]) * 3) % 16 for it, o in its} == set(range(16)), (g.out, lin)
            assert {it.iw * 3 % 16 for it, _ in its} == set(range(16)), (g.out, lin)
            assert {o % 16 for _, o in its} == set(range(16)), (g.out, lin)


_LUT = None


def _lut(oracle):
    global _LUT
    if _LUT is None:
        _LUT = oracle.normalize_lut(np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255)
    return _LUT


def _concat(blobs, leads, tail):
    """Samples back to back, each at the next offset with the wanted value
    mod 16 (None: 8-byte aligned); `tail` bytes follow the last one."""
    offs, pos = [], 0
    for b, lead in zip(blobs, leads):
        if lead is None:
            pos = (pos + 7) // 8 * 8
        else:
            pos += (lead - pos) % 16
        offs.append(pos)
        pos += len(b)
    buf = np.zeros(pos + tail, np.uint8)
    for o, b in zip(offs, blobs):
        buf[o:o + len(b)] = b
    return buf, np.array(offs, np.uint64), np.array([len(b) for b in blobs], np.uint64)


def _run_group(hip_lib, oracle, g, rng):
    torch = _torch()
    from ffcv_amd import libffcv as L
    oh, ow = g.out
    B = len(g.items)
    imgs = []
    for n, it in enumerate(g.items):
        if it.mode != 1:
            imgs.append(rng.integers(0, 256, (it.ih, it.iw, 3), dtype=np.uint8))
        elif n % 7 == 6:  # saturated extremes now and then
            imgs.append((rng.integers(0, 2, (it.ih, it.iw, 3)) * 255).astype(np.uint8))
        else:
            imgs.append(natural_image(rng, it.ih, it.iw))
    buf, offs, sizes = _concat([im.reshape(-1) for im in imgs], [it.lead for it in g.items], g.tail)
    for it, o in zip(g.items, offs):
        assert it.lead is None or int(o) % 16 == it.lead
    if g.tail == 0:  # the last crop ends on the buffer's last byte
        i, j, h, w = g.items[-1].crop
        assert int(offs[-1]) + ((i + h - 1) * g.items[-1].iw + j + w) * 3 == buf.size
    crops = np.array([it.crop for it in g.items], np.int32)
    for it, (i, j, h, w) in zip(g.items, crops):  # every crop lies inside its image
        assert 0 <= i and 0 <= j and h >= 1 and w >= 1 and i + h <= it.ih and j + w <= it.iw
    modes = np.array([it.mode for it in g.items])
    raw = np.flatnonzero(modes == 1)
    u8 = oracle.rrc_batch([(imgs[k].reshape(-1), g.items[k].ih, g.items[k].iw, 1) for k in raw], crops[raw], oh, ow)
    flips = np.array([it.flip for it in g.items], np.uint8) if g.flips else None
    cut = np.array([it.cut for it in g.items], np.int32) if g.cs else None
    if cut is not None:
        assert (cut >= 0).all() and (cut[:, 0] + g.cs <= oh).all() and (cut[:, 1] + g.cs <= ow).all()
    d_buf = torch.from_numpy(buf).to('cuda:0')
    assert d_buf.data_ptr() % 16 == 0
    d_smp = _dev(_samples(offs, sizes, [it.ih for it in g.items], [it.iw for it in g.items], modes))
    d_crops = torch.from_numpy(crops).to('cuda:0')
    d_cut = torch.from_numpy(cut).to('cuda:0') if cut is not None else None
    d_flips = torch.from_numpy(flips).to('cuda:0') if flips is not None else None
    lut = _lut(oracle)
    d_lut = torch.from_numpy(np.ascontiguousarray(lut).view(np.int16)).to('cuda:0')
    for fp16 in (False, True):
        want = _oracle_post(u8, flips[raw] if flips is not None else None, cut[raw] if cut is not None else None,
                            g.cs, FILL, lut if fp16 else None, g.cbf)
        want = np.ascontiguousarray(want).view(np.uint8).reshape(len(raw), -1)
        dense = want.shape[1]
        assert dense == oh * ow * 3 * (2 if fp16 else 1)
        stride = dense + g.pads[fp16]
        exp = np.full((B, stride), SENT, np.uint8)
        exp[raw, :dense] = want
        for use_ws in (False, True):
            p = L.RRCParams()
            p.out_h, p.out_w = oh, ow
            p.cutout_size = g.cs
            for c in range(3):
                p.cutout_fill[c] = FILL[c]
            p.cutout_fill[3] = int(g.cbf)
            p.out_stride = stride if g.pads[fp16] else 0
            if fp16:
                p.lut = d_lut.data_ptr()
            out = torch.full((B * stride,), SENT, dtype=torch.uint8, device='cuda:0')
            assert out.data_ptr() % 8 == 0
            ws = torch.empty(L.rrc_raw_workspace_bytes(B, oh, ow), dtype=torch.uint8, device='cuda:0') if use_ws else None
            L.rrc_raw_batch(d_buf, d_smp, B, d_crops, d_cut, d_flips, p, out, workspace=ws)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(B, stride)
            bad = np.flatnonzero((got != exp).any(1))
            assert bad.size == 0, (f'{g.what} out {g.out} fp16 {fp16} ws {use_ws} pads {g.pads} cs {g.cs} cbf {g.cbf}: '
                                   f'samples {bad[:8]} differ; crops {crops[bad[:4]].tolist()}; first bytes '
                                   f'{np.flatnonzero(got[bad[0]] != exp[bad[0]])[:6]}')
            if not fp16 and not use_ws and not g.flips and not g.cs:
                # the kernel against exact arithmetic, directly
                for n, k in enumerate(raw):
                    i, j, h, w = crops[k]
                    err, _, _, _, bound = R.compare(got[k, :dense].reshape(oh, ow, 3), imgs[k][i:i + h, j:j + w])
                    assert err <= bound, (g.what, g.out, crops[k].tolist(), err, bound)


def _run(hip_lib, oracle, fn, seed):
    rng = np.random.default_rng(seed)
    for g in fn():
        _run_group(hip_lib, oracle, g, rng)


@gpu
def test_width_classes(hip_lib, oracle):
    _run(hip_lib, oracle, groups_widths, 1)


@gpu
def test_quad_and_scalar_tail_split(hip_lib, oracle):
    _run(hip_lib, oracle, groups_quads, 2)


@gpu
def test_thread_groups(hip_lib, oracle):
    _run(hip_lib, oracle, groups_thread_groups, 3)


@gpu
def test_staging(hip_lib, oracle):
    _run(hip_lib, oracle, groups_staging, 4)


@gpu
def test_linear_row_walk(hip_lib, oracle):
    _run(hip_lib, oracle, groups_row_walk, 5)


@gpu
def test_area_scales(hip_lib, oracle):
    _run(hip_lib, oracle, groups_area, 6)


@gpu
def test_epilogue_on_both_paths(hip_lib, oracle):
    _run(hip_lib, oracle, groups_epilogue, 7)


@gpu
def test_out_stride(hip_lib, oracle):
    _run(hip_lib, oracle, groups_stride, 8)


@gpu
def test_non_raw_sample_in_raw_batch(hip_lib, oracle):
    _run(hip_lib, oracle, groups_mixed, 9)


@gpu
def test_crop_ends_on_last_byte(hip_lib, oracle):
    _run(hip_lib, oracle, groups_last_byte, 10)


@gpu
def test_cutout_across_bands_and_quads_in_each_walk(hip_lib, oracle):
    _run(hip_lib, oracle, groups_cutout_across_walks, 11)
