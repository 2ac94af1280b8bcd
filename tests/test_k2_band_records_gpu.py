"""K2's per-band records (written by K1b, one thread per band) against the oracle.

Every case goes through the fused entry point (ffcv_jpeg_rrc_fused: gather,
draws, decode, crop, resize, epilogue) and is compared bit for bit with the
CPU oracle on the crops the launch drew (which must equal the oracle's own
draws).  The shapes are the smallest that stress what a record holds: a
partial last band, tile clamps at every image edge, odd crop offsets, every
subsampling (fast and general selectors), the area scales around 1 and 2, a
band whose LDS layout does not fit, both epilogue orders, a failed image
between good ones, and a second launch with another geometry on one context.
The draw parameters and seeds were chosen with the oracle's draws so that the
asserted crop properties hold.
"""
import ctypes

import numpy as np
import pytest

from ffcv_amd.synthetic import natural_image, encode_jpeg, pack

pytestmark = pytest.mark.gpu

FILL = (124, 9, 203)
SUBS = ['4:2:0', '4:2:2', '4:4:4', 'gray']


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch


@pytest.fixture(autouse=True)
def _need_device():
    _torch()


def _encode(img, sub, q=90):
    if sub == 'gray':
        return encode_jpeg(img[:, :, 0].copy(), q)
    return encode_jpeg(img, q, sub)


class Case:
    """Images + the oracle's draws for one fused launch."""

    def __init__(self, oracle, shapes, subs, out_hw, seed, epoch, scale=(0.08, 1.0), ratio=(0.75, 4 / 3),
                 cutout=0, flip_p=0.0, img_seed=0, junk=()):
        rng = np.random.default_rng(img_seed)
        self.shapes, self.out_hw, self.seed, self.epoch = shapes, out_hw, seed, epoch
        self.scale, self.ratio, self.cutout, self.flip_p = scale, ratio, cutout, flip_p
        self.blobs = [_encode(natural_image(rng, h, w), subs[k % len(subs)]) for k, (h, w) in enumerate(shapes)]
        for k in junk:  # a sample that fails to parse
            self.blobs[k] = rng.integers(0, 256, 300).astype(np.uint8)
        self.junk = list(junk)
        self.hs = [h for h, _ in shapes]
        self.ws = [w for _, w in shapes]
        self.ids = np.arange(len(shapes), dtype=np.uint64)
        self.crops, self.cut = oracle.draw_batch(self.ids, self.hs, self.ws, seed, epoch, scale=scale, ratio=ratio,
                                                 out_h=out_hw[0], out_w=out_hw[1], cutout_size=cutout)
        self.flips = np.array([flip_p > 0 and oracle.MT(oracle.sample_seed(seed, epoch, int(i), 3)).uniform(0, 1) < flip_p
                               for i in self.ids], np.uint8)
        good = [k for k in range(len(shapes)) if k not in self.junk]
        self.u8 = np.zeros((len(shapes), out_hw[0], out_hw[1], 3), np.uint8)
        self.u8[good] = oracle.rrc_batch([(self.blobs[k], self.hs[k], self.ws[k], 0) for k in good],
                                         self.crops[good], out_hw[0], out_hw[1])

    def want(self, lut=None, cut_before_flip=False):
        u8 = self.u8.copy()
        for k in range(len(self.shapes)):
            if k in self.junk:
                continue
            if self.cutout and cut_before_flip:
                y, x = self.cut[k]
                u8[k, y:y + self.cutout, x:x + self.cutout] = FILL
            if self.flips[k]:
                u8[k] = u8[k, :, ::-1]
            if self.cutout and not cut_before_flip:
                y, x = self.cut[k]
                u8[k, y:y + self.cutout, x:x + self.cutout] = FILL
        if lut is None:
            return u8
        idx = u8.astype(np.int64)
        out = np.stack([lut[idx[..., c], c] for c in range(3)], -1)
        out[self.junk] = 0
        return out


def _lut(oracle):
    return oracle.normalize_lut(np.array([0.485, 0.456, 0.406]) * 255, np.array([0.229, 0.224, 0.225]) * 255)


def _decoder(cases):
    from ffcv_amd import libffcv as L
    return L.JpegDecoder(max(len(c.shapes) for c in cases), max(max(c.hs) for c in cases),
                         max(max(c.ws) for c in cases), max(max(len(b) for b in c.blobs) for c in cases))


def _run(hip_lib, oracle, case, dec, use_lut=False, cut_before_flip=False):
    """One fused launch of `case` on `dec`; asserts draws, status and pixels."""
    torch = _torch()
    from ffcv_amd import libffcv as L
    from ffcv_amd.libffcv import SAMPLE_DTYPE
    buf, offs, sizes = pack(case.blobs)
    table = np.zeros(len(offs), SAMPLE_DTYPE)
    table['offset'], table['size'], table['height'], table['width'] = offs, sizes, case.hs, case.ws
    d_buf = torch.from_numpy(buf).to('cuda:0')
    d_table = torch.from_numpy(table.view(np.uint8)).to('cuda:0')
    d_ids = torch.from_numpy(case.ids.view(np.int64)).to('cuda:0')
    B, (OH, OW) = len(case.shapes), case.out_hw
    dp = L.DrawParams()
    dp.crop_kind = 0
    dp.out_h, dp.out_w = OH, OW
    dp.cutout_size = case.cutout
    dp.scale[0], dp.scale[1] = case.scale
    dp.ratio[0], dp.ratio[1] = case.ratio
    dp.center_ratio = 224 / 256
    dp.loader_seed, dp.epoch = case.seed, case.epoch
    dp.flip_prob = float(case.flip_p)
    rp = L.RRCParams()
    rp.out_h, rp.out_w = OH, OW
    rp.cutout_size = case.cutout
    for i, f in enumerate(FILL):
        rp.cutout_fill[i] = f
    rp.cutout_fill[3] = 1 if cut_before_flip else 0
    lut = _lut(oracle) if use_lut else None
    if use_lut:
        d_lut = torch.from_numpy(lut.view(np.int16)).to('cuda:0')
        rp.lut = d_lut.data_ptr()
    crops = torch.full((B, 4), -7, dtype=torch.int32, device='cuda:0')
    cut = torch.full((B, 2), -7, dtype=torch.int32, device='cuda:0') if case.cutout else None
    flips = torch.full((B,), 9, dtype=torch.uint8, device='cuda:0') if case.flip_p > 0 else None
    out = torch.full((B, OH, OW, 3), 77, dtype=torch.float16 if use_lut else torch.uint8, device='cuda:0')
    status = torch.full((B,), -1, dtype=torch.int32, device='cuda:0')
    dec.rrc_fused(d_buf, d_table, d_ids, dp, crops, cut, flips, rp, out, status)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    good = np.array([k not in case.junk for k in range(B)])
    assert (st[good] == 0).all() and (st[~good] != 0).all(), st
    assert np.array_equal(crops.cpu().numpy()[good], case.crops[good])
    if case.cutout:
        assert np.array_equal(cut.cpu().numpy()[good], case.cut[good])
    if case.flip_p > 0:
        assert np.array_equal(flips.cpu().numpy()[good], case.flips[good])
    want = case.want(lut, cut_before_flip)
    got = out.cpu().numpy()
    bad = np.argwhere((got.view(np.uint8) != want.view(np.uint8)).reshape(B, -1).any(1)).ravel()
    assert bad.size == 0, f'images {bad} differ (crops {case.crops[bad].tolist()}, lut {use_lut})'
    return got


MIXED = [(64, 64), (63, 61), (37, 53), (48, 64), (64, 40), (33, 34), (57, 29), (20, 64)]


@pytest.mark.parametrize('out_h', [17, 40])
def test_partial_last_band(hip_lib, oracle, out_h):
    """out_h 17 and 40 at out_w 32: the last band has 1 and 8 rows."""
    case = Case(oracle, MIXED, SUBS, (out_h, 32), seed=11, epoch=1, cutout=8, flip_p=0.5, img_seed=out_h)
    dec = _decoder([case])
    for use_lut in (False, True):
        _run(hip_lib, oracle, case, dec, use_lut)


def test_edge_crops_and_odd_offsets(hip_lib, oracle):
    """Whole-image crops (every tile clamp acts at once: scale 1 at the
    image's own aspect) and random crops with odd offsets that touch each edge."""
    sq = [(64, 64), (63, 63), (37, 37), (50, 50), (64, 64), (21, 21), (49, 49), (62, 62)]
    full = Case(oracle, sq, ['4:2:0', '4:2:2', '4:4:4'], (40, 32), seed=3, epoch=0, scale=(1.0, 1.0), ratio=(1.0, 1.0),
                img_seed=5)
    assert all(tuple(c) == (0, 0, h, w) for c, (h, w) in zip(full.crops, sq))
    rnd = Case(oracle, MIXED, ['4:2:0', '4:2:0', '4:2:2', '4:4:4'], (40, 32), seed=EDGE_SEED, epoch=2,
               scale=(0.3, 0.9), img_seed=6)
    c, hs, ws = rnd.crops, np.array(rnd.hs), np.array(rnd.ws)
    assert (c[:, 0] == 0).any() and (c[:, 1] == 0).any()  # top, left
    assert (c[:, 0] + c[:, 2] == hs).any() and (c[:, 1] + c[:, 3] == ws).any()  # bottom, right
    assert ((c[:, 0] & 1) & (c[:, 1] & 1)).any()  # odd ri and rj together
    dec = _decoder([full, rnd])
    _run(hip_lib, oracle, full, dec)
    _run(hip_lib, oracle, rnd, dec, use_lut=True)


EDGE_SEED = 12  # (the first loader seed whose draws over MIXED satisfy the asserts above)


@pytest.mark.parametrize('sub', SUBS)
def test_subsamplings(hip_lib, oracle, sub):
    """4:2:0 takes the fast selectors (4:2:2 and 4:4:4 the linear one only),
    grayscale and the area crops of the others the general path."""
    case = Case(oracle, MIXED, [sub], (40, 32), seed=7, epoch=3, scale=(0.1, 1.0), cutout=6, flip_p=0.5, img_seed=9)
    assert (case.crops[:, 2] > 40).any() and (case.crops[:, 2] < 40).any()  # area and linear crops
    dec = _decoder([case])
    for use_lut in (False, True):
        _run(hip_lib, oracle, case, dec, use_lut)


def test_area_scales(hip_lib, oracle):
    """Whole-image crops of square 4:2:0 images to 32 x 32: scale just above 1
    (33, 34), in between, just below 2 (62, 63), exactly 2 (64: the general
    path); then to 24 x 24, where 49 .. 64 are at 2 or more."""
    sq = [(33, 33), (34, 34), (47, 47), (62, 62), (63, 63), (64, 64), (48, 48), (49, 49)]
    a = Case(oracle, sq, ['4:2:0'], (32, 32), seed=1, epoch=0, scale=(1.0, 1.0), ratio=(1.0, 1.0), cutout=5,
             flip_p=0.5, img_seed=12)
    b = Case(oracle, sq, ['4:2:0'], (24, 24), seed=1, epoch=1, scale=(1.0, 1.0), ratio=(1.0, 1.0), img_seed=12)
    for c in (a, b):
        assert all(tuple(x) == (0, 0, h, w) for x, (h, w) in zip(c.crops, sq))
    dec = _decoder([a, b])
    for use_lut in (False, True):
        _run(hip_lib, oracle, a, dec, use_lut)
        _run(hip_lib, oracle, b, dec, use_lut)


def test_lds_overflow_falls_back(hip_lib, oracle):
    """A full-width 256-px crop to 224: 256 x 256 (about 20 crop rows per
    band) and 440 x 256 (scale 1.96 down the rows: about 34 crop rows of 768
    bytes per band, past K2's LDS, so those bands take the general path)."""
    torch = _torch()
    shapes = [(256, 256), (440, 256)]
    cases = [Case(oracle, [s], ['4:2:0'], (224, 224), seed=2, epoch=k, scale=(1.0, 1.0),
                  ratio=(s[1] / s[0], s[1] / s[0]), flip_p=0.5, img_seed=20 + k) for k, s in enumerate(shapes)]
    for c, s in zip(cases, shapes):
        assert tuple(c.crops[0]) == (0, 0, s[0], s[1])
    dec = _decoder(cases)
    dbg = torch.zeros((1, 16), dtype=torch.int64, device='cuda:0')  # slot 11: bands on the general path
    hip_lib.ffcv_jpeg_set_debug(dec.handle, ctypes.c_void_p(dbg.data_ptr()))
    general = []
    for c in cases:
        for use_lut in (False, True):
            dbg.zero_()
            _run(hip_lib, oracle, c, dec, use_lut)
            general.append(int(dbg[0, 11].item()))
    hip_lib.ffcv_jpeg_set_debug(dec.handle, None)
    assert general[0] == 0 and general[1] == 0, general  # 256 x 256: every band fits (the area selector)
    assert general[2] == 14 and general[3] == 14, general  # 440 x 256: every band falls back


@pytest.mark.parametrize('use_lut', [False, True])
@pytest.mark.parametrize('cut_before_flip', [False, True])
def test_epilogue_orders(hip_lib, oracle, use_lut, cut_before_flip):
    case = Case(oracle, MIXED, ['4:2:0'], (40, 32), seed=13, epoch=4, scale=(0.1, 1.0), cutout=12, flip_p=0.5,
                img_seed=3)
    assert case.flips.any() and not case.flips.all()
    _run(hip_lib, oracle, case, _decoder([case]), use_lut, cut_before_flip)


def test_failed_image_between_good_ones(hip_lib, oracle):
    """Image 3 fails to parse: its bands are zero-filled beside good bands."""
    case = Case(oracle, MIXED, SUBS, (40, 32), seed=17, epoch=0, cutout=8, flip_p=0.5, img_seed=4, junk=(3,))
    dec = _decoder([case])
    for use_lut in (False, True):
        got = _run(hip_lib, oracle, case, dec, use_lut)
        assert (got[3].view(np.uint8) == 0).all()


def test_geometry_change_on_one_context(hip_lib, oracle):
    """Two launches on one context with other crops and output sizes (and a
    different band count): the second cannot pass on the first one's records;
    then the first again."""
    a = Case(oracle, MIXED, SUBS, (40, 32), seed=19, epoch=0, cutout=8, flip_p=0.5, img_seed=8)
    b = Case(oracle, MIXED, SUBS, (17, 24), seed=19, epoch=1, scale=(0.3, 1.0), cutout=4, flip_p=0.5, img_seed=8)
    assert not np.array_equal(a.crops, b.crops)
    dec = _decoder([a, b])
    for case in (a, b, a):
        _run(hip_lib, oracle, case, dec, use_lut=True)


def test_tall_output_grows_the_record_buffer(hip_lib, oracle):
    """out_h 500 has 32 bands, twice what a context's record buffer starts
    with, and out_w + out_h is past the tap table: the linear walk computes
    its taps from the image record's scales."""
    case = Case(oracle, MIXED[:4], SUBS, (500, 32), seed=23, epoch=0, flip_p=0.5, img_seed=2)
    dec = _decoder([case])
    _run(hip_lib, oracle, case, dec)
    small = Case(oracle, MIXED[:4], SUBS, (17, 32), seed=23, epoch=1, img_seed=2)
    _run(hip_lib, oracle, small, dec)
