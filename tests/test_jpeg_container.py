"""The CPU decoder on JPEG container layouts Pillow never writes.

tests/jpeg_surgery.py takes Pillow streams apart and rebuilds them with other
containers around the same entropy-coded bytes.  Every accepted variant must
decode in libjpeg-turbo itself (which keeps a broken builder from passing
vacuously) and `imdecode` must equal it bit for bit; container-only variants
must also leave the pixels and the coefficients of the base stream unchanged.
Every rejected variant must fail in both, except DRI 4, which libjpeg-turbo
decodes (zero blocks after the first restart interval, whose RST never
comes) and `imdecode` must follow.  tests/test_jpeg_container_gpu.py runs the
same variants through K1, K1b and K2.
"""
import os
import re

import numpy as np
import pytest

from tests import jpeg_surgery as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every variant name; each must be built from at least one base stream
ACCEPT_NAMES = ['com0', 'com1', 'com2', 'com3', 'app1_first', 'app1_before_sos', 'app2_straddle', 'fill3',
                'dqt_merged', 'dht_merged', 'dqt16', 'sof1', 'dri0', 'trailing', 'no_eoi', 'ids23', 'six_slots',
                'unused_id3', 'dc0_twice', 'gray22', 'gray41', 'rgb_ids', 'adobe0', 'adobe1',
                'l440', 'l411', 'l1x4', 'dims']
REJECT_NAMES = ['dht_overrun', 'dht_overrun_std', 'dqt_short', 'sos_first', 'no_dqt', 'no_dht', 'nonintegral',
                'prec12', 'four_comp', 'dri4']
# 7 colour bases x 22 + 2 grey x 20 container / colour variants, 18 layout variants, 9 small layouts
N_ACCEPT = 7 * 22 + 2 * 20 + 18 + 9
# 10 per colour base with standard tables, 9 with optimised ones, 8 per grey base
N_REJECT = 6 * 10 + 9 + 2 * 8


@pytest.fixture(scope='module')
def bases():
    return J.bases()


def _imdecode(L, blob, h, w):
    out = np.zeros((h, w, 3), np.uint8)
    return L.imdecode(blob, out, h, w), out


def test_surgery_round_trip(bases):
    assert ACCEPT_NAMES == J.ACCEPT and REJECT_NAMES == J.REJECT
    src = open(os.path.join(ROOT, 'ffcv_amd', 'csrc', 'jpeg_defs.h')).read()
    assert int(re.search(r'^#define HDR_BYTES (\d+)', src, re.M).group(1)) == J.HDR_BYTES
    for b in bases:
        segs, scan = J.split(b.blob)
        assert segs[-1][0] == J.SOS and scan[-2:] == b'\xff\xd9'
        assert np.array_equal(J.join(segs, scan), b.blob), b.name
        offs, scan_off = J.offsets(segs, 3)
        blob = J.join(segs, scan, 3)
        assert all(blob[o] == 0xFF and blob[o + 1] == m for o, (m, _) in zip(offs, segs))
        assert bytes(blob[scan_off:]) == scan


def test_base_streams(hip_lib, bases):
    """Streams on both sides of 1.5 KB of entropy-coded data (K1 uses fewer
    than 64 lanes below it), and the stuffing the noise streams are there for."""
    from ffcv_amd import libffcv as L
    ecs = L.jpeg_scan_stats([b.blob for b in bases])[:, 2].astype(np.int64)
    assert (ecs > 0).all() and (ecs < 1536).sum() >= 3 and (ecs > 1536).sum() >= 3, ecs
    for b in bases:
        if b.name.startswith('noise'):
            scan = J.split(b.blob)[1]
            assert scan.count(b'\xff\x00') * 200 >= len(scan), b.name  # about one byte in 256 is 0xFF


def test_accepted_variants(hip_lib, oracle, bases):
    from ffcv_amd import libffcv as L
    ran, names = 0, set()
    for b in bases:
        ref = oracle.ljt_decode(b.blob)
        ref_co = L.cpu_jpeg_coefficients(b.blob)
        for v in J.accepted(b):
            want = oracle.ljt_decode(v.blob)  # raises if libjpeg-turbo rejects the variant
            assert want.shape == (v.h, v.w, 3), v.name
            rc, got = _imdecode(L, v.blob, v.h, v.w)
            assert rc == 0, (v.name, L.lib().ffcv_last_error())
            assert np.array_equal(got, want), v.name
            if v.group == 'container':
                assert np.array_equal(want, ref), v.name
                assert np.array_equal(L.cpu_jpeg_coefficients(v.blob), ref_co), v.name
            elif v.group == 'colour' and not v.name.endswith('adobe1'):
                assert not np.array_equal(want, ref), v.name  # decoded as RGB: no colour conversion
            ran += 1
            names.add(v.name.split('/')[1])
    for v in J.small_layouts():
        want = oracle.ljt_decode(v.blob)
        rc, got = _imdecode(L, v.blob, v.h, v.w)
        assert rc == 0 and np.array_equal(got, want), v.name
        ran += 1
    assert names == set(ACCEPT_NAMES), names ^ set(ACCEPT_NAMES)
    assert ran == N_ACCEPT, ran


def test_rejected_variants(hip_lib, oracle, bases):
    from ffcv_amd import libffcv as L
    ran, names = 0, set()
    for b in bases:
        t = J.trimmed(b)
        if t is not None:  # the stream dht_overrun is made from is a valid one
            assert np.array_equal(oracle.ljt_decode(t), oracle.ljt_decode(b.blob)), b.name
        for r in J.rejected(b):
            if r.cpu_decodes:
                want = oracle.ljt_decode(r.blob)
                rc, got = _imdecode(L, r.blob, r.h, r.w)
                assert rc == 0 and np.array_equal(got, want), r.name
            else:
                with pytest.raises(ValueError):
                    oracle.ljt_decode(r.blob)
                rc, _ = _imdecode(L, r.blob, r.h, r.w)
                assert rc == -1, r.name
            ran += 1
            names.add(r.name.split('/')[1])
    assert names == set(REJECT_NAMES), names ^ set(REJECT_NAMES)
    assert ran == N_REJECT, ran


def test_truncated_scan_matches_libjpeg(hip_lib, oracle, bases):
    """A scan cut short: libjpeg-turbo finishes the MCU in progress on zero
    bits and leaves the later MCUs zero (grey), and so must imdecode (it went
    on decoding zero bits for every later MCU before).  The MCU in progress is
    left out of the pixel comparison: real bits followed by zeros give blocks
    (63 coefficients of -1 beside one near -1023) on which libjpeg-turbo's
    16-bit SIMD IDCT wraps and its C form does not, as on 0 / 255 noise
    (tests/test_k1_write_chunks_gpu.py); its neighbours within one chroma
    sample (fancy upsampling) go with it."""
    from ffcv_amd import libffcv as L
    geom = {'4:2:0': (2, 2, 6), '4:2:2': (2, 1, 4), '4:4:4': (1, 1, 3), 'gray': (1, 1, 1)}
    ran = partial = 0
    for b in bases:
        off = J.offsets(J.split(b.blob)[0])[1]
        n = len(b.blob) - off
        hs, vs, bpm = geom[b.sub]
        mcux = -(-b.w // (8 * hs))
        full = L.cpu_jpeg_coefficients(b.blob)
        for cut in sorted({off, off + 1, off + n // 3, off + n // 2, off + n // 2 + 1, len(b.blob) - 3}):
            want = oracle.ljt_decode(b.blob[:cut])
            rc, got = _imdecode(L, b.blob[:cut], b.h, b.w)
            assert rc == 0, (b.name, cut)
            co = L.cpu_jpeg_coefficients(b.blob[:cut])
            assert co.shape == full.shape
            differ = np.nonzero((co != full).any(1))[0]
            keep = np.ones((b.h, b.w), bool)
            if differ.size:
                m = int(differ[0]) // bpm  # the MCU the data ran out in; every later one is zero
                assert np.array_equal(co[:m * bpm], full[:m * bpm]) and not co[(m + 1) * bpm:].any(), (b.name, cut)
                y, x = (m // mcux) * 8 * vs, (m % mcux) * 8 * hs
                keep[max(0, y - 2):y + 8 * vs + 2, max(0, x - 2):x + 8 * hs + 2] = False
                partial += 1
            assert np.array_equal(got[keep], want[keep]), (b.name, cut)
            ran += 1
    assert ran >= 5 * len(bases) and partial >= 4 * len(bases), (ran, partial)
