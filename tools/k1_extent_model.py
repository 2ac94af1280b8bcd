"""Host model of K1's decode extent: which margin to add to the linear estimate.

K1 (entropy_passes) decodes the bits [0, E) of a scan,

    E = min(bits, bits / mcuy * need_rows + (bits >> 8) * REL + ABS),

where need_rows is the number of MCU rows up to the last one that holds a
block of the crop window, and decodes the whole scan again when the blocks of
those rows turn out to end past E.  This script takes the true end of every
MCU row from tools/sync_sim.c mode 13 and the crops from the oracle's draws
(the benchmark's RandomResizedCrop: scale 0.08-1, ratio 3/4-4/3), and prints,
for a grid of (REL, ABS), the mean decoded fraction, the fall-back rate and

    cost = mean(f) * (SYNC + WRITE) + mean(fell back ? E / bits : 0) * SYNC,
    f = 1 for a draw that falls back (it pays everything in full after the
    shortened rounds), else E / bits

in VALU instructions per image (round 1 12.6 k + later rounds
26 k = SYNC, write pass 29 k = WRITE).  A row counts as covered when it ends
at or before E (the kernel also completes a block whose last symbol starts
before E, so the fall-back rate printed is an upper bound).  Two inputs:

  bench  32 images of the benchmark's generator (natural_image /
         imagenet_like_shape(rng, 256), q90 4:2:0, default_rng(i * 37): the
         sample of profiles/k1_wchunk_model.txt)
  photo  32 views with a 256-px long side cut from the 1024x642 photograph of
         tests/golden/photo.npz (half at full, half at half resolution),
         re-encoded q90 4:2:0

    python tools/k1_extent_model.py > profiles/k1_extent_model.txt
"""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffcv_amd.synthetic import natural_image, imagenet_like_shape, encode_jpeg  # noqa: E402
from oracle import oracle as O  # noqa: E402

SYNC, WRITE = 12.6e3 + 26e3, 29e3
DRAWS = 4000  # per image
RELS = [0, 4, 8, 12, 16, 24, 32, 48]
ABSS = [0, 256, 512, 1024, 2048, 4096]


def need_rows_420(H, crops):
    """entropy_passes' need_rows for 4:2:0 (parse_header's window rows)."""
    last = crops[:, 0] + crops[:, 2] - 1
    luma = (last >> 3) >> 1
    ch = (H + 1) // 2
    chroma = np.minimum((last >> 1) + 1, ch - 1) >> 3
    return np.maximum(luma, chroma) + 1


def row_ends(exe, blob, d):
    f = os.path.join(d, 'x.jpg')
    np.asarray(blob).tofile(f)
    out = subprocess.run([exe, f, '64', '13'], check=True, capture_output=True, text=True).stdout
    line = [l for l in out.splitlines() if l.startswith('rows:')][0]
    head, rows = line.split('|')
    h = head.split()
    bits, mcuy = int(h[2]), int(h[6])
    ends = np.array([int(p.split(':')[1]) for p in rows.split()], np.int64)
    assert len(ends) == mcuy
    return bits, mcuy, ends


def bench_images():
    for i in range(32):
        rng = np.random.default_rng(i * 37)
        img = natural_image(rng, *imagenet_like_shape(rng, 256))
        yield img.shape[0], img.shape[1], encode_jpeg(img, 90, '4:2:0')


def photo_images():
    from PIL import Image
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'photo.npz'))
    k = list(g['cases']).index('1024x642 q90 4:2:0')
    big = Image.open(io.BytesIO(g['data'][g['offs'][k]:g['offs'][k + 1]].tobytes())).convert('RGB')
    srcs = [np.asarray(big), np.asarray(big.resize((512, 321), Image.BOX))]
    rng = np.random.default_rng(5)
    for i in range(32):
        src = srcs[i % 2]
        h, w = imagenet_like_shape(rng, 256)
        y, x = int(rng.integers(0, src.shape[0] - h + 1)), int(rng.integers(0, src.shape[1] - w + 1))
        yield h, w, encode_jpeg(np.ascontiguousarray(src[y:y + h, x:x + w]), 90, '4:2:0')


def main():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, 'sync_sim')
        subprocess.run([os.environ.get('CC', 'cc'), '-O2', '-o', exe, os.path.join(ROOT, 'tools', 'sync_sim.c')],
                       check=True)
        for name, gen in (('bench', bench_images), ('photo', photo_images)):
            per = []  # (bits, est[draw], true end[draw], full[draw])
            print(f'## {name}: MCU-row ends against the linear estimate (bits; true - estimate as % of the scan)')
            for i, (H, W, blob) in enumerate(gen()):
                bits, mcuy, ends = row_ends(exe, blob, d)
                est_r = bits // mcuy * np.arange(1, mcuy + 1)
                dev = (ends - est_r) / bits * 100
                print(f'image {i:2d} {H}x{W} {len(blob)} B bits {bits} mcuy {mcuy} | dev% min {dev[:-1].min():+.2f} '
                      f'max {dev[:-1].max():+.2f} | ' + ' '.join(f'{x:+.1f}' for x in dev))
                crops, _ = O.draw_batch(np.arange(DRAWS) + i * DRAWS, [H] * DRAWS, [W] * DRAWS, 0, 0)
                nr = need_rows_420(H, crops.astype(np.int64))
                assert nr.max() <= mcuy
                per.append((bits, est_r[nr - 1], ends[nr - 1], nr == mcuy, nr / mcuy))
            frac_rows = np.concatenate([p[4] for p in per])
            full = np.concatenate([p[3] for p in per])
            print(f'{name}: {len(per)} images x {DRAWS} draws: needed MCU rows / all, mean {frac_rows.mean():.3f}; '
                  f'crops that reach the last MCU row {full.mean() * 100:.1f}%')
            print(f'{name}: REL ABS | mean E/bits  P(fall-back)%  cost (VALU / image)  saving vs full {SYNC + WRITE:.0f}')
            best = None
            for rel in RELS:
                for ab in ABSS:
                    fr, fb = [], []
                    for bits, est, end, isfull, _ in per:
                        E = np.minimum(bits, est + (bits >> 8) * rel + ab)
                        E = np.where(isfull, bits, E)
                        fell = (end > E) & ~isfull
                        fr.append(E / bits)
                        fb.append(fell)
                    fr, fb = np.concatenate(fr), np.concatenate(fb)
                    # a fall-back pays the shortened rounds, then everything in full
                    cost = (np.where(fb, 1.0, fr).mean()) * (SYNC + WRITE) + (fb * fr).mean() * SYNC
                    print(f'{name}: {rel:3d} {ab:4d} | {fr.mean():.4f}  {fb.mean() * 100:6.3f}  {cost:8.0f}  '
                          f'{SYNC + WRITE - cost:7.0f}')
                    if best is None or cost < best[0]:
                        best = (cost, rel, ab, fr.mean(), fb.mean())
            print(f'{name}: best REL {best[1]} ABS {best[2]}: mean E/bits {best[3]:.4f}, fall-back {best[4] * 100:.3f}%, '
                  f'cost {best[0]:.0f}, saving {SYNC + WRITE - best[0]:.0f} VALU / image')


if __name__ == '__main__':
    main()
