"""RandomAffine (DESIGN s21): what one launch of ffcv_affine_batch costs next
to a device-to-device copy of the same bytes.

    python tools/affine_bench.py [--reps 40] [--rounds 3] [--warmup 10] [--ring-mb 640] [--lib PATH]

Shapes: 12,288 x 32 x 32 (the whole-image regime) and 512 x 224 x 224 (tiles),
uniformly random pixels, coefficients drawn per sample by ffcv_affine_draw_batch.

  bilinear  degrees=30, every sample applied
  nearest   the same coefficients under nearest
  none      no sample applied: the launch copies
  minify    degrees=0, translate=(0.25, 0.25), scale=(0.5, 2.0), shear=(-20, 20,
            0, 0), bilinear, every sample applied (the share of its tiles that
            the direct regime takes is printed)
  quarter   degrees=10, scale=(0.25, 0.25), bilinear, every sample applied:
            minification by 4, whose tiles inside the image all exceed the LDS
            budget and read global memory directly (share printed)
  d2d       the yardstick: one device-to-device copy of the same bytes

From HIP events around each variant.  The variants alternate inside each
repetition after a warm-up of each; every launch takes the next source and
destination of rings of --ring-mb each (more than the 256 MB Infinity Cache),
so no launch finds its input in a cache.  Per variant: the median / min / max
over --rounds of the per-round median microseconds, the algorithmic bytes (one
read and one write of the batch) per second against the 8.0 TB/s HBM peak, and
the ratio to the copy.  The output is checked against the host twin on a few
images first.  --lib times a variant library (python -m ffcv_amd._build --out
PATH -- -DAFFINE_TILE_ROWS=16 ...).  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((12288, 32, 32), (512, 224, 224))
HBM_PEAK = 8.0e12
FILL = (7, 130, 251)


def ranges(H, W, deg, translate=(0.0, 0.0), scale=(1.0, 1.0), shear=(0.0, 0.0, 0.0, 0.0)):
    tw, th = translate[0] * W, translate[1] * H
    return (-deg, deg, -tw, tw, -th, th) + tuple(scale) + tuple(shear)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--ring-mb', type=int, default=640)
    ap.add_argument('--lib', help='a variant library to time instead of the product library')
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
    elif not os.path.exists(L.LIB_PATH):
        _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    th, tw = L.affine_tile_shape()
    for B, H, W in CASES:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        src = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
        dst = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
        for t in src:
            t.random_(0, 256, generator=gen)
        ids = ch.arange(B, dtype=ch.int64, device=dev) * 7
        on, off = ch.ones((B,), dtype=ch.uint8, device=dev), ch.zeros((B,), dtype=ch.uint8, device=dev)
        drawn = ch.empty((B,), dtype=ch.uint8, device=dev)
        coef = {name: ch.empty((B, 6), dtype=ch.int64, device=dev) for name in ('rot', 'minify', 'quarter')}
        L.affine_draw_batch(ids, 1, 0, 1.0, ranges(H, W, 30.0), H, W, drawn, coef['rot'])
        L.affine_draw_batch(ids, 1, 0, 1.0, ranges(H, W, 0.0, (0.25, 0.25), (0.5, 2.0), (-20.0, 20.0, 0.0, 0.0)), H, W,
                            drawn, coef['minify'])
        L.affine_draw_batch(ids, 1, 0, 1.0, ranges(H, W, 10.0, scale=(0.25, 0.25)), H, W, drawn, coef['quarter'])
        variants = {'bilinear': (L.AFFINE_BILINEAR, on, 'rot'), 'nearest': (L.AFFINE_NEAREST, on, 'rot'),
                    'none': (L.AFFINE_BILINEAR, off, 'rot'), 'minify': (L.AFFINE_BILINEAR, on, 'minify'),
                    'quarter': (L.AFFINE_BILINEAR, on, 'quarter')}

        def run(i, name):
            if name == 'd2d':
                dst[i % nring].copy_(src[i % nring])
            else:
                mode, apply, c = variants[name]
                L.affine_batch(src[i % nring], dst[i % nring], mode, FILL, apply, coef[c])
        whole = nbytes // B <= L.affine_whole_bytes()
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring, 'whole_image': whole,
               'tile': f'{th}x{tw}', 'tile_lds': L.affine_tile_lds(),
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        # the launches compute what the host twin computes
        before = src[0][:4].cpu().numpy()
        for name in variants:
            mode, apply, c = variants[name]
            run(0, name)
            ch.cuda.synchronize()
            want = np.empty_like(before)
            L.affine_batch_host(before, want, mode, FILL, apply[:4].cpu().numpy(), coef[c][:4].cpu().numpy())
            res[name + '_equals_host_twin'] = bool(np.array_equal(dst[0][:4].cpu().numpy(), want))
        if not whole:
            for name in ('minify', 'quarter'):
                q = coef[name][:64].cpu().numpy()
                sizes = [L.affine_tile_bytes(H, W, L.AFFINE_BILINEAR, q[k], r, c) for k in range(64)
                         for r in range(-(-H // th)) for c in range(-(-W // tw))]
                res[name + '_direct_tile_share'] = round(float(np.mean([s > L.affine_tile_lds() for s in sizes])), 3)
                res[name + '_empty_tile_share'] = round(float(np.mean([s == 0 for s in sizes])), 3)
        names = tuple(variants) + ('d2d',)
        for name in names:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in names}
        for _ in range(args.rounds):
            evs = {name: [] for name in names}
            for i in range(args.reps):
                for j, name in enumerate(names):
                    a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                    a.record()
                    run(len(names) * i + j, name)
                    b.record()
                    evs[name].append((a, b))
            ch.cuda.synchronize()
            for name in names:
                medians[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[name]])))
        for name in names:
            m = medians[name]
            med = float(np.median(m))
            res[name] = {'median': round(med, 1), 'min': round(min(m), 1), 'max': round(max(m), 1),
                         'of_hbm_peak': round(2 * nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        for name in variants:
            res[name + '_over_d2d'] = round(res[name]['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del src, dst


if __name__ == '__main__':
    main()
