"""RandomPerspective (DESIGN s32): what one launch of ffcv_perspective_batch
costs next to ffcv_affine_batch on the same batch and to a device-to-device
copy of the same bytes.

    python tools/perspective_bench.py [--reps 30] [--rounds 3] [--warmup 5] [--ring-mb 640] [--lib PATH]

Shapes: 512 x 32 x 32 and 256 x 64 x 64 (the whole-image regime), 256 x 128 x
128 and 256 x 224 x 224 (tiles), uniformly random pixels, coefficients drawn
per sample by ffcv_perspective_draw_batch at distortion_scale 0.5, every
sample applied.

  bilinear, nearest   ffcv_perspective_batch
  affine_bilinear, affine_nearest   ffcv_affine_batch, degrees=30
  d2d                 one device-to-device copy of the same bytes

From HIP events around each launch.  The variants alternate inside each
repetition after a warm-up of each; every launch takes the next source and
destination of rings of --ring-mb each (more than twice the 256 MB Infinity
Cache), so no launch finds its input in a cache.  Per variant: the median /
min / max over --rounds of the per-round median microseconds, and the ratios
to the affine launch of the same mode and to the copy.  The output is checked
against the host twin on a few images first, and the share of tiles per regime
is printed.  --lib times a variant library (python -m ffcv_amd._build --out
PATH -- -DPERSP_TILE_LDS=32768 ...).  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 64, 64), (256, 128, 128), (256, 224, 224))
FILL = (7, 130, 251)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ring-mb', type=int, default=640)
    ap.add_argument('--shapes', type=int, nargs='*', help='indices into the shapes, default all')
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
    th, tw = L.perspective_tile_shape()
    lds = L.perspective_tile_lds()
    for B, H, W in [CASES[i] for i in (args.shapes or range(len(CASES)))]:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        src = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
        dst = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
        for t in src:
            t.random_(0, 256, generator=gen)
        ids = ch.arange(B, dtype=ch.int64, device=dev) * 7
        on = ch.ones((B,), dtype=ch.uint8, device=dev)
        drawn = ch.empty((B,), dtype=ch.uint8, device=dev)
        coef = ch.empty((B, 9), dtype=ch.float64, device=dev)
        acoef = ch.empty((B, 6), dtype=ch.int64, device=dev)
        L.perspective_draw_batch(ids, 1, 0, 1.0, 0.5, H, W, drawn, coef)
        L.affine_draw_batch(ids, 1, 0, 1.0, (-30.0, 30.0, 0, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 0), H, W, drawn, acoef)
        modes = {'bilinear': L.AFFINE_BILINEAR, 'nearest': L.AFFINE_NEAREST}

        def run(i, name):
            s, d = src[i % nring], dst[i % nring]
            if name == 'd2d':
                d.copy_(s)
            elif name.startswith('affine_'):
                L.affine_batch(s, d, modes[name[7:]], FILL, on, acoef)
            else:
                L.perspective_batch(s, d, modes[name], FILL, on, coef)
        whole = nbytes // B <= L.perspective_whole_bytes()
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring, 'whole_image': whole,
               'tile': f'{th}x{tw}', 'tile_lds': lds, 'config': f'{args.reps} launches x {args.rounds} rounds'}
        before, q = src[0][:4].cpu().numpy(), coef[:64].cpu().numpy()
        for name, mode in modes.items():          # the launches compute what the host twin computes
            run(0, name)
            ch.cuda.synchronize()
            want = L.perspective_batch_host(before, np.empty_like(before), mode, FILL, np.ones(4, np.uint8), q[:4])
            res[name + '_equals_host_twin'] = bool(np.array_equal(dst[0][:4].cpu().numpy(), want))
        if not whole:
            sizes = np.array([L.perspective_tile_bytes(H, W, 0, q[k], r, c) for k in range(len(q))
                              for r in range(-(-H // th)) for c in range(-(-W // tw))], dtype=np.float64)
            res['staged_tile_share'] = round(float(np.mean((sizes > 0) & (sizes <= lds))), 3)
            res['direct_tile_share'] = round(float(np.mean(sizes > lds)), 3)
            res['empty_tile_share'] = round(float(np.mean(sizes == 0)), 3)
        names = ('bilinear', 'affine_bilinear', 'nearest', 'affine_nearest', 'd2d')
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
            res[name] = {'median': round(float(np.median(m)), 1), 'min': round(min(m), 1), 'max': round(max(m), 1)}
        for name in modes:
            res[name + '_over_affine'] = round(res[name]['median'] / res['affine_' + name]['median'], 2)
            res[name + '_over_d2d'] = round(res[name]['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del src, dst


if __name__ == '__main__':
    main()
