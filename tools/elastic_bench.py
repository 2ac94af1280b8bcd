"""ElasticTransform (DESIGN s33): what one launch of ffcv_elastic_batch costs
next to ffcv_affine_batch on the same batch and to a device-to-device copy of
the same bytes.

    python tools/elastic_bench.py [--reps 30] [--rounds 3] [--warmup 5] [--ring-mb 640] [--lib PATH]

Shapes: 512 x 32 x 32 and 256 x 224 x 224, uniformly random pixels, the
default arguments (alpha 50, sigma 5).

  bilinear, nearest   ffcv_elastic_batch
  affine_bilinear, affine_nearest   ffcv_affine_batch, degrees=30
  d2d                 one device-to-device copy of the same bytes

From HIP events around each launch.  The variants alternate inside each
repetition after a warm-up of each; every launch takes the next source and
destination of rings of --ring-mb each (more than twice the 256 MB Infinity
Cache), so no launch finds its input in a cache.  Per variant: the median /
min / max over --rounds of the per-round median microseconds, and the ratios
to the affine launch of the same mode and to the copy.  The output is checked
against the host twin on a few images first, and the share of tiles per regime
is printed (from 16 samples).  --lib times a variant library.  Prints one JSON
line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 224, 224))
FILL = (7, 130, 251)
ALPHA, SIGMA = 50.0, 5.0


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
    th, tw = L.elastic_tile_shape()
    lds = L.elastic_tile_lds()
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
        acoef = ch.empty((B, 6), dtype=ch.int64, device=dev)
        L.affine_draw_batch(ids, 1, 0, 1.0, (-30.0, 30.0, 0, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 0), H, W, drawn, acoef)
        modes = {'bilinear': L.AFFINE_BILINEAR, 'nearest': L.AFFINE_NEAREST}

        def run(i, name):
            s, d = src[i % nring], dst[i % nring]
            if name == 'd2d':
                d.copy_(s)
            elif name.startswith('affine_'):
                L.affine_batch(s, d, modes[name[7:]], FILL, on, acoef)
            else:
                L.elastic_batch(s, d, modes[name], FILL, ids, 1, 0, ALPHA, SIGMA)
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring,
               'tile': f'{th}x{tw}', 'tile_lds': lds, 'lds_bytes': L.elastic_lds_bytes(H, W, SIGMA),
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        before, hids = src[0][:4].cpu().numpy(), ids[:4].cpu().numpy().astype(np.uint64)
        for name, mode in modes.items():          # the launches compute what the host twin computes
            run(0, name)
            ch.cuda.synchronize()
            want = L.elastic_batch_host(before, np.empty_like(before), mode, FILL, hids, 1, 0, ALPHA, SIGMA)
            res[name + '_equals_host_twin'] = bool(np.array_equal(dst[0][:4].cpu().numpy(), want))
        sizes = np.array([L.elastic_tile_bytes(H, W, 0, 7 * k, 1, 0, ALPHA, SIGMA, r, c) for k in range(16)
                          for r in range(-(-H // th)) for c in range(-(-W // tw))], dtype=np.float64)
        res['staged_tile_share'] = round(float(np.mean((sizes > 0) & (sizes <= lds))), 3)
        res['direct_tile_share'] = round(float(np.mean(sizes > lds)), 3)
        res['staged_bytes_mean'] = round(float(sizes.mean()), 1)
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
