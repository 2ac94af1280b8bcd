"""GaussianBlur (DESIGN s19): what one launch of ffcv_gaussian_blur_batch costs
next to a device-to-device copy of the same bytes.

    python tools/blur_bench.py [--reps 60] [--rounds 3] [--warmup 10] [--ring-mb 640]

Shapes: 12,288 x 32 x 32 at k = 3 (the whole-image regime) and 512 x 224 x 224
at k = 23 (bands and column strips), sigma drawn per sample in [0.1, 2).

  blur   every sample applied
  copy   no sample applied: the launch's copy path
  d2d    the yardstick: one device-to-device copy of the same bytes

From HIP events around each launch.  The three variants alternate inside each
repetition after a warm-up of each; every launch takes the next source and
destination of rings of batches of --ring-mb each (more than the 256 MB
Infinity Cache), so no launch finds its input in a cache.  Per variant: the
median / min / max over --rounds of the per-round median microseconds, and the
algorithmic bytes (one read and one write of the batch) per second against the
8.0 TB/s HBM peak.  The blurred output is checked against the host twin on a
few images first.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((12288, 32, 32, 3), (512, 224, 224, 23))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--ring-mb', type=int, default=640)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    for B, H, W, ksize in CASES:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        src = [ch.randint(0, 256, (B, H, W, 3), dtype=ch.uint8, device=dev, generator=gen) for _ in range(nring)]
        dst = [ch.zeros((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
        ids = ch.arange(B, dtype=ch.int64, device=dev) * 7
        drawn = ch.empty((B,), dtype=ch.uint8, device=dev)
        sigma = ch.empty((B,), dtype=ch.float64, device=dev)
        weights = ch.empty((B, L.BLUR_WROW), dtype=ch.float32, device=dev)
        L.blur_draw_batch(ids, 1, 0, 1.0, 0.1, 2.0, ksize, drawn, sigma, weights)
        on, off = ch.ones((B,), dtype=ch.uint8, device=dev), ch.zeros((B,), dtype=ch.uint8, device=dev)

        def run(i, name):
            s, d = src[i % nring], dst[i % nring]
            if name == 'd2d':
                d.copy_(s)
            else:
                L.gaussian_blur_batch(s, d, ksize, on if name == 'blur' else off, weights)
        # the launch computes what the host twin computes
        run(0, 'blur')
        ch.cuda.synchronize()
        host = np.empty((4, H, W, 3), np.uint8)
        L.gaussian_blur_batch_host(src[0][:4].cpu().numpy(), host, ksize, np.ones(4, np.uint8),
                                   weights[:4].cpu().numpy())
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'ksize': ksize, 'bytes': 2 * nbytes, 'ring': nring,
               'strip_cols': L.gaussian_blur_strip_cols(H, W, ksize),
               'whole_image': 15 * H * W <= L.gaussian_blur_lds_bytes(),
               'config': f'{args.reps} launches x {args.rounds} rounds',
               'equals_host_twin': bool(np.array_equal(dst[0][:4].cpu().numpy(), host))}
        run(0, 'copy')
        ch.cuda.synchronize()
        res['copy_equals_input'] = bool(ch.equal(dst[0], src[0]))
        variants = ('blur', 'copy', 'd2d')
        for name in variants:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            evs = {name: [] for name in variants}
            for i in range(args.reps):
                for j, name in enumerate(variants):
                    a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                    a.record()
                    run(3 * i + j, name)
                    b.record()
                    evs[name].append((a, b))
            ch.cuda.synchronize()
            for name in variants:
                medians[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[name]])))
        for name in variants:
            m = medians[name]
            med = float(np.median(m))
            res[name] = {'median': round(med, 1), 'min': round(min(m), 1), 'max': round(max(m), 1),
                         'of_hbm_peak': round(2 * nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        res['blur_over_d2d'] = round(res['blur']['median'] / res['d2d']['median'], 2)
        res['copy_over_d2d'] = round(res['copy']['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del src, dst


if __name__ == '__main__':
    main()
