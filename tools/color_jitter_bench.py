"""Device colour jitter (DESIGN s14): per-launch device time of
ffcv_color_jitter_batch from HIP events, through the C ABI.

CIFAR shape (12,288 images of 32 x 32, the one-workgroup regime):
  fused3        brightness -> contrast -> saturation as ONE launch
  separate3     the same three steps as three single-step launches
  brightness    one brightness-only launch
  lut_u8        ffcv_lut_batch with a uint8 [256][3] table over the same
                bytes: an existing u8 -> u8 table pass of identical traffic,
                the yardstick for the brightness-only launch
C3 shape (512 images of 224 x 224, the tiled regime):
  c3_contrast   brightness -> contrast -> saturation: two passes
  c3_pointwise  brightness -> saturation: one pointwise pass

Every variant works on a ring of buffers larger than the 256 MiB Infinity
Cache, so a launch reads from and writes to HBM; the variants of a shape
alternate inside each repetition, and the whole measurement is repeated
--rounds times to show the run-to-run spread.  All steps apply (apply = 1),
ratios are uniform on [0.6, 1.4].  Prints one JSON line: per variant the
median / min / max over rounds of the per-round median microseconds, the
algorithmic bytes (one read and one write of the batch per pass) and that
traffic's share of the 8.0 TB/s HBM peak at the median.

--only NAME --iters N runs N launches of one variant and nothing else (for a
counter run under a profiler).

    python tools/color_jitter_bench.py [--reps 50] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s (spec)
RING_BYTES = 600 << 20
B, C, S = 1, 2, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50, help='timed launches per variant and round')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    import torch as ch
    assert ch.cuda.is_available(), 'color_jitter_bench needs the GPU (no CPU fallback)'
    from ffcv_amd import libffcv as L
    dev = ch.device('cuda:0')
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)

    def shape_setup(batch, h, w):
        nb = batch * h * w * 3
        ring = [ch.randint(0, 256, (batch, h, w, 3), dtype=ch.uint8, device=dev, generator=gen)
                for _ in range(max(2, -(-RING_BYTES // nb)))]
        apply = ch.ones((3, batch), dtype=ch.uint8, device=dev)
        ratio = (ch.rand((3, batch), dtype=ch.float64, device=dev, generator=gen) * 0.8 + 0.6)
        ws = ch.zeros((batch,), dtype=ch.int64, device=dev)
        return ring, apply, ratio, ws, nb

    variants = {}   # name -> (fn(i), passes)
    ring1, apply1, ratio1, ws1, nb1 = shape_setup(12288, 32, 32)
    out1 = ch.empty_like(ring1[0])
    lut = ch.randint(0, 256, (256, 3), dtype=ch.uint8, device=dev, generator=gen)
    variants['fused3'] = (lambda i: L.color_jitter_batch(ring1[i % len(ring1)], [B, C, S], apply1, ratio1), 1, nb1)

    def separate3(i):
        im = ring1[i % len(ring1)]
        for j, k in enumerate((B, C, S)):
            L.color_jitter_batch(im, [k], apply1[j:j + 1], ratio1[j:j + 1])
    variants['separate3'] = (separate3, 3, nb1)
    variants['brightness'] = (lambda i: L.color_jitter_batch(ring1[i % len(ring1)], [B], apply1, ratio1), 1, nb1)
    variants['lut_u8'] = (lambda i: L.lut_batch(ring1[i % len(ring1)], lut, out1), 1, nb1)
    ring3, apply3, ratio3, ws3, nb3 = shape_setup(512, 224, 224)
    variants['c3_contrast'] = (lambda i: L.color_jitter_batch(ring3[i % len(ring3)], [B, C, S], apply3, ratio3, ws3),
                               2, nb3)
    variants['c3_pointwise'] = (lambda i: L.color_jitter_batch(ring3[i % len(ring3)], [B, S], apply3, ratio3), 1, nb3)

    if args.only:
        fn = variants[args.only][0]
        for i in range(args.iters):
            fn(i)
        ch.cuda.synchronize()
        print(json.dumps({'only': args.only, 'iters': args.iters, 'batch_bytes': variants[args.only][2]}))
        return

    for name, (fn, _, _) in variants.items():
        for i in range(args.warmup):
            fn(i)
    ch.cuda.synchronize()
    medians = {name: [] for name in variants}
    for _ in range(args.rounds):
        evs = {name: [] for name in variants}
        for i in range(args.reps):
            for name, (fn, _, _) in variants.items():   # the variants alternate
                a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                a.record()
                fn(i)
                b.record()
                evs[name].append((a, b))
        ch.cuda.synchronize()
        for name, pairs in evs.items():
            medians[name].append(float(np.median([a.elapsed_time(b) for a, b in pairs])) * 1e3)
    res = {'config': 'colour jitter: 12,288 x 32x32 (one workgroup per image) and 512 x 224x224 (tiles); '
                     f'{args.reps} launches x {args.rounds} rounds, ring of {RING_BYTES >> 20} MiB',
           'lds_bytes': L.color_jitter_lds_bytes(), 'unit': 'us', 'variants': {}}
    for name, (_, passes, nb) in variants.items():
        m = np.array(medians[name])
        traffic = 2 * nb * passes
        res['variants'][name] = {'median_us': round(float(np.median(m)), 2), 'min_us': round(float(m.min()), 2),
                                 'max_us': round(float(m.max()), 2), 'passes': passes, 'bytes': traffic,
                                 'hbm_fraction': round(traffic / (float(np.median(m)) * 1e-6) / HBM_PEAK, 4)}
    res['value'] = res['variants']['fused3']['median_us']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
