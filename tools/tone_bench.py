"""The table operations (DESIGN s22): what ffcv_tone_batch with [equalize]
costs next to ffcv_color_jitter_batch with [contrast], the nearest older launch
with a per-image statistic, and next to a device-to-device copy.

    python tools/tone_bench.py [--reps 60] [--rounds 3] [--warmup 10] [--ring-mb 640]

Shapes: 512 x 32 x 32 (the whole-image regime: one launch each) and 256 x 224 x
224 (tiles of 4,096 pixels: a memset and two launches each), every sample
applied.

  equalize   ffcv_tone_batch [equalize] on uniformly random pixels
  flat       the same on images whose channels are constant: every lane of a
             wave adds to one LDS counter
  contrast   ffcv_color_jitter_batch [contrast], ratio 1.3, random pixels
  d2d        one device-to-device copy of the same bytes

From HIP events around each variant, in one process.  The variants alternate
inside each repetition after a warm-up of each; every launch takes the next
batch of rings of --ring-mb each (more than the 256 MB Infinity Cache), so no
launch finds its input in a cache.  The operations work in place, so the rings
are refilled before every round.  Per variant: the median / min / max over
--rounds of the per-round median microseconds.  The outputs are checked against
the host twins on a few images first.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 224, 224))


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
    variants = ('equalize', 'flat', 'contrast', 'd2d')
    for B, H, W in CASES:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        rings = {name: [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
                 for name in ('equalize', 'flat', 'contrast', 'dst')}

        def refill():
            for name in ('equalize', 'contrast'):
                for t in rings[name]:
                    t.random_(0, 256, generator=gen)
            for t in rings['flat']:
                t[...] = ch.randint(0, 256, (B, 1, 1, 3), dtype=ch.uint8, device=dev, generator=gen)
        refill()
        on = ch.ones((1, B), dtype=ch.uint8, device=dev)
        ratio = ch.full((1, B), 1.3, dtype=ch.float64, device=dev)
        tiled = H * W * 3 > L.tone_lds_bytes()
        assert tiled == (H * W * 3 > L.color_jitter_lds_bytes())
        tws = ch.empty((L.tone_workspace_bytes(B) // 4,), dtype=ch.int32, device=dev) if tiled else None
        cws = ch.empty((B,), dtype=ch.int64, device=dev) if tiled else None

        def run(i, name):
            if name == 'd2d':
                rings['dst'][i % nring].copy_(rings['equalize'][i % nring])
            elif name == 'contrast':
                L.color_jitter_batch(rings['contrast'][i % nring], [L.CJ_CONTRAST], on, ratio, cws)
            else:
                L.tone_batch(rings[name][i % nring], [L.TONE_EQUALIZE], 8, on, tws)
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring,
               'whole_image': not tiled, 'config': f'{args.reps} launches x {args.rounds} rounds'}
        # the launches compute what the host twins compute
        before = {name: rings[name][0][:4].cpu().numpy() for name in ('equalize', 'flat', 'contrast')}
        for name in before:
            run(0, name)
        ch.cuda.synchronize()
        one = np.ones((1, 4), np.uint8)
        for name in ('equalize', 'flat'):
            L.tone_batch_host(before[name], [L.TONE_EQUALIZE], 8, one)
        L.color_jitter_batch_host(before['contrast'], [L.CJ_CONTRAST], one, np.full((1, 4), 1.3))
        res['equal_host_twins'] = all(bool(np.array_equal(rings[name][0][:4].cpu().numpy(), before[name]))
                                      for name in before)
        for name in variants:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            refill()
            ch.cuda.synchronize()
            evs = {name: [] for name in variants}
            for i in range(args.reps):
                for j, name in enumerate(variants):
                    a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                    a.record()
                    run(len(variants) * i + j, name)
                    b.record()
                    evs[name].append((a, b))
            ch.cuda.synchronize()
            for name in variants:
                medians[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[name]])))
        for name in variants:
            m = medians[name]
            res[name] = {'median': round(float(np.median(m)), 1), 'min': round(min(m), 1), 'max': round(max(m), 1)}
        for name in ('equalize', 'flat'):
            res[name + '_over_contrast'] = round(res[name]['median'] / res['contrast']['median'], 2)
        res['equalize_over_d2d'] = round(res['equalize']['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del rings


if __name__ == '__main__':
    main()
