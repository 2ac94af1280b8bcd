"""RandomHue / RandomColorJitter (DESIGN s20): what one launch of
ffcv_hue_batch, and all launches of the joint colour jitter, cost next to a
device-to-device copy of the same bytes.

    python tools/hue_bench.py [--reps 60] [--rounds 3] [--warmup 10] [--ring-mb 640]

Shapes: 12,288 x 32 x 32 (the whole-image regime) and 512 x 224 x 224 (tiles of
4,096 pixels), uniformly random pixels (nearly all of them coloured: the full
per-pixel arithmetic), a shift drawn per sample in [-0.1, 0.1).

  hue    ffcv_hue_batch, every sample applied
  skip   ffcv_hue_batch, no sample applied: workgroups that return at once
  joint  RandomColorJitter(0.4, 0.4, 0.2, 0.1), every sample applied, ALL its
         launches: the joint draw, ffcv_color_jitter_batch (brightness,
         contrast, saturation: one launch for 32 x 32; a memset and two for
         224 x 224) and ffcv_hue_batch
  d2d    the yardstick: one device-to-device copy of the same bytes

From HIP events around each variant.  The four variants alternate inside each
repetition after a warm-up of each; every launch takes the next batch of rings
of --ring-mb each (more than the 256 MB Infinity Cache), so no launch finds its
input in a cache.  The operations work in place, so the rings of `hue` and
`joint` are refilled with random pixels before every round; the share of gray
pixels (which skip the arithmetic) in the ring at the end is printed.  Per
variant: the median / min / max over --rounds of the per-round median
microseconds, and the algorithmic bytes (one read and one write of the batch)
per second against the 8.0 TB/s HBM peak.  The output of both is checked
against the host twins on a few images first.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((12288, 32, 32), (512, 224, 224))
MAGS = (0.4, 0.4, 0.2, 0.1)
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
    for B, H, W in CASES:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        rings = {name: [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
                 for name in ('hue', 'joint', 'dst')}

        def refill():
            for name in ('hue', 'joint'):
                for t in rings[name]:
                    t.random_(0, 256, generator=gen)
        refill()
        ids = ch.arange(B, dtype=ch.int64, device=dev) * 7
        on, off = ch.ones((B,), dtype=ch.uint8, device=dev), ch.zeros((B,), dtype=ch.uint8, device=dev)
        drawn = ch.empty((B,), dtype=ch.uint8, device=dev)
        shift = ch.empty((B,), dtype=ch.float64, device=dev)
        L.hue_draw_batch(ids, 1, 0, 1.0, 0.1, drawn, shift)
        japply = ch.empty((4, B), dtype=ch.uint8, device=dev)
        jratio = ch.empty((4, B), dtype=ch.float64, device=dev)
        ws = ch.empty((B,), dtype=ch.int64, device=dev) if H * W * 3 > L.color_jitter_lds_bytes() else None

        def run(i, name):
            if name == 'd2d':
                rings['dst'][i % nring].copy_(rings['hue'][i % nring])
            elif name == 'joint':
                im = rings['joint'][i % nring]
                L.color_jitter_joint_draw_batch(ids, 1, 0, 1.0, MAGS, japply, jratio)
                L.color_jitter_batch(im, [L.CJ_BRIGHTNESS, L.CJ_CONTRAST, L.CJ_SATURATION], japply, jratio, ws)
                L.hue_batch(im, japply[3], jratio[3])
            else:
                L.hue_batch(rings['hue'][i % nring], on if name == 'hue' else off, shift)
        # the launches compute what the host twins compute
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring,
               'whole_image': H * W * 3 <= L.color_jitter_lds_bytes(),
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        before = rings['hue'][0][:4].cpu().numpy()
        jbefore = rings['joint'][0][:4].cpu().numpy()
        whole = rings['hue'][0].clone()
        run(0, 'skip')
        ch.cuda.synchronize()
        res['skip_leaves_input'] = bool(ch.equal(rings['hue'][0], whole))
        del whole
        run(0, 'hue')
        run(0, 'joint')
        ch.cuda.synchronize()
        L.hue_batch_host(before, np.ones(4, np.uint8), shift[:4].cpu().numpy())
        res['hue_equals_host_twin'] = bool(np.array_equal(rings['hue'][0][:4].cpu().numpy(), before))
        ja, jr = japply[:, :4].cpu().numpy(), jratio[:, :4].cpu().numpy()
        L.color_jitter_batch_host(jbefore, [1, 2, 3], ja[:3], jr[:3])
        L.hue_batch_host(jbefore, ja[3], jr[3])
        res['joint_equals_host_twins'] = bool(np.array_equal(rings['joint'][0][:4].cpu().numpy(), jbefore))
        variants = ('hue', 'skip', 'joint', 'd2d')
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
            med = float(np.median(m))
            res[name] = {'median': round(med, 1), 'min': round(min(m), 1), 'max': round(max(m), 1),
                         'of_hbm_peak': round(2 * nbytes / (med * 1e-6) / HBM_PEAK, 4)}
        for name in ('hue', 'skip', 'joint'):
            res[name + '_over_d2d'] = round(res[name]['median'] / res['d2d']['median'], 2)
            if name != 'skip':
                t = ch.cat([x.view(-1, 3) for x in rings[name]])
                res[name + '_gray_share_at_end'] = round(float(((t[:, 0] == t[:, 1]) & (t[:, 1] == t[:, 2]))
                                                               .float().mean()), 4)
                del t
        print(json.dumps(res), flush=True)
        del rings


if __name__ == '__main__':
    main()
