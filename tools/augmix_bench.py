"""AugMix (DESIGN s28): what the fused path (the draw launches and ONE pixel
launch: up to 64 x 64 the original stays in LDS, the chains run there and the
mix is in registers; beyond, persistent workgroups with one image buffer in
LDS pass the chains' results through a slab of memory each) costs next to the
rounds path (the draw launches, per chain a copy
and three rounds of the five pixel launches of TrivialAugmentWide, then the
streaming mix) and next to a device-to-device copy.

    python tools/augmix_bench.py [--reps 40] [--rounds 3] [--warmup 5] [--ring-mb 640] [--width 3]

Shapes: 512 x 32 x 32 and 256 x 64 x 64 (the edge of ffcv_augmix_batch), and
256 x 128 x 128 and 256 x 224 x 224 (ffcv_augmix_large_batch, a workspace of
ffcv_augmix_large_workspace_bytes), uniformly random pixels, severity 3, random
depth, alpha 1, nearest.

  fused   ffcv_augmix_draw_batch, ffcv_augmix_batch or ffcv_augmix_large_batch
  rounds  ffcv_augmix_draw_batch, then the operation's launches beyond the
          fused regime (the baseline: existing kernels and ffcv_augmix_mix_batch)
  d2d     one device-to-device copy of the same bytes

By the method of tools/randaugment_bench.py: HIP events around each variant in
one process, the variants alternating inside each repetition after a warm-up of
each, every launch on the next batch of rings of --ring-mb each (more than the
256 MB Infinity Cache).  Per variant: the median / min / max over --rounds of
the per-round median microseconds.  First the two paths' outputs are checked
equal on the whole batch.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 64, 64), (256, 128, 128), (256, 224, 224))
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)
SEVERITY, DEPTH, ALPHA, SEED = 3, -1, 1.0, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ring-mb', type=int, default=640)
    ap.add_argument('--width', type=int, default=3)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    from ffcv_amd.transforms.auto_augment import augmix_table
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    width = args.width
    variants = ('fused', 'rounds', 'd2d')
    mode, fill = L.AFFINE_NEAREST, (0, 0, 0)
    for B, H, W in CASES:
        large = 9 * H * W > L.augmix_lds_bytes()
        assert not large or (3 * H * W >= L.randaugment_large_min_bytes() and L.augmix_large_fits(H, W))
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        rings = {name: [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
                 for name in ('src', 'dst')}
        for t in rings['src']:
            t.random_(0, 256, generator=gen)
        ids = ch.from_numpy(np.arange(B, dtype=np.uint64).view(np.int64)).to(dev)
        table = ch.from_numpy(augmix_table(H, W)).to(dev)
        d = {name: ch.empty(shape(B), dtype=getattr(ch, np.dtype(dt).name), device=dev)
             for name, dt, shape in L.augmix_arrays(width)}
        results = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(width)]
        spare = ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev)
        # the work buffers of the operation's device code, as it allocates them
        cj_ws = ch.empty(B, dtype=ch.int64, device=dev) if H * W * 3 > L.color_jitter_lds_bytes() else None
        tone_ws = ch.empty(768 * B, dtype=ch.int32, device=dev) if H * W * 3 > L.tone_lds_bytes() else None
        large_ws = ch.empty(L.augmix_large_workspace_bytes(H, W, width) if large else 0, dtype=ch.uint8, device=dev)

        def draw():
            L.augmix_draw_batch(ids, SEED, 0, SEVERITY, width, DEPTH, ALPHA, True, table, H, W, d)

        def run_rounds(x, dst):
            draw()
            for i in range(width):
                bufs = [spare, results[i], spare, results[i]]       # three rounds: the last lands in the result
                bufs[0].copy_(x)
                for r in range(3):
                    cur, nxt = bufs[r], bufs[r + 1]
                    a = L.randaugment_slot(d, 3 * i + r)
                    L.color_jitter_batch(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3], cj_ws)
                    L.color_jitter_batch(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
                    L.tone_batch_bits(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'], tone_ws)
                    L.affine_batch(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'])
                    L.sharpness_batch(cur, nxt, a['sharp_apply'], a['sharp_factor'])
            L.augmix_mix_batch(x, results, d['weights'], dst)

        def run(i, name):
            src, dst = rings['src'][i % nring], rings['dst'][i % nring]
            if name == 'd2d':
                dst.copy_(src)
            elif name == 'fused':
                draw()
                if large:
                    L.augmix_large_batch(src, dst, width, mode, fill, d, large_ws)
                else:
                    L.augmix_batch(src, dst, width, mode, fill, d)
            else:
                run_rounds(src, dst)
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'width': width, 'bytes': 2 * nbytes, 'ring': nring,
               'entry': 'ffcv_augmix_large_batch' if large else 'ffcv_augmix_batch',
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        run(0, 'fused')
        fused_out = rings['dst'][0].clone()
        run(0, 'rounds')
        res['fused_equals_rounds'] = bool(ch.equal(fused_out, rings['dst'][0]))
        assert res['fused_equals_rounds'], res
        res['changed'] = int((fused_out != rings['src'][0]).flatten(1).any(dim=1).sum())
        for name in variants:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
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
        res['rounds_over_fused'] = round(res['rounds']['median'] / res['fused']['median'], 2)
        res['fused_over_d2d'] = round(res['fused']['median'] / res['d2d']['median'], 2)
        res['rounds_over_d2d'] = round(res['rounds']['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del rings


if __name__ == '__main__':
    main()
