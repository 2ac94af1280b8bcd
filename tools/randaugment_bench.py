"""RandAugment (DESIGN s27): what the fused path (the draw launch and ONE pixel
launch that keeps each image in LDS across its slots) costs next to the rounds
path (the draw launch and, slot after slot, the five pixel launches of
TrivialAugmentWide on the slot's slices of the same arrays) and next to a
device-to-device copy.

    python tools/randaugment_bench.py [--reps 60] [--rounds 3] [--warmup 10] [--ring-mb 640] [--num-ops 2]

Shapes: 512 x 32 x 32 and 256 x 64 x 64 (the edge of the fused regime),
uniformly random pixels, num_ops = 2, magnitude 9 of 31 bins, nearest.

  fused   ffcv_randaugment_draw_batch, ffcv_randaugment_batch
  rounds  ffcv_randaugment_draw_batch, then per slot two ffcv_color_jitter_batch,
          ffcv_tone_batch_bits, ffcv_affine_batch and ffcv_sharpness_batch, as the
          operation runs them beyond the fused regime (the baseline: existing kernels)
  d2d     one device-to-device copy of the same bytes

From HIP events around each variant, in one process.  The variants alternate
inside each repetition after a warm-up of each; every launch takes the next
batch of rings of --ring-mb each (more than the 256 MB Infinity Cache), so no
launch finds its input in a cache.  The rounds work in place on their input, so
their ring is refilled before every round.  Per variant: the median / min / max
over --rounds of the per-round median microseconds.  First the two paths'
outputs are checked equal on the whole batch, and against the host twins on a
few images.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 64, 64))
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)
NBINS, MAGNITUDE, SEED = 31, 9, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--ring-mb', type=int, default=640)
    ap.add_argument('--num-ops', type=int, default=2)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    from ffcv_amd.transforms.auto_augment import randaugment_table
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    S = args.num_ops
    variants = ('fused', 'rounds', 'd2d')
    mode, fill = L.AFFINE_NEAREST, (0, 0, 0)
    for B, H, W in CASES:
        assert 6 * H * W <= L.randaugment_lds_bytes()
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        rings = {name: [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
                 for name in ('src', 'rounds', 'dst')}

        def refill(names):
            for name in names:
                for t in rings[name]:
                    t.random_(0, 256, generator=gen)
        refill(('src', 'rounds'))
        ids_np = np.arange(B, dtype=np.uint64)
        ids = ch.from_numpy(ids_np.view(np.int64)).to(dev)
        table_np = randaugment_table(NBINS, H, W)
        table = ch.from_numpy(table_np).to(dev)
        d = {name: ch.empty(shape(B), dtype=getattr(ch, np.dtype(dt).name), device=dev)
             for name, dt, shape in L.randaugment_arrays(S)}
        spare = [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(min(2, S - 1))]

        def run_rounds(x, dst):
            L.randaugment_draw_batch(ids, SEED, 0, S, NBINS, MAGNITUDE, table, H, W, d)
            cur = x
            for s in range(S):
                nxt = dst if s == S - 1 else spare[s % 2]
                a = L.randaugment_slot(d, s)
                L.color_jitter_batch(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
                L.color_jitter_batch(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
                L.tone_batch_bits(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'])
                L.affine_batch(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'])
                L.sharpness_batch(cur, nxt, a['sharp_apply'], a['sharp_factor'])
                cur = nxt

        def run(i, name):
            src, dst = rings['src'][i % nring], rings['dst'][i % nring]
            if name == 'd2d':
                dst.copy_(src)
            elif name == 'fused':
                L.randaugment_draw_batch(ids, SEED, 0, S, NBINS, MAGNITUDE, table, H, W, d)
                L.randaugment_batch(src, dst, S, mode, fill, d)
            else:
                run_rounds(rings['rounds'][i % nring], dst)
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'num_ops': S, 'bytes': 2 * nbytes, 'ring': nring,
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        # both paths compute the same bytes, which are the host twins'
        before = rings['src'][0].clone()
        run(0, 'fused')
        fused_out = rings['dst'][0].clone()
        run_rounds(before.clone(), rings['dst'][0])
        res['fused_equals_rounds'] = bool(ch.equal(fused_out, rings['dst'][0]))
        n = 16
        hd = L.randaugment_draw_batch_host(ids_np[:n], SEED, 0, S, NBINS, MAGNITUDE, table_np, H, W)
        cur = before[:n].cpu().numpy()
        for s in range(S):
            a = L.randaugment_slot(hd, s)
            nxt = np.empty_like(cur)
            L.color_jitter_batch_host(cur, CJ_STEPS, a['cj_apply'][:3], a['cj_ratio'][:3])
            L.color_jitter_batch_host(cur, SOLARIZE_STEPS, a['cj_apply'][3:], a['cj_ratio'][3:])
            L.tone_batch_bits_host(cur, TONE_STEPS, a['tone_apply'], a['tone_bits'])
            L.affine_batch_host(cur, nxt, mode, fill, a['aff_apply'], a['aff_coef'])
            L.sharpness_batch_host(cur, nxt, a['sharp_apply'], a['sharp_factor'])
            cur = nxt
        res['equal_host_twins'] = bool(np.array_equal(fused_out[:n].cpu().numpy(), cur))
        res['ops'] = np.bincount(d['op'].cpu().numpy().ravel(), minlength=L.POLICY_NOPS).tolist()
        for name in variants:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            refill(('rounds',))
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
