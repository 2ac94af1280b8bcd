"""RandomAdjustSharpness and TrivialAugmentWide (DESIGN s24): what
ffcv_sharpness_batch costs next to ffcv_gaussian_blur_batch at k = 3, the
nearest older stencil, and next to a device-to-device copy; and what the whole
TrivialAugmentWide sequence (its draw launch and its pixel launches) costs next
to that copy.

    python tools/sharpness_bench.py [--reps 60] [--rounds 3] [--warmup 10] [--ring-mb 640]

Shapes: 512 x 32 x 32 (the whole-image regime of both stencils) and 256 x 224 x
224 (bands of rows), every sample applied.

  sharpness  ffcv_sharpness_batch, every code 1, factor 2
  blur3      ffcv_gaussian_blur_batch, k = 3, sigma 1, every flag 1
  d2d        one device-to-device copy of the same bytes
  taw        ffcv_policy_draw_batch, two ffcv_color_jitter_batch, ffcv_tone_batch_bits,
             ffcv_affine_batch (nearest) and ffcv_sharpness_batch, as the operation runs them

From HIP events around each variant, in one process.  The variants alternate
inside each repetition after a warm-up of each; every launch takes the next
batch of rings of --ring-mb each (more than the 256 MB Infinity Cache), so no
launch finds its input in a cache.  The policy's colour and tone launches work
in place, so its ring is refilled before every round.  Per variant: the median
/ min / max over --rounds of the per-round median microseconds.  The outputs
are checked against the host twins on a few images first.  Prints one JSON line
per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((512, 32, 32), (256, 224, 224))
CJ_STEPS, SOLARIZE_STEPS, TONE_STEPS = (1, 3, 2), (5,), (1, 2, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--ring-mb', type=int, default=640)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    from ffcv_amd.transforms.auto_augment import value_table
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    variants = ('sharpness', 'blur3', 'd2d', 'taw')
    table_np = value_table(31)
    table = ch.from_numpy(table_np).to(dev)
    for B, H, W in CASES:
        nbytes = B * H * W * 3
        nring = max(2, -(-args.ring_mb * (1 << 20) // nbytes))
        rings = {name: [ch.empty((B, H, W, 3), dtype=ch.uint8, device=dev) for _ in range(nring)]
                 for name in ('src', 'taw', 'dst')}

        def refill(names):
            for name in names:
                for t in rings[name]:
                    t.random_(0, 256, generator=gen)
        refill(('src', 'taw'))
        ids_np = np.arange(B, dtype=np.uint64)
        ids = ch.from_numpy(ids_np.view(np.int64)).to(dev)
        ones = ch.ones((B,), dtype=ch.uint8, device=dev)
        factor = ch.full((B,), 2.0, dtype=ch.float32, device=dev)
        sigma = ch.empty((B,), dtype=ch.float64, device=dev)
        weights = ch.empty((B, L.BLUR_WROW), dtype=ch.float32, device=dev)
        flags = ch.empty((B,), dtype=ch.uint8, device=dev)
        L.blur_draw_batch(ids, 0, 0, 1.0, 1.0, 1.0, 3, flags, sigma, weights)
        pol = {name: ch.empty(shape(B), dtype=getattr(ch, np.dtype(dt).name), device=dev)
               for name, dt, shape in L.POLICY_ARRAYS}
        cws = ch.empty((B,), dtype=ch.int64, device=dev) if H * W * 3 > L.color_jitter_lds_bytes() else None
        tws = ch.empty((768 * B,), dtype=ch.int32, device=dev) if H * W * 3 > L.tone_lds_bytes() else None

        def run(i, name):
            src, dst = rings['src'][i % nring], rings['dst'][i % nring]
            if name == 'd2d':
                dst.copy_(src)
            elif name == 'sharpness':
                L.sharpness_batch(src, dst, ones, factor)
            elif name == 'blur3':
                L.gaussian_blur_batch(src, dst, 3, flags, weights)
            else:
                x = rings['taw'][i % nring]
                L.policy_draw_batch(ids, 3, 0, 31, table, H, W, pol)
                L.color_jitter_batch(x, CJ_STEPS, pol['cj_apply'][:3], pol['cj_ratio'][:3], cws)
                L.color_jitter_batch(x, SOLARIZE_STEPS, pol['cj_apply'][3:], pol['cj_ratio'][3:])
                L.tone_batch_bits(x, TONE_STEPS, pol['tone_apply'], pol['tone_bits'], tws)
                L.affine_batch(x, dst, L.AFFINE_NEAREST, (0, 0, 0), pol['aff_apply'], pol['aff_coef'])
                L.sharpness_batch(x, dst, pol['sharp_apply'], pol['sharp_factor'])
        res = {'unit': 'us', 'batch': B, 'shape': f'{H}x{W}', 'bytes': 2 * nbytes, 'ring': nring,
               'whole_image': H * W * 6 <= L.sharpness_lds_bytes(),
               'config': f'{args.reps} launches x {args.rounds} rounds'}
        # the launches compute what the host twins compute
        n = 16
        ok = True
        before = rings['src'][0][:n].cpu().numpy()
        run(0, 'sharpness')
        want = np.empty_like(before)
        L.sharpness_batch_host(before, want, np.ones(n, np.uint8), np.full(n, 2, np.float32))
        ok &= bool(np.array_equal(rings['dst'][0][:n].cpu().numpy(), want))
        run(0, 'blur3')
        L.gaussian_blur_batch_host(before, want, 3, np.ones(n, np.uint8), weights[:n].cpu().numpy())
        ok &= bool(np.array_equal(rings['dst'][0][:n].cpu().numpy(), want))
        x = rings['taw'][0][:n].cpu().numpy()
        run(0, 'taw')
        d = L.policy_draw_batch_host(ids_np, 3, 0, 31, table_np, H, W)
        L.color_jitter_batch_host(x, CJ_STEPS, d['cj_apply'][:3, :n], d['cj_ratio'][:3, :n])
        L.color_jitter_batch_host(x, SOLARIZE_STEPS, d['cj_apply'][3:, :n], d['cj_ratio'][3:, :n])
        L.tone_batch_bits_host(x, TONE_STEPS, d['tone_apply'][:, :n], d['tone_bits'][:n])
        L.affine_batch_host(x, want, L.AFFINE_NEAREST, (0, 0, 0), d['aff_apply'][:n], d['aff_coef'][:n])
        L.sharpness_batch_host(x, want, d['sharp_apply'][:n], d['sharp_factor'][:n])
        ok &= bool(np.array_equal(rings['dst'][0][:n].cpu().numpy(), want))
        res['equal_host_twins'] = ok
        res['taw_ops'] = np.bincount(d['op'], minlength=L.POLICY_NOPS).tolist()
        for name in variants:
            for i in range(args.warmup):
                run(i, name)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            refill(('taw',))
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
        res['sharpness_over_blur3'] = round(res['sharpness']['median'] / res['blur3']['median'], 2)
        res['sharpness_over_d2d'] = round(res['sharpness']['median'] / res['d2d']['median'], 2)
        res['taw_over_d2d'] = round(res['taw']['median'] / res['d2d']['median'], 2)
        print(json.dumps(res), flush=True)
        del rings


if __name__ == '__main__':
    main()
