"""The Pillow-exact resampler (DESIGN s30): ffcv_resample_images_batch in both
modes, its candidate plans, and beside it a device copy and the INTER_AREA
launch a user would compare with.

    python tools/resample_bench.py [--reps 60] [--rounds 3] [--warmup 5] [--cases 512x32x32,...]

Per case (batch x source side -> output side; the defaults are those of the
DESIGN table) and per mode, from HIP events through the C ABI, crops drawn on
the device at the default scale (0.08, 1) and ratio (3/4, 4/3):

  resample      the launch as the library plans it (32 output rows a band; 16
                source rows a chunk for sources of up to 128 rows, 8 above)
  resample2     the same code again: its distance from `resample` is the
                repeat-to-repeat spread a difference has to exceed
  b<R>c<C>      the candidate plans: R output rows a band, C source rows a chunk
  area          ffcv_rrc_images_batch (INTER_AREA) on the same windows
  copy          a device copy of the input batch (its bytes in and out again)

The variants alternate inside each repetition after a warm-up of each.  Every
launch of every variant reads the next batch of a ring (a running launch
counter picks the slot) that holds more than twice the 256 MB of last-level
cache, so a batch is read again only after more than 512 MB of other batches
and no launch finds its input in a cache.  The plan hook
(ffcv_resample_images_batch_plan) is bound here, not in ffcv_amd.libffcv.
Per variant: the median / min / max over --rounds of the per-round median
microseconds.  The candidates' outputs are checked to equal the default
plan's first.  Prints one JSON line per case and mode.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = '512x32x32,512x64x32,256x128x112,256x224x224,256x256x224'
PLANS = ((16, 8), (64, 8), (32, 4), (32, 8), (32, 16))     # (band_rows, chunk_rows)
LLC_BYTES = 256 << 20


def bench_case(args, ch, L, dev, B, src, dst):
    img = src * src * 3
    nring = max(4, -(-2 * LLC_BYTES // (B * img)) + 1)
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    ring = ch.randint(0, 256, (nring, B, src, src, 3), dtype=ch.uint8, device=dev, generator=gen)
    spare = ch.empty_like(ring[0])
    crops = ch.empty((B, 4), dtype=ch.int32, device=dev)
    L.crop_draw_batch(ch.arange(B, dtype=ch.int64, device=dev) * 7, src, src, (0.08, 1.0), (0.75, 4 / 3), 1, 0, crops)
    hw = crops.cpu().numpy()[:, 2:].astype(np.int64)
    out = ch.zeros((B, dst, dst, 3), dtype=ch.uint8, device=dev)
    p = L.RRCParams()
    p.out_h = p.out_w = dst
    nws = L.rrc_images_workspace_bytes(B, src, src, dst, dst)
    ws = ch.empty(nws, dtype=ch.uint8, device=dev) if nws else None
    plan_fn = L.lib().ffcv_resample_images_batch_plan      # the measurement hook: not in ffcv_hip.h
    plan_fn.restype = ctypes.c_int
    plan_fn.argtypes = L._SIGS['ffcv_resample_images_batch'][1] + [ctypes.c_int, ctypes.c_int]
    stream = ctypes.c_void_p(ch.cuda.current_stream().cuda_stream)
    launches = [0]

    def batch():          # the ring slot of this launch: every launch of every variant takes the next one
        launches[0] += 1
        return ring[launches[0] % nring]
    for mode in ('bilinear', 'bicubic'):
        def resample(band_rows=0, chunk_rows=0):
            L._check(plan_fn(batch().data_ptr(), img, B, src, src, crops.data_ptr(), L.RESAMPLE_MODES[mode], dst, dst,
                             out.data_ptr(), 0, None, stream, band_rows, chunk_rows), 'ffcv_resample_images_batch_plan')
        variants = {'resample': resample, 'resample2': resample,
                    'area': lambda: L.rrc_images_batch(batch(), img, B, src, src, crops, None, None, p, out, None, ws),
                    'copy': lambda: spare.copy_(batch())}
        launches[0] = 0
        resample()
        want = out.clone()
        for r, c in PLANS:
            variants[f'b{r}c{c}'] = lambda r=r, c=c: resample(r, c)
            launches[0] = 0
            resample(r, c)
            assert ch.equal(out, want), (mode, r, c)
        for fn in variants.values():
            for i in range(args.warmup):
                fn()
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            evs = {name: [] for name in variants}
            for i in range(args.reps):
                for name, fn in variants.items():
                    a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    evs[name].append((a, b))
            ch.cuda.synchronize()
            for name in variants:
                medians[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[name]])))
        res = {'case': f'{B} x {src}->{dst}', 'mode': mode, 'unit': 'us', 'ring_batches': nring,
               'config': f'{args.reps} launches x {args.rounds} rounds',
               'window_bytes': int((hw[:, 0] * hw[:, 1] * 3).sum()), 'out_bytes': B * dst * dst * 3,
               'copy_bytes_each_way': B * img}
        for name, m in medians.items():
            res[name] = {'median': round(float(np.median(m)), 2), 'min': round(min(m), 2), 'max': round(max(m), 2)}
        res['spread_us'] = round(max(abs(res['resample']['median'] - res['resample2']['median']),
                                     res['resample']['max'] - res['resample']['min']), 2)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cases', default=CASES)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    for case in args.cases.split(','):
        B, src, dst = (int(x) for x in case.split('x'))
        bench_case(args, ch, L, 'cuda:0', B, src, dst)


if __name__ == '__main__':
    main()
