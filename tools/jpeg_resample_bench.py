"""The crop decoders' Pillow-exact modes (DESIGN s31): ffcv_jpeg_resample_batch
in both modes and its candidate plans beside the INTER_AREA launch
(ffcv_jpeg_rrc_batch, uint8, no epilogue) on the same batch and the same crops.

    python tools/jpeg_resample_bench.py [--reps 30] [--rounds 3] [--warmup 3] [--cases 512x256x224,128x512x224]

Per case (batch x long side of the JPEGs -> output side; q90 4:2:0 natural
images of ImageNet-like aspect, random-resized-crop windows at the default
scale and ratio), from HIP events around the whole launch and from the
context's per-kernel events (K1, K1b, the K2 slot):

  area          ffcv_jpeg_rrc_batch
  bilinear      ffcv_jpeg_resample_batch as the library plans it
  bicubic       ... (32 output rows a band; 16 window rows a chunk up to 128 rows, 8 above)
  bicubic2      the same code again: its distance from `bicubic` is the
                repeat-to-repeat spread a difference has to exceed
  b<R>c<C>      bicubic with R output rows a band and C window rows a chunk

The variants alternate inside each repetition after a warm-up of each.  Every
launch reads the next copy of the batch's bytes in a ring of copies that
holds more than twice the 256 MB of last-level cache (the streams repeat, their
addresses do not), so no launch finds its input in a cache.  The plan hook
(ffcv_jpeg_resample_batch_plan) is bound here, not in ffcv_amd.libffcv; the
candidates' outputs are checked to equal the default plan's first.  Per
variant: the median / min / max over --rounds of the per-round median
microseconds of the launch, and the median of the K2 slot.  One JSON line per case.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = '512x256x224,128x512x224'
PLANS = ((16, 8), (64, 8), (32, 4), (32, 8), (32, 16))     # (band_rows, chunk_rows)
LLC_BYTES = 256 << 20
DISTINCT = 64       # streams encoded per case; the batch repeats them


def bench_case(args, ch, L, dev, B, side, dst):
    from ffcv_amd.fields.decoders import RandomResizedCropRGBImageDecoder
    from ffcv_amd.synthetic import encode_jpeg, imagenet_like_shape, natural_image, pack
    rng = np.random.default_rng(0)
    shapes = [imagenet_like_shape(rng, side) for _ in range(DISTINCT)]
    blobs = [encode_jpeg(natural_image(rng, h, w), 90, '4:2:0') for h, w in shapes]
    pick = np.arange(B) % DISTINCT
    buf, offs, sizes = pack([blobs[i] for i in pick])
    nbytes = (len(buf) + 255) // 256 * 256
    nring = max(4, -(-2 * LLC_BYTES // nbytes) + 1)
    ring = ch.zeros((nring, nbytes), dtype=ch.uint8, device=dev)
    ring[:, :len(buf)] = ch.from_numpy(np.asarray(buf)).to(dev)
    smp = np.zeros((nring, B), L.SAMPLE_DTYPE)
    smp['size'], smp['height'], smp['width'] = sizes, [shapes[i][0] for i in pick], [shapes[i][1] for i in pick]
    smp['offset'] = np.asarray(offs, np.uint64)[None, :] + (np.arange(nring, dtype=np.uint64) * np.uint64(nbytes))[:, None]
    d_smp = ch.from_numpy(smp.view(np.uint8).reshape(nring, B * 32)).to(dev)
    crops = np.empty((B, 4), np.int32)
    L.draw_batch_host(np.arange(B, dtype=np.uint64) * 7, smp[0]['height'], smp[0]['width'],
                      RandomResizedCropRGBImageDecoder((dst, dst))._draw_params(1, 0, dst, dst), crops)
    d_crops = ch.from_numpy(crops).to(dev)
    out = ch.zeros((B, dst, dst, 3), dtype=ch.uint8, device=dev)
    status = ch.zeros(B, dtype=ch.int32, device=dev)
    dec = L.JpegDecoder(B, max(s[0] for s in shapes), max(s[1] for s in shapes), max(len(b) for b in blobs))
    p = L.RRCParams()
    p.out_h = p.out_w = dst
    plan_fn = L.lib().ffcv_jpeg_resample_batch_plan      # the measurement hook: not in ffcv_hip.h
    plan_fn.restype = ctypes.c_int
    plan_fn.argtypes = L._SIGS['ffcv_jpeg_resample_batch'][1] + [ctypes.c_int, ctypes.c_int]
    stream = ctypes.c_void_p(ch.cuda.current_stream().cuda_stream)
    launches = [0]

    def slot():           # the ring slot of this launch: every launch of every variant takes the next one
        launches[0] += 1
        return d_smp[launches[0] % nring]

    def resample(mode, band_rows=0, chunk_rows=0):
        L._check(plan_fn(dec.handle, stream, ring.data_ptr(), slot().data_ptr(), B, d_crops.data_ptr(),
                         L.RESAMPLE_MODES[mode], dst, dst, out.data_ptr(), 0, status.data_ptr(), band_rows, chunk_rows),
                 'ffcv_jpeg_resample_batch_plan')
    variants = {'area': lambda: dec.rrc(ring, slot(), B, d_crops, None, None, p, out, status),
                'bilinear': lambda: resample('bilinear'), 'bicubic': lambda: resample('bicubic'),
                'bicubic2': lambda: resample('bicubic')}
    resample('bicubic')
    want = out.clone()
    assert int(status.abs().sum()) == 0
    for r, c in PLANS:
        variants[f'b{r}c{c}'] = lambda r=r, c=c: resample('bicubic', r, c)
        try:
            resample('bicubic', r, c)
        except Exception:          # this chunk height does not fit the context's plan
            del variants[f'b{r}c{c}']
            continue
        assert ch.equal(out, want), (r, c)
    for fn in variants.values():
        for i in range(args.warmup):
            fn()
    ch.cuda.synchronize()
    names = list(variants)
    medians, k2 = {n: [] for n in names}, {n: [] for n in names}
    for _ in range(args.rounds):
        evs = {n: [] for n in names}
        dec.set_timing(args.reps * len(names))
        for i in range(args.reps):
            for n in names:
                a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                a.record()
                variants[n]()
                b.record()
                evs[n].append((a, b))
        ch.cuda.synchronize()
        ms = dec.timing_read().reshape(args.reps, len(names), 3)      # launches in issue order
        dec.set_timing(0)
        for j, n in enumerate(names):
            medians[n].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[n]])))
            k2[n].append(float(np.median(ms[:, j, 2]) * 1e3))
    res = {'case': f'{B} x {side}px q90 -> {dst}', 'unit': 'us', 'ring_copies': nring, 'batch_bytes': int(len(buf)),
           'config': f'{args.reps} launches x {args.rounds} rounds'}
    for n in names:
        m = medians[n]
        res[n] = {'launch': round(float(np.median(m)), 1), 'min': round(min(m), 1), 'max': round(max(m), 1),
                  'k2_slot': round(float(np.median(k2[n])), 1)}
    res['spread_us'] = round(max(abs(res['bicubic']['launch'] - res['bicubic2']['launch']),
                                 res['bicubic']['max'] - res['bicubic']['min']), 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cases', default=CASES)
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import libffcv as L
    assert ch.cuda.is_available(), 'needs the MI355X'
    for case in args.cases.split(','):
        B, side, dst = (int(x) for x in case.split('x'))
        bench_case(args, ch, L, 'cuda:0', B, side, dst)


if __name__ == '__main__':
    main()
