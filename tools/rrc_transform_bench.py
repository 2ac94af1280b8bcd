"""RandomResizedCrop transform (DESIGN s18): the one-workgroup-per-image LDS
kernel against the raw decoder's band kernel on the same dense input, and
what the transform costs a Loader.

    python tools/rrc_transform_bench.py [--reps 200] [--rounds 3] [--batch 512] [--n 20480] [--epochs 3]
                                        [--skip-loader]

Part 1, ffcv_rrc_images_batch alone, from HIP events through the C ABI, on a
batch of --batch random images, crops drawn on the device at the default
scale (0.08, 1) and ratio (3/4, 4/3):

    source -> output   32 -> 32, 64 -> 32, 64 -> 64, 96 -> 64, 128 -> 112, u8 and fp16

  lds    the LDS regime: one launch, a workgroup per image
  band   the band regime on the same input: the descriptor kernel, the taps
         kernel and the raw decoder's band kernel (ffcv_rrc_raw_batch_ws)
  lds2, band2   the same code again: their distance from lds / band is the
         repeat-to-repeat spread a difference has to exceed

The outputs of the two regimes are checked to be identical first.  The four
variants alternate inside each repetition after a warm-up of each, through a
ring of four input batches; per variant: the median / min / max over --rounds
of the per-round median microseconds, and the achieved bytes/s (crop bytes
read + output bytes written) against the 8 TB/s HBM peak.  At these sizes the
launch is overhead-bound: a batch moves a few MB.

Part 2, one Loader epoch of --n raw 32 x 32 samples, batch 512, device cache:

    base  SimpleRGBImageDecoder + RandomHorizontalFlip + Cutout(8) + ToTensor + ToDevice + ToTorchImage +
          NormalizeImage fp16 | IntDecoder + ToTensor + ToDevice
    rrc   the same with RandomResizedCrop(size 32) behind the decoder (flip, cutout and the table are
          lowered into its launch)

each at batches_per_launch=1 and at the default grouping, the four Loaders
alternating epoch by epoch after a warm-up epoch of each.  Prints one JSON
line per case.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((32, 32), (64, 32), (64, 64), (96, 64), (128, 112))
HBM_PEAK = 8.0e12
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])


def kernel_part(args, ch, L, dev):
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    B = args.batch
    lut = ch.from_numpy(((np.arange(256)[:, None] - MEAN[None, :]) / STD[None, :]).astype(np.float16)
                        .view(np.int16)).to(dev)
    ids = ch.arange(B, dtype=ch.int64, device=dev) * 7
    for src, dst in CASES:
        ring = [ch.randint(0, 256, (B, src, src, 3), dtype=ch.uint8, device=dev, generator=gen) for _ in range(4)]
        crops = ch.empty((B, 4), dtype=ch.int32, device=dev)
        L.crop_draw_batch(ids, src, src, (0.08, 1.0), (0.75, 4 / 3), 1, 0, crops)
        hw = crops.cpu().numpy()[:, 2:].astype(np.int64)
        ws = ch.empty(L.rrc_images_band_workspace_bytes(B, dst, dst), dtype=ch.uint8, device=dev)
        for fp16 in (False, True):
            p = L.RRCParams()
            p.out_h = p.out_w = dst
            if fp16:
                p.lut = lut.data_ptr()
            es = 2 if fp16 else 1
            outs = {r: ch.zeros((B, dst, dst, 3 * es), dtype=ch.uint8, device=dev) for r in (1, 2)}

            def run(i, regime):
                L.rrc_images_batch(ring[i % 4], src * src * 3, B, src, src, crops, None, None, p, outs[regime], None,
                                   ws if regime == 2 else None, regime=regime)
            res = {'part': 'kernel', 'unit': 'us', 'case': f'{src}->{dst}', 'dtype': 'fp16' if fp16 else 'u8',
                   'batch': B, 'config': f'{args.reps} launches x {args.rounds} rounds',
                   'auto_regime': 'lds' if L.rrc_images_workspace_bytes(B, src, src, dst, dst) == 0 else 'band'}
            try:
                run(0, 1)
            except L.FFCVError as e:   # the source and the taps do not fit one workgroup's LDS
                res['lds'] = None
                res['note'] = str(e)
                print(json.dumps(res), flush=True)
                continue
            run(0, 2)
            ch.cuda.synchronize()
            res['identical'] = bool(ch.equal(outs[1], outs[2]))
            variants = {'lds': 1, 'band': 2, 'lds2': 1, 'band2': 2}
            for regime in variants.values():
                for i in range(args.warmup):
                    run(i, regime)
            ch.cuda.synchronize()
            medians = {name: [] for name in variants}
            for _ in range(args.rounds):
                evs = {name: [] for name in variants}
                for i in range(args.reps):
                    for name, regime in variants.items():
                        a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                        a.record()
                        run(i, regime)
                        b.record()
                        evs[name].append((a, b))
                ch.cuda.synchronize()
                for name in variants:
                    medians[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in evs[name]])))
            nbytes = int((hw[:, 0] * hw[:, 1] * 3).sum()) + B * dst * dst * 3 * es
            for name in variants:
                m = medians[name]
                med = float(np.median(m))
                res[name] = {'median': round(med, 2), 'min': round(min(m), 2), 'max': round(max(m), 2),
                             'GB/s': round(nbytes / med / 1e3, 1), 'of_hbm_peak': round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
            spread = max(abs(res['lds']['median'] - res['lds2']['median']),
                         abs(res['band']['median'] - res['band2']['median']),
                         res['lds']['max'] - res['lds']['min'], res['band']['max'] - res['band']['min'])
            res['spread_us'] = round(spread, 2)
            res['band_minus_lds_us'] = round(res['band']['median'] - res['lds']['median'], 2)
            res['lds_faster_beyond_spread'] = bool(res['band_minus_lds_us'] > spread)
            res['bytes'] = nbytes
            print(json.dumps(res), flush=True)


def loader_part(args, ch, dev):
    from ffcv_amd.loader import Loader
    from ffcv_amd.writer import DatasetWriter
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
    from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomHorizontalFlip,
                                     RandomResizedCrop)
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, (args.n, 32, 32, 3), dtype=np.uint8)

    class DS:
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            return imgs[i], i % 10
    fn = os.path.join(tempfile.mkdtemp(), 'cifar_shape.beton')
    DatasetWriter(fn, {'image': RGBImageField(write_mode='raw'), 'label': IntField()},
                  num_workers=1).from_indexed_dataset(DS(), chunksize=1000)

    def mk(rrc, **kw):
        ops = [SimpleRGBImageDecoder()] + ([RandomResizedCrop((0.08, 1.0), (0.75, 4 / 3), 32)] if rrc else []) + \
              [RandomHorizontalFlip(0.5), Cutout(8, (125, 123, 114)), ToTensor(), ToDevice(dev), ToTorchImage(),
               NormalizeImage(MEAN, STD, np.float16)]
        return Loader(fn, batch_size=512, seed=1, drop_last=False, pipelines={
            'image': ops, 'label': [IntDecoder(), ToTensor(), ToDevice(dev)]}, **kw)
    loaders = {'base b1': mk(False, batches_per_launch=1), 'rrc b1': mk(True, batches_per_launch=1),
               'base grouped': mk(False), 'rrc grouped': mk(True)}

    def epoch(loader):
        t0 = time.perf_counter()
        n = 0
        for images, labels in loader:
            n += int(labels.shape[0])
        ch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    for loader in loaders.values():
        epoch(loader)
    rates = {name: [] for name in loaders}
    for _ in range(args.epochs):
        for name, loader in loaders.items():
            rates[name].append(epoch(loader))
    res = {'part': 'loader', 'unit': 'samples/s', 'n': args.n, 'batch': 512,
           'config': f'{args.epochs} epochs alternating after a warm-up epoch each'}
    for name, r in rates.items():
        res[name] = {'median': round(float(np.median(r))), 'min': round(min(r)), 'max': round(max(r))}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--n', type=int, default=20480)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--skip-loader', action='store_true')
    args = ap.parse_args()
    import torch as ch
    from ffcv_amd import _build, libffcv as L
    _build.build()
    assert ch.cuda.is_available(), 'needs the MI355X'
    dev = 'cuda:0'
    kernel_part(args, ch, L, dev)
    if not args.skip_loader:
        loader_part(args, ch, dev)


if __name__ == '__main__':
    main()
