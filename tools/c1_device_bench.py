"""Small-image device path (DESIGN s13): a CIFAR-shaped synthetic .beton
(50,000 raw 32x32 RGBImageField + IntField samples, batch 512, SEQUENTIAL,
drop_last) on a device Loader running the reference's CIFAR chain

    SimpleRGBImageDecoder -> RandomHorizontalFlip -> RandomTranslate(2, mean)
      -> Cutout(4, mean) -> ToTensor -> ToDevice -> ToTorchImage
      -> NormalizeImage(mean, std, float16)

Prints one JSON line:
  value / images_per_s   Loader rate (median epoch of --epochs timed epochs
                         after --warmup; each epoch ends in a device sync)
  launch_us              HIP-event time per batch of the draws + the fused
                         kernel (ffcv_draw_batch, ffcv_translate_draw_batch,
                         ffcv_simple_aug_batch) over --batches batches, at batch
                         512 and at the Loader's launch size
  fused_kernel_us, hbm_fraction
                         the fused kernel alone, and its algorithmic bytes
                         (3,072 read + 6,144 written per image) per second
                         over the 8.0 TB/s HBM peak

--no-translate drops RandomTranslate from the chain: the staged path (gather +
flip + cutout + LUT kernels), which is also all a tree without RandomTranslate
can run; launch_us is then the event time of that path's six launches
(gather, draw + flip, draw + cutout, LUT) and the fused-kernel fields are null.

    python tools/c1_device_bench.py [--no-translate] [--n 50000] [--epochs 100]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
FILL = tuple(int(v) for v in MEAN)
HBM_PEAK = 8.0e12  # bytes/s (spec)
BYTES_PER_IMAGE = 32 * 32 * 3 * (1 + 2)  # read u8 once, write fp16 once


def event_times(ch, fn, n, warmup=20):
    """Mean microseconds of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    ch.cuda.synchronize()
    evs = [(ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    ch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in evs]) * 1e3
    return float(t.mean()), float(np.median(t)), float(t.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--batch-size', type=int, default=512)
    ap.add_argument('--epochs', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batches', type=int, default=200, help='batches timed with events')
    ap.add_argument('--no-translate', action='store_true')
    args = ap.parse_args()
    import torch as ch
    assert ch.cuda.is_available(), 'c1_device_bench needs the GPU (no CPU fallback)'
    from ffcv_amd.writer import DatasetWriter
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
    from ffcv_amd.loader import Loader, OrderOption
    from ffcv_amd import transforms as T

    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, (args.n, 32, 32, 3), dtype=np.uint8)

    class DS:
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            return imgs[i], i % 10

    fn = os.path.join(tempfile.mkdtemp(), 'c1_device.beton')
    DatasetWriter(fn, {'image': RGBImageField(write_mode='raw'), 'label': IntField()},
                  num_workers=min(8, len(os.sched_getaffinity(0)))).from_indexed_dataset(DS())
    dev = ch.device('cuda:0')
    chain = [SimpleRGBImageDecoder(), T.RandomHorizontalFlip(0.5)]
    if not args.no_translate:
        chain.append(T.RandomTranslate(2, FILL))
    chain += [T.Cutout(4, FILL), T.ToTensor(), T.ToDevice(dev, non_blocking=True), T.ToTorchImage(),
              T.NormalizeImage(MEAN, STD, np.float16)]
    loader = Loader(fn, batch_size=args.batch_size, order=OrderOption.SEQUENTIAL, drop_last=True, seed=0,
                    pipelines={'image': chain, 'label': [IntDecoder(), T.ToTensor(), T.ToDevice(dev)]})
    dec = loader.pipeline_specs['image'].decoder
    times = []
    n = 0
    for e in range(args.warmup + args.epochs):
        ch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for images, labels in loader:
            n += images.shape[0]
        ch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert images.dtype == ch.float16 and tuple(images.shape[1:]) == (3, 32, 32)
    timed = np.array(times[args.warmup:])
    rate = n / float(np.median(timed))
    res = {'config': f'C1 device: {args.n} raw 32x32 + int, batch {args.batch_size}, SEQUENTIAL, drop_last, '
                     f'flip -> {"" if args.no_translate else "translate(2) -> "}cutout(4) -> fp16 normalize',
           'value': round(rate, 1), 'unit': 'images/s', 'images_per_s': round(rate, 1),
           'images_per_s_best': round(n / float(timed.min()), 1),
           'images_per_s_worst': round(n / float(timed.max()), 1),
           'epochs_timed': int(timed.size), 'samples_per_epoch': n,
           'fused': bool(getattr(dec, 'fused', False)), 'translate': not args.no_translate,
           'launch_us': None, 'fused_kernel_us': None, 'hbm_fraction': None}
    if args.no_translate:
        # the staged path's launches of one batch through the C ABI (what the
        # operations enqueue: gather, draw + flip, draw + cutout, LUT)
        from ffcv_amd import libffcv as L
        from ffcv_amd.loader.epoch_iterator import launch_group
        dd = loader.device_dataset
        table, data = dd.table(0).view(-1, 32), dd.data
        lut = chain[-1].device_lut(dev)
        dpf, dpc = L.DrawParams(), L.DrawParams()
        dpf.flip_prob = 0.5
        dpc.out_h = dpc.out_w = 32
        dpc.cutout_size = 4
        group = launch_group(loader, args.n // args.batch_size)
        res.update(launch_us={}, batches_per_launch=group)
        for B in (args.batch_size, min(args.n, group * args.batch_size)):
            wins = []
            for w in range(max(1, args.n // B)):
                ids = (ch.arange(B, dtype=ch.int64, device=dev) + w * B) % args.n
                smp = ch.empty((B, 32), dtype=ch.uint8, device=dev)
                L.gather_samples(table, ids, smp)
                wins.append((ids, smp))
            cyx = ch.empty((B, 2), dtype=ch.int32, device=dev)
            flips = ch.empty(B, dtype=ch.uint8, device=dev)
            raw = ch.empty((B, 32, 32, 3), dtype=ch.uint8, device=dev)
            flipped = ch.empty_like(raw)
            out = ch.empty((B, 32, 32, 3), dtype=ch.int16, device=dev)
            turn = [0]

            def staged():
                ids, smp = wins[turn[0] % len(wins)]
                turn[0] += 1
                L.gather_raw_batch(data, smp, B, raw, 3072)
                L.draw_batch(ids, None, dpf, None, None, flips, None)
                L.flip_batch(raw, flipped, flips)
                L.draw_batch(ids, None, dpc, None, cyx, None, None)
                L.cutout_batch(flipped, cyx, 4, FILL)
                L.lut_batch(flipped, lut, out)
            t = event_times(ch, staged, args.batches)
            res['launch_us'][str(B)] = {'mean': round(t[0], 2), 'median': round(t[1], 2), 'min': round(t[2], 2)}
    else:
        # the launches of one batch through the C ABI, on the Loader's own
        # HBM-resident dataset (150 MB: it stays in the 256 MB Infinity Cache,
        # as it does in training), windows rotating over the dataset
        from ffcv_amd import libffcv as L
        from ffcv_amd.loader.epoch_iterator import launch_group
        assert dec.fused, 'the chain was not lowered into the fused launch'
        dd = loader.device_dataset
        table, data = dd.table(0).view(-1, 32), dd.data
        lut = chain[-1].device_lut(dev)
        sp = L.SimpleAugParams()
        sp.n_steps = 3
        sp.steps[0], sp.steps[1], sp.steps[2] = L.AUG_FLIP, L.AUG_TRANSLATE, L.AUG_CUTOUT
        sp.padding, sp.cutout_size = 2, 4
        for c in range(3):
            sp.translate_fill[c] = sp.cutout_fill[c] = FILL[c]
        dp = L.DrawParams()
        dp.out_h = dp.out_w = 32
        dp.cutout_size, dp.flip_prob = 4, 0.5
        group = launch_group(loader, args.n // args.batch_size)
        res.update(launch_us={}, fused_kernel_us={}, hbm_fraction={}, batches_per_launch=group)
        for B in (args.batch_size, min(args.n, group * args.batch_size)):
            wins = []
            for w in range(max(1, args.n // B)):
                ids = (ch.arange(B, dtype=ch.int64, device=dev) + w * B) % args.n
                smp = ch.empty((B, 32), dtype=ch.uint8, device=dev)
                L.gather_samples(table, ids, smp)
                wins.append((ids, smp))
            tyx = ch.empty((B, 2), dtype=ch.int32, device=dev)
            cyx = ch.empty((B, 2), dtype=ch.int32, device=dev)
            flips = ch.empty(B, dtype=ch.uint8, device=dev)
            out = ch.empty((B, 32, 32, 3), dtype=ch.float16, device=dev)
            turn = [0]

            def kernel():
                ids, smp = wins[turn[0] % len(wins)]
                turn[0] += 1
                L.simple_aug_batch(data, smp, B, 32, 32, sp, flips, cyx, tyx, lut, out, 0)

            def draws_and_kernel():
                ids, smp = wins[turn[0] % len(wins)]
                L.draw_batch(ids, None, dp, None, cyx, flips, None)
                L.translate_draw_batch(ids, 0, 0, 2, tyx)
                kernel()
            both = event_times(ch, draws_and_kernel, args.batches)
            alone = event_times(ch, kernel, args.batches)
            res['launch_us'][str(B)] = {'mean': round(both[0], 2), 'median': round(both[1], 2),
                                        'min': round(both[2], 2)}
            res['fused_kernel_us'][str(B)] = {'mean': round(alone[0], 2), 'median': round(alone[1], 2),
                                              'min': round(alone[2], 2)}
            res['hbm_fraction'][str(B)] = round(B * BYTES_PER_IMAGE / (alone[1] * 1e-6) / HBM_PEAK, 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
