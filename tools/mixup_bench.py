"""Device mixup (DESIGN s15): what ffcv_mixup_batch costs next to a copy of
the same bytes, and what the mixup operations cost a Loader.

    python tools/mixup_bench.py [--reps 20] [--rounds 3] [--n 24576] [--epochs 3] [--skip-loader]

Part 1, the kernel alone, from HIP events through the C ABI, uint8, one
lambda per sample, batches of 512:

    512 x 32x32x3      1.5 MB: a launch-latency case
    512 x 224x224x3    77 MB: one ImageNet batch
    12288 x 224x224x3  1.85 GB: one launch group of 24 batches

  run8 / run4 / run2   the kernel walking runs of 8, 4 (the shipped form), 2
                       samples with the previous sample's bytes in registers
  run1                 the plain form: every sample and its neighbour are read
  copy                 torch's device copy_ of the same bytes

Every variant works through a ring of buffer pairs larger than the 256 MiB
Infinity Cache; the variants of a shape alternate inside each repetition,
after a warm-up of every variant; the measurement is repeated --rounds times
to show the spread.  Per variant: the median / min / max over rounds of the
per-round median microseconds, GB/s of algorithmic traffic (one read and one
write of the batch) at the median, and that as a fraction of the copy's.

Part 2, one Loader epoch of --n synthetic ImageNet-shape JPEGs (the bench
generator's), batch 512, device cache, entropy index warm:

    base   RRC(224) + Cutout(32) + ToTensor + ToDevice + ToTorchImage +
           NormalizeImage fp16 | IntDecoder + ToTensor + ToDevice
           (lowers to the one fused decode launch)
    mixup  the same with ImageMixup(0.5, False) after Cutout, and LabelMixup +
           MixupToOneHot(1000) on the labels (the decode launch writes uint8,
           then ffcv_mixup_batch, then the NormalizeImage table pass)

each at batches_per_launch=1 and at the default grouping, the four Loaders
alternating epoch by epoch after a warm-up epoch of each.  Prints one JSON
line per part.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING_BYTES = 600 << 20
SHAPES = ((512, 32), (512, 224), (12288, 224))
BATCH = 512


def kernel_part(args, ch, L, dev):
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    res = {'part': 'kernel', 'unit': 'us', 'config': f'uint8, lambda per sample, batches of {BATCH}; {args.reps} '
           f'launches x {args.rounds} rounds, ring > {RING_BYTES >> 20} MiB', 'shapes': {}}
    for n, side in SHAPES:
        elems = side * side * 3
        nb = n * elems
        pairs = max(2, -(-RING_BYTES // (2 * nb)))
        ring = [(ch.randint(0, 256, (n, side, side, 3), dtype=ch.uint8, device=dev, generator=gen),
                 ch.empty((n, side, side, 3), dtype=ch.uint8, device=dev)) for _ in range(pairs)]
        lam = ch.rand((n,), dtype=ch.float64, device=dev, generator=gen)
        variants = {f'run{r}': (lambda i, r=r: L.mixup_batch(*ring[i % pairs], lam, BATCH, False, run=r))
                    for r in (8, 4, 2, 1)}
        variants['copy'] = lambda i: ring[i % pairs][1].copy_(ring[i % pairs][0])
        for fn in variants.values():
            for i in range(args.warmup):
                fn(i)
        ch.cuda.synchronize()
        medians = {name: [] for name in variants}
        for _ in range(args.rounds):
            evs = {name: [] for name in variants}
            for i in range(args.reps):
                for name, fn in variants.items():   # the variants alternate
                    a, b = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(i)
                    b.record()
                    evs[name].append((a, b))
            ch.cuda.synchronize()
            for name, ev in evs.items():
                medians[name].append(float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3)
        out = {}
        copy_us = float(np.median(medians['copy']))
        for name in variants:
            m = np.array(medians[name])
            med = float(np.median(m))
            out[name] = {'median_us': round(med, 2), 'min_us': round(float(m.min()), 2),
                         'max_us': round(float(m.max()), 2), 'gb_per_s': round(2 * nb / (med * 1e-6) / 1e9, 1),
                         'of_copy': round(copy_us / med, 3)}
        res['shapes'][f'{n}x{side}x{side}x3'] = {'bytes': 2 * nb, 'ring_pairs': pairs, 'variants': out}
        del ring, variants
        ch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


def _encode_prepared(self, destination, item, malloc):
    """RGBImageField.encode for bytes that are already a JPEG (the bench
    generator's encodings), laid out exactly as the jpg branch writes them."""
    data, h, w = item
    destination['mode'] = 0  # IMAGE_MODES['jpg']
    destination['height'], destination['width'] = h, w
    destination['data_ptr'], storage = malloc(data.nbytes)
    storage[:] = data


def loader_part(args, ch, dev):
    from bench import make_unique, IMAGENET_MEAN, IMAGENET_STD
    from ffcv_amd.writer import DatasetWriter
    from ffcv_amd.fields import RGBImageField, IntField
    from ffcv_amd.fields.decoders import RandomResizedCropRGBImageDecoder, IntDecoder
    from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, ImageMixup, LabelMixup,
                                     MixupToOneHot)
    from ffcv_amd.loader import Loader, OrderOption

    tile, offs, sizes, hs, ws = make_unique('jpg', 256, 4096, 0, 16)

    class DS:  # pre-encoded JPEG bytes, written as they are
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            u = i % len(offs)
            return (tile[offs[u]:offs[u] + sizes[u]], int(hs[u]), int(ws[u])), i % 1000

    fn = os.path.join(args.dir or tempfile.mkdtemp(), f'mixup_bench_{args.n}.beton')
    if not os.path.exists(fn):
        field = RGBImageField(write_mode='jpg')
        field.encode = types.MethodType(_encode_prepared, field)
        DatasetWriter(fn, {'image': field, 'label': IntField()}, num_workers=1).from_indexed_dataset(DS())

    def pipelines(mix):
        image = [RandomResizedCropRGBImageDecoder((224, 224)), Cutout(32, (124, 116, 103))]
        label = [IntDecoder()]
        if mix:
            image.append(ImageMixup(0.5, False))
            label.append(LabelMixup(0.5, False))
        image += [ToTensor(), ToDevice(dev), ToTorchImage(), NormalizeImage(IMAGENET_MEAN, IMAGENET_STD, np.float16)]
        label += [ToTensor(), ToDevice(dev)]
        if mix:
            label.append(MixupToOneHot(1000))
        return {'image': image, 'label': label}

    loaders = {}
    for mix in (False, True):
        for g in (1, None):
            name = ('mixup' if mix else 'base') + ('_g1' if g == 1 else '_grouped')
            loaders[name] = Loader(fn, batch_size=BATCH, order=OrderOption.RANDOM, seed=0, drop_last=True, device=dev,
                                   pipelines=pipelines(mix), batches_per_launch=g)

    def epoch(loader):
        ch.cuda.synchronize()
        t0 = time.perf_counter()
        it = iter(loader)
        n = 0
        for images, labels in it:
            n += int(images.shape[0])
        ch.cuda.synchronize()
        return n / (time.perf_counter() - t0), it.G

    groups = {}
    for name, ld in loaders.items():   # warm-up: buffers, code objects, the entropy index
        _, groups[name] = epoch(ld)
    rates = {name: [] for name in loaders}
    for _ in range(args.epochs):
        for name, ld in loaders.items():   # the Loaders alternate
            rates[name].append(epoch(ld)[0])
    res = {'part': 'loader', 'unit': 'images/s', 'dataset': args.n, 'batch': BATCH, 'epochs': args.epochs,
           'loaders': {name: {'batches_per_launch': groups[name], 'median': round(float(np.median(r))),
                              'min': round(min(r)), 'max': round(max(r))} for name, r in rates.items()}}
    med = {name: float(np.median(r)) for name, r in rates.items()}
    res['mixup_over_base'] = {'g1': round(med['mixup_g1'] / med['base_g1'], 3),
                              'grouped': round(med['mixup_grouped'] / med['base_grouped'], 3)}
    res['grouped_over_g1'] = {'base': round(med['base_grouped'] / med['base_g1'], 2),
                              'mixup': round(med['mixup_grouped'] / med['mixup_g1'], 2)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20, help='timed launches per variant and round')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n', type=int, default=24576, help='samples of the Loader part\'s dataset')
    ap.add_argument('--epochs', type=int, default=3, help='timed epochs per Loader')
    ap.add_argument('--dir', default=None)
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--skip-loader', action='store_true')
    args = ap.parse_args()
    import torch as ch
    assert ch.cuda.is_available(), 'mixup_bench needs the GPU (no CPU fallback)'
    from ffcv_amd import libffcv as L
    dev = ch.device('cuda:0')
    if not args.skip_kernel:
        kernel_part(args, ch, L, dev)
    if not args.skip_loader:
        loader_part(args, ch, dev)


if __name__ == '__main__':
    main()
