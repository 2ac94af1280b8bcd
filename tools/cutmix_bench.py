"""Device CutMix (DESIGN s25): what ffcv_cutmix_batch costs next to a copy of
the same bytes, next to the mixup kernel and next to torch's own select, and
what the placement of the image operation costs a Loader.

    python tools/cutmix_bench.py [--reps 20] [--rounds 3] [--n 24576] [--epochs 3] [--skip-loader]

Part 1, the kernel alone, from HIP events through the C ABI, one box per
sample drawn with alpha 1, batches of 512:

    512 x 32x32x3 uint8             1.5 MB: a launch-latency case
    512 x 224x224x3 uint8, fp16     77 / 154 MB: one ImageNet batch
    12288 x 224x224x3 uint8, fp16   1.85 / 3.7 GB: one launch group of 24 batches

  cutmix   ffcv_cutmix_batch
  mixup    ffcv_mixup_batch on the same buffers (uint8 shapes only)
  copy     torch's device copy_ of the same bytes
  where    torch.where(mask, rolled, x) with the mask and the rolled batch
           (roll(1) inside every batch of 512) built inside the timed region,
           as a user without the kernel would write it

Every variant works through a ring of buffer pairs larger than the 256 MiB
Infinity Cache; the variants of a shape alternate inside each repetition,
after a warm-up of every variant; the measurement is repeated --rounds times
to show the spread.  Per variant: the median / min / max over rounds of the
per-round median microseconds, GB/s of algorithmic traffic (one read and one
write of the batch) at the median, and that as a fraction of the copy's.

Part 2, one Loader epoch of --n synthetic ImageNet-shape JPEGs (the bench
generator's), batch 512, device cache, entropy index warm, default grouping:

    base          RRC(224) + Cutout(32) + ToTensor + ToDevice + ToTorchImage +
                  NormalizeImage fp16 | IntDecoder + ToTensor + ToDevice
    mixup_before  ImageMixup(0.5, False) before ToTensor (the decode launch
                  writes uint8, then the mix, then the NormalizeImage table pass)
    cutmix_before ImageCutMix(1.0, False) in the same place
    cutmix_after  ImageCutMix(1.0, False) after NormalizeImage: the fused decode
                  launch stays, the select runs on the float16 batch

the Loaders alternating epoch by epoch after a warm-up epoch of each.  Prints
one JSON line per part.
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
SHAPES = ((512, 32, 'uint8'), (512, 224, 'uint8'), (512, 224, 'float16'), (12288, 224, 'uint8'),
          (12288, 224, 'float16'))
BATCH = 512


def _boxes(n, side):
    rs = np.random.RandomState(0)
    lam = rs.beta(1.0, 1.0, n)
    cy, cx = rs.randint(0, side, n), rs.randint(0, side, n)
    r = np.floor(0.5 * np.sqrt(1.0 - lam) * side).astype(np.int64)
    return np.stack([np.maximum(cy - r, 0), np.maximum(cx - r, 0), np.minimum(cy + r, side),
                     np.minimum(cx + r, side)], 1).astype(np.int32)


def kernel_part(args, ch, L, dev):
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    res = {'part': 'kernel', 'unit': 'us', 'config': f'one box per sample (alpha 1), batches of {BATCH}; {args.reps} '
           f'launches x {args.rounds} rounds, ring > {RING_BYTES >> 20} MiB', 'shapes': {}}
    for n, side, dtype in SHAPES:
        tdt = getattr(ch, dtype)
        nb = n * side * side * 3 * (1 if dtype == 'uint8' else 2)
        pairs = max(2, -(-RING_BYTES // (2 * nb)))
        ring = []
        for _ in range(pairs):
            src = ch.randint(0, 256, (n, side, side, 3), dtype=ch.uint8, device=dev, generator=gen)
            ring.append((src.to(tdt), ch.empty((n, side, side, 3), dtype=tdt, device=dev)))
            del src
        boxes = ch.from_numpy(_boxes(n, side)).to(dev)
        lam = ch.rand((n,), dtype=ch.float64, device=dev, generator=gen)
        rows = ch.arange(side, device=dev).view(1, side, 1, 1)
        cols = ch.arange(side, device=dev).view(1, 1, side, 1)
        y1, x1, y2, x2 = (boxes[:, k].view(n, 1, 1, 1) for k in range(4))

        def where(i):
            x, out = ring[i % pairs]
            mask = (rows >= y1) & (rows < y2) & (cols >= x1) & (cols < x2)
            rolled = x.view(n // BATCH, BATCH, side, side, 3).roll(1, 1).view(n, side, side, 3)
            ch.where(mask, rolled, x, out=out)

        variants = {'cutmix': lambda i: L.cutmix_batch(*ring[i % pairs], boxes, BATCH, False)}
        if dtype == 'uint8':
            variants['mixup'] = lambda i: L.mixup_batch(*ring[i % pairs], lam, BATCH, False)
        variants['copy'] = lambda i: ring[i % pairs][1].copy_(ring[i % pairs][0])
        variants['where'] = where
        # the variants compute the same bytes where they should
        L.cutmix_batch(*ring[0], boxes, BATCH, False)
        got = ring[0][1].clone()
        where(0)
        assert ch.equal(got, ring[0][1]), 'cutmix and torch.where disagree'
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
        shape = {'bytes': 2 * nb, 'ring_pairs': pairs, 'variants': out}
        if 'mixup' in out:
            mix = out['mixup']
            shape['cutmix_minus_mixup_us'] = round(out['cutmix']['median_us'] - mix['median_us'], 2)
            shape['mixup_spread_us'] = round(mix['max_us'] - mix['min_us'], 2)
        res['shapes'][f'{n}x{side}x{side}x3 {dtype}'] = shape
        del ring, variants, where, boxes, got
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
                                     MixupToOneHot, ImageCutMix, LabelCutMix)
    from ffcv_amd.loader import Loader, OrderOption

    tile, offs, sizes, hs, ws = make_unique('jpg', 256, 4096, 0, 16)

    class DS:  # pre-encoded JPEG bytes, written as they are
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            u = i % len(offs)
            return (tile[offs[u]:offs[u] + sizes[u]], int(hs[u]), int(ws[u])), i % 1000

    fn = os.path.join(args.dir or tempfile.mkdtemp(), f'cutmix_bench_{args.n}.beton')
    if not os.path.exists(fn):
        field = RGBImageField(write_mode='jpg')
        field.encode = types.MethodType(_encode_prepared, field)
        DatasetWriter(fn, {'image': field, 'label': IntField()}, num_workers=1).from_indexed_dataset(DS())

    def pipelines(kind):
        image = [RandomResizedCropRGBImageDecoder((224, 224)), Cutout(32, (124, 116, 103))]
        label = [IntDecoder()]
        tail = [ToTensor(), ToDevice(dev), ToTorchImage(), NormalizeImage(IMAGENET_MEAN, IMAGENET_STD, np.float16)]
        if kind == 'mixup_before':
            image += [ImageMixup(0.5, False)] + tail
            label.append(LabelMixup(0.5, False))
        elif kind == 'cutmix_before':
            image += [ImageCutMix(1.0, False)] + tail
            label.append(LabelCutMix(1.0, False, (224, 224)))
        elif kind == 'cutmix_after':
            image += tail + [ImageCutMix(1.0, False)]
            label.append(LabelCutMix(1.0, False, (224, 224)))
        else:
            image += tail
        label += [ToTensor(), ToDevice(dev)]
        if kind != 'base':
            label.append(MixupToOneHot(1000))
        return {'image': image, 'label': label}

    loaders = {kind: Loader(fn, batch_size=BATCH, order=OrderOption.RANDOM, seed=0, drop_last=True, device=dev,
                            pipelines=pipelines(kind))
               for kind in ('base', 'mixup_before', 'cutmix_before', 'cutmix_after')}

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
    med = {name: float(np.median(r)) for name, r in rates.items()}
    res = {'part': 'loader', 'unit': 'images/s', 'dataset': args.n, 'batch': BATCH, 'epochs': args.epochs,
           'loaders': {name: {'batches_per_launch': groups[name], 'median': round(med[name]),
                              'min': round(min(r)), 'max': round(max(r)),
                              'over_base': round(med[name] / med['base'], 3)} for name, r in rates.items()}}
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
    assert ch.cuda.is_available(), 'cutmix_bench needs the GPU (no CPU fallback)'
    from ffcv_amd import libffcv as L
    dev = ch.device('cuda:0')
    if not args.skip_kernel:
        kernel_part(args, ch, L, dev)
    if not args.skip_loader:
        loader_part(args, ch, dev)


if __name__ == '__main__':
    main()
