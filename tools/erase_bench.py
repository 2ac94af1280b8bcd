"""Device RandomErasing (DESIGN s26): what the fill launch and the draw launch
cost next to a store of the same bytes and next to a launch that erases
nothing, which kernel form does best, and what the operation costs a Loader.

    python tools/erase_bench.py [--reps 20] [--rounds 3] [--n 24576] [--epochs 3] [--skip-loader]

Part 1, the launches alone, from HIP events through the C ABI, the boxes drawn
by ffcv_erase_draw_batch itself (default scale and ratio) at p = 0.25 and
p = 1:

    512 x 32x32x3 uint8        1.5 MB: a launch-latency case
    512 x 224x224x3 float16    154 MB: one ImageNet batch behind NormalizeImage
    12288 x 224x224x3 float16  3.7 GB: one launch group of 24 such batches

  constant  ffcv_erase_batch, one value per channel
  noise     ffcv_erase_batch, the per-pixel noise table
  c/B, n/B, n/B/cache   the same launches in another form
            (ffcv_erase_batch_form): B workgroups per (sample, plane) where
            the product has 8 for a batch and 4 for the group; cache: the table
            read through the cache where the product stages it in LDS
  draw      ffcv_erase_draw_batch with keys
  fill      (a) torch's fill_ of ONE contiguous uint8 tensor of the erased
            bytes: the store roof
  empty     (b) the constant launch on boxes drawn at p = 0: the launch floor

Every variant works through a ring of buffers larger than the 256 MiB Infinity
Cache; the variants of a shape alternate inside each repetition, after a
warm-up of every variant; the measurement is repeated --rounds times to show
the spread.  Per variant: the median / min / max over rounds of the per-round
median microseconds and the ratios of the median to (a) and to (b).

Part 2, one Loader epoch of --n synthetic ImageNet-shape JPEGs (the bench
generator's), batch 512, device cache, entropy index warm, default grouping:

    base   RRC(224) + Cutout(32) + ToTensor + ToDevice + ToTorchImage +
           NormalizeImage fp16 | IntDecoder + ToTensor + ToDevice
    erase  the same with RandomErasing(0.25, value='pixel') after NormalizeImage

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
SHAPES = ((512, 32, 'uint8'), (512, 224, 'float16'), (12288, 224, 'float16'))
PS = (0.25, 1.0)
SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
BANDS = (1, 2, 4, 8, 16)
NOISE_FORMS = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (1, 0), (4, 0), (16, 0))


def kernel_part(args, ch, L, dev):
    from ffcv_amd.transforms.erase import noise_table
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    res = {'part': 'kernel', 'unit': 'us', 'config': f'boxes drawn on the device, scale {SCALE}, ratio {RATIO}; '
           f'{args.reps} launches x {args.rounds} rounds, ring > {RING_BYTES >> 20} MiB', 'shapes': {}}
    for n, side, dtype in SHAPES:
        tdt = getattr(ch, dtype)
        isz = 1 if dtype == 'uint8' else 2
        nb = n * side * side * 3 * isz
        slots = max(2, -(-RING_BYTES // nb))
        ring = [ch.randint(0, 256, (n, side, side, 3), dtype=ch.uint8, device=dev, generator=gen).to(tdt)
                for _ in range(slots)]
        ids = ch.arange(n, dtype=ch.int64, device=dev)
        table = ch.from_numpy(noise_table(128, 64, np.uint8) if isz == 1 else noise_table(0, 1, np.float16)).to(dev)
        pattern = ch.from_numpy(np.array([3, 5, 7], np.uint8 if isz == 1 else np.float16)).to(dev).view(ch.uint8)
        keys = ch.empty(n, dtype=ch.int64, device=dev)
        empty_boxes = ch.zeros((n, 4), dtype=ch.int32, device=dev)
        draw_boxes, draw_keys = ch.empty((n, 4), dtype=ch.int32, device=dev), ch.empty(n, dtype=ch.int64, device=dev)
        shape = {'bytes': nb, 'ring_slots': slots, 'p': {}}
        for p in PS:
            boxes = ch.empty((n, 4), dtype=ch.int32, device=dev)
            L.erase_draw_batch(ids, 0, 0, p, SCALE, RATIO, side, side, boxes, keys)
            ch.cuda.synchronize()
            b = boxes.cpu().numpy().astype(np.int64)
            erased = int((b[:, 2] * b[:, 3]).sum()) * 3 * isz
            flat = [ch.empty(max(erased, 1), dtype=ch.uint8, device=dev)
                    for _ in range(max(2, min(slots, -(-RING_BYTES // max(erased, 1)))))]
            variants = {'constant': lambda i: L.erase_batch(ring[i % slots], boxes, pattern),
                        'noise': lambda i: L.erase_batch(ring[i % slots], boxes, table, keys)}
            for bands in BANDS:
                variants[f'c/{bands}'] = lambda i, f=(bands, 0): L.erase_batch(ring[i % slots], boxes, pattern, form=f)
            for bands, lds in NOISE_FORMS:
                variants[f'n/{bands}' + ('' if lds else '/cache')] = \
                    lambda i, f=(bands, lds): L.erase_batch(ring[i % slots], boxes, table, keys, form=f)
            variants['draw'] = lambda i: L.erase_draw_batch(ids, 0, i, p, SCALE, RATIO, side, side, draw_boxes,
                                                            draw_keys)
            variants['fill'] = lambda i: flat[i % len(flat)].fill_(7)
            variants['empty'] = lambda i: L.erase_batch(ring[i % slots], empty_boxes, pattern)
            # the forms compute the same bytes
            want = L.erase_batch(ring[0].clone(), boxes, table, keys)
            for f in NOISE_FORMS:
                assert ch.equal(L.erase_batch(ring[0].clone(), boxes, table, keys, form=f), want), f
            for fn in variants.values():
                for i in range(args.warmup):
                    fn(i)
            ch.cuda.synchronize()
            medians = {name: [] for name in variants}
            for _ in range(args.rounds):
                evs = {name: [] for name in variants}
                for i in range(args.reps):
                    for name, fn in variants.items():   # the variants alternate
                        a, e = ch.cuda.Event(enable_timing=True), ch.cuda.Event(enable_timing=True)
                        a.record()
                        fn(i)
                        e.record()
                        evs[name].append((a, e))
                ch.cuda.synchronize()
                for name, ev in evs.items():
                    medians[name].append(float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e3)
            fill_us, empty_us = float(np.median(medians['fill'])), float(np.median(medians['empty']))
            out = {}
            for name in variants:
                m = np.array(medians[name])
                med = float(np.median(m))
                out[name] = {'median_us': round(med, 2), 'min_us': round(float(m.min()), 2),
                             'max_us': round(float(m.max()), 2), 'over_fill': round(med / fill_us, 2),
                             'over_empty': round(med / empty_us, 2)}
            shape['p'][str(p)] = {'erased_samples': int((b[:, 2] > 0).sum()), 'erased_bytes': erased, 'variants': out}
            del variants, flat, boxes, want
        res['shapes'][f'{n}x{side}x{side}x3 {dtype}'] = shape
        del ring
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
    from ffcv_amd.transforms import ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomErasing
    from ffcv_amd.loader import Loader, OrderOption

    tile, offs, sizes, hs, ws = make_unique('jpg', 256, 4096, 0, 16)

    class DS:  # pre-encoded JPEG bytes, written as they are
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            u = i % len(offs)
            return (tile[offs[u]:offs[u] + sizes[u]], int(hs[u]), int(ws[u])), i % 1000

    fn = os.path.join(args.dir or tempfile.mkdtemp(), f'erase_bench_{args.n}.beton')
    if not os.path.exists(fn):
        field = RGBImageField(write_mode='jpg')
        field.encode = types.MethodType(_encode_prepared, field)
        DatasetWriter(fn, {'image': field, 'label': IntField()}, num_workers=1).from_indexed_dataset(DS())

    def pipelines(kind):
        image = [RandomResizedCropRGBImageDecoder((224, 224)), Cutout(32, (124, 116, 103)), ToTensor(), ToDevice(dev),
                 ToTorchImage(), NormalizeImage(IMAGENET_MEAN, IMAGENET_STD, np.float16)]
        if kind == 'erase':
            image.append(RandomErasing(0.25, value='pixel'))
        return {'image': image, 'label': [IntDecoder(), ToTensor(), ToDevice(dev)]}

    loaders = {kind: Loader(fn, batch_size=512, order=OrderOption.RANDOM, seed=0, drop_last=True, device=dev,
                            pipelines=pipelines(kind)) for kind in ('base', 'erase')}

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
    res = {'part': 'loader', 'unit': 'images/s', 'dataset': args.n, 'batch': 512, 'epochs': args.epochs,
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
    assert ch.cuda.is_available(), 'erase_bench needs the GPU (no CPU fallback)'
    from ffcv_amd import libffcv as L
    dev = ch.device('cuda:0')
    if not args.skip_kernel:
        kernel_part(args, ch, L, dev)
    if not args.skip_loader:
        loader_part(args, ch, dev)


if __name__ == '__main__':
    main()
