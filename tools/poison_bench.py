"""Device Poison (DESIGN s16): what ffcv_poison_batch costs next to a copy of
the poisoned bytes, which kernel form is fastest, what a launch that finds
nothing to do costs, and what Poison + ReplaceLabel cost a Loader.

    python tools/poison_bench.py [--reps 20] [--rounds 3] [--n 24576] [--epochs 3] [--skip-loader]

Part 1, the kernel alone, from HIP events through the C ABI, in place on uint8:

    12288 x 224x224x3  1.85 GB: one launch group of 24 batches
    512 x 224x224x3    77 MB: one ImageNet batch
    512 x 32x32x3      1.5 MB: a launch-latency case

at poison rates 0, 1 %, 10 % and 100 % of the launch's samples (chosen at
random positions; at rate 0 the set holds as many ids as at 1 %, none of them
in the launch).

  b<B>r<R>   the kernel with B bytes per thread, one workgroup per run of R
             samples and table chunk, the workgroups of a run neighbours
  b<B>r<R>c  the same with the workgroups of a table chunk neighbours
  abi        ffcv_poison_batch itself: the shipped form, its run length chosen
             from the launch's size
  copy       torch's device copy_ of as many samples as are poisoned
  empty      rate 0 only: a launch of one workgroup (ffcv_replace_label_batch
             on one row), what any launch costs

Every variant works through a ring of buffers and, below 100 %, through
disjoint poison sets, so that successive launches touch different bytes (more
than the 256 MiB Infinity Cache where the shape allows); the variants of a
shape alternate inside each repetition, after a warm-up of every variant; the
measurement is repeated --rounds times to show the spread.  Per variant: the
median / min / max over rounds of the per-round median microseconds, GB/s of
algorithmic traffic (one read and one write of the poisoned samples only) at
the median, and that as a fraction of the copy's.

Part 2, one Loader epoch of --n synthetic ImageNet-shape JPEGs (the bench
generator's), batch 512, device cache, entropy index warm:

    base    RRC(224) + Cutout(32) + ToTensor + ToDevice + ToTorchImage +
            NormalizeImage fp16 | IntDecoder + ToTensor + ToDevice
            (lowers to the one fused decode launch)
    poison  the same with Poison (10 % of the dataset) after Cutout and
            ReplaceLabel behind the labels' ToDevice (the decode launch writes
            uint8, then ffcv_poison_batch, then the NormalizeImage table pass)

each at batches_per_launch=1 and at the default grouping, the four Loaders
alternating epoch by epoch after a warm-up epoch of each.  Prints one JSON
line per shape and part.
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
MAX_BUFFERS = 8
MAX_SETS = 64
SHAPES = ((12288, 224), (512, 224), (512, 32))
RATES = (0.0, 0.01, 0.1, 1.0)
FORMS = [(b, r, o) for b in (4, 8, 16) for r in (8, 16, 32, 64) for o in (0, 1)]
DATASET = 1281167


def kernel_part(args, ch, L, dev):
    gen = ch.Generator(device=dev)
    gen.manual_seed(0)
    rng = np.random.default_rng(0)
    one_label = ch.zeros((1, 1), dtype=ch.int64, device=dev)
    one_id = ch.zeros((1,), dtype=ch.int64, device=dev)
    for n, side in SHAPES:
        elems = side * side * 3
        nb = n * elems
        buffers = max(2, min(MAX_BUFFERS, -(-RING_BYTES // nb)))
        ring = [ch.randint(0, 256, (n, side, side, 3), dtype=ch.uint8, device=dev, generator=gen)
                for _ in range(buffers)]
        keep = ch.rand((elems,), dtype=ch.float64, device=dev, generator=gen)
        add = ch.rand((elems,), dtype=ch.float64, device=dev, generator=gen) * 255
        sample_np = rng.permutation(DATASET)[:n].astype(np.int64)
        sample_ids = ch.from_numpy(sample_np).to(dev)
        res = {'part': 'kernel', 'unit': 'us', 'shape': f'{n}x{side}x{side}x3', 'buffers': buffers,
               'config': f'uint8 in place; {args.reps} launches x {args.rounds} rounds', 'rates': {}}
        for rate in RATES:
            hits = n if rate == 1.0 else int(round(rate * n))
            if rate == 0.0:
                sets = [np.sort(DATASET + rng.permutation(DATASET)[:max(1, int(round(0.01 * n)))])]
            else:
                want = -(-RING_BYTES // (buffers * hits * elems))
                nsets = max(1, min(MAX_SETS, n // hits, want))
                perm = rng.permutation(n)
                sets = [np.sort(sample_np[perm[j * hits:(j + 1) * hits]]) for j in range(nsets)]
            d_sets = [ch.from_numpy(s.astype(np.int64)).to(dev) for s in sets]
            nsets = len(d_sets)

            def poison(i, form):
                L.poison_batch(ring[i % buffers], sample_ids, d_sets[(i // buffers) % nsets], keep, add, form=form)

            variants = {f'b{b}r{r}' + 'c' * o: (lambda i, f=(b, r, o): poison(i, f)) for b, r, o in FORMS}
            variants['abi'] = lambda i: poison(i, None)
            if hits:
                def copy(i):
                    lo = ((i // buffers) % nsets) * hits
                    ring[(i + 1) % buffers][lo:lo + hits].copy_(ring[i % buffers][lo:lo + hits])
                variants['copy'] = copy
            else:
                variants['empty'] = lambda i: L.replace_label_batch(one_label, one_id, one_id, 1)
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
            yard = float(np.median(medians['copy' if hits else 'empty']))
            for name in variants:
                m = np.array(medians[name])
                med = float(np.median(m))
                out[name] = {'median_us': round(med, 2), 'min_us': round(float(m.min()), 2),
                             'max_us': round(float(m.max()), 2)}
                if hits:
                    out[name]['gb_per_s'] = round(2 * hits * elems / (med * 1e-6) / 1e9, 1)
                    out[name]['of_copy'] = round(yard / med, 3)
                else:
                    out[name]['over_empty'] = round(med / yard, 2)
            res['rates'][str(rate)] = {'poisoned_samples': hits, 'poison_sets': nsets, 'set_size': int(len(sets[0])),
                                       'bytes': 2 * hits * elems, 'variants': out}
        print(json.dumps(res), flush=True)
        del ring, variants
        ch.cuda.empty_cache()


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
    from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, Poison, ReplaceLabel)
    from ffcv_amd.loader import Loader, OrderOption

    tile, offs, sizes, hs, ws = make_unique('jpg', 256, 4096, 0, 16)

    class DS:  # pre-encoded JPEG bytes, written as they are
        def __len__(self):
            return args.n

        def __getitem__(self, i):
            u = i % len(offs)
            return (tile[offs[u]:offs[u] + sizes[u]], int(hs[u]), int(ws[u])), i % 1000

    fn = os.path.join(args.dir or tempfile.mkdtemp(), f'poison_bench_{args.n}.beton')
    if not os.path.exists(fn):
        field = RGBImageField(write_mode='jpg')
        field.encode = types.MethodType(_encode_prepared, field)
        DatasetWriter(fn, {'image': field, 'label': IntField()}, num_workers=1).from_indexed_dataset(DS())

    rng = np.random.default_rng(0)
    mask = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    alpha = np.zeros((224, 224), np.float32)
    alpha[-32:, -32:] = 1.0                                  # an opaque corner trigger
    chosen = rng.permutation(args.n)[:args.n // 10]

    def pipelines(poison):
        image = [RandomResizedCropRGBImageDecoder((224, 224)), Cutout(32, (124, 116, 103))]
        label = [IntDecoder(), ToTensor(), ToDevice(dev)]
        if poison:
            image.append(Poison(mask, alpha, chosen))
            label.append(ReplaceLabel(chosen, 0))
        image += [ToTensor(), ToDevice(dev), ToTorchImage(), NormalizeImage(IMAGENET_MEAN, IMAGENET_STD, np.float16)]
        return {'image': image, 'label': label}

    loaders = {}
    for poison in (False, True):
        for g in (1, None):
            name = ('poison' if poison else 'base') + ('_g1' if g == 1 else '_grouped')
            loaders[name] = Loader(fn, batch_size=512, order=OrderOption.RANDOM, seed=0, drop_last=True, device=dev,
                                   pipelines=pipelines(poison), batches_per_launch=g)

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
    res = {'part': 'loader', 'unit': 'images/s', 'dataset': args.n, 'batch': 512, 'epochs': args.epochs,
           'poisoned': int(len(chosen)),
           'loaders': {name: {'batches_per_launch': groups[name], 'median': round(float(np.median(r))),
                              'min': round(min(r)), 'max': round(max(r))} for name, r in rates.items()}}
    med = {name: float(np.median(r)) for name, r in rates.items()}
    res['poison_over_base'] = {'g1': round(med['poison_g1'] / med['base_g1'], 3),
                               'grouped': round(med['poison_grouped'] / med['base_grouped'], 3)}
    res['grouped_over_g1'] = {'base': round(med['base_grouped'] / med['base_g1'], 2),
                              'poison': round(med['poison_grouped'] / med['poison_g1'], 2)}
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
    assert ch.cuda.is_available(), 'poison_bench needs the GPU (no CPU fallback)'
    from ffcv_amd import libffcv as L
    dev = ch.device('cuda:0')
    if not args.skip_kernel:
        kernel_part(args, ch, L, dev)
    if not args.skip_loader:
        loader_part(args, ch, dev)


if __name__ == '__main__':
    main()
