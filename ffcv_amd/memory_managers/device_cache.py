"""HBM-resident dataset (new; the MI355X counterpart of the OS cache).

The whole ``.beton`` file is copied into device memory once, in chunks from
the memory map, and stays resident across epochs (288 GB of HBM3E holds the
ImageNet-256 JPEG file, 22 GB, many times over).  Decoders then read sample
bytes at their file offsets directly from HBM, so no per-batch PCIe traffic
is needed.  One copy per (file, device) is shared by all Loaders in the
process.
"""
import os
import threading

import numpy as np
import torch as ch

_cache = {}
# zeroed bytes behind the file: kernels that read the resident bytes with
# aligned wide loads may run this far past a sample's end
PADDING = 64
_lock = threading.Lock()


def upload_file(fname, device, chunk=256 << 20):
    key = (os.path.realpath(fname), os.path.getmtime(fname), str(device))
    with _lock:
        if key in _cache:
            return _cache[key]
        mm = np.memmap(fname, 'uint8', mode='r')
        n = mm.shape[0]
        dev = ch.empty(n + PADDING, dtype=ch.uint8, device=device)
        dev[n:].zero_()
        pinned = ch.empty(min(chunk, n) or 1, dtype=ch.uint8).pin_memory()
        s = ch.cuda.Stream(device)
        with ch.cuda.stream(s):
            for off in range(0, n, chunk):
                m = min(chunk, n - off)
                pinned.numpy()[:m] = mm[off:off + m]
                dev[off:off + m].copy_(pinned[:m], non_blocking=True)
                s.synchronize()
        _cache[key] = dev
        return dev
