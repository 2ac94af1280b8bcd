"""numpy statements of the standalone device operations (cutout, flip, table
lookup, raw gather), written from the reference's definitions that
include/ffcv_hip.h cites, not from the way the kernels index.  Translate is
tests/translate_ref.translate_np."""
import numpy as np


def cutout_np(img, y, x, c, fill):
    """cutout.py:36-47: the c x c square at (y, x) becomes fill; numpy slicing
    drops the part past the bottom or right edge."""
    out = np.array(img, np.uint8)
    out[y:y + c, x:x + c] = np.asarray(fill, np.uint8)
    return out


def flip_np(img, flag):
    """flip.py:35-40: images[i, :, ::-1] where the flag is not zero."""
    img = np.asarray(img)
    return img[:, ::-1].copy() if flag else img.copy()


def lut_np(flat_u8, table):
    """normalize.py:64-65: output[i] = table[input[i] * 3 + i % 3] for a
    (256, 3) table of any dtype over a flat channels-last uint8 array."""
    flat = np.asarray(flat_u8, np.uint8).reshape(-1)
    table = np.asarray(table)
    assert table.shape == (256, 3)
    return table[flat, np.arange(flat.size) % 3]


def gather_raw_np(base, samples, out_stride, background=0xA5):
    """rgb_image.py:123-136, raw branch: row k of the output starts with the
    ``size`` bytes at ``offset`` of a mode-1 sample; everything else (the rest
    of the row, the row of a sample of another mode) keeps ``background``."""
    out = np.full((len(samples), out_stride), background, np.uint8)
    for k, s in enumerate(samples):
        if int(s['mode']) != 1:
            continue
        o, n = int(s['offset']), int(s['size'])
        out[k, :n] = base[o:o + n]
    return out
