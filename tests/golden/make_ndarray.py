"""Generate tests/golden/ndarray.npz by running the REFERENCE's own
DatasetWriter (num_workers=1) over NDArrayField / TorchTensorField / JSONField
samples, through the stub modules of make_golden.py (this container only; no
test imports this file).  Only the OUTPUTS are saved:

  beton_a    file A, 11 samples: IntField (the sample's index),
             NDArrayField(float32, (5, 3)), NDArrayField(uint8, (7,)),
             TorchTensorField(int16, (2, 2, 3)), JSONField
  beton_b    file B, 9 samples: BytesField of i % 17 + 1 bytes, then
             NDArrayField(float64, (3,)), whose pointers therefore land on
             many residues mod 16
  args_*     the reference fields' to_binary() bytes (1024 each)
  a_f32, a_u8, a_i16, a_json, b_bytes_<i>, b_f64
             the arrays that went in (a_json: one JSON text per sample)

The files' pages are zero padded, so the compressed archive stays small.

Run:  python tests/golden/make_ndarray.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, REF  # noqa: E402

N_A, N_B = 11, 9


def inputs():
    """The samples of both files, from fixed seeds."""
    rng = np.random.default_rng(1711)
    a = {
        'a_f32': rng.normal(0, 3, (N_A, 5, 3)).astype(np.float32),
        'a_u8': rng.integers(0, 256, (N_A, 7), dtype=np.uint8),
        'a_i16': rng.integers(-32768, 32768, (N_A, 2, 2, 3)).astype(np.int16),
    }
    docs = [{'id': i, 'name': 'sample-%d' % i, 'tags': ['t%d' % (i % 3)] * (i % 4), 'score': i / 8,
             'nested': {'ok': i % 2 == 0, 'text': 'héllo 世界' if i % 5 == 0 else None}}
            for i in range(N_A)]
    b_bytes = [rng.integers(1, 256, i % 17 + 1, dtype=np.uint8) for i in range(N_B)]
    b_f64 = rng.normal(0, 1e3, (N_B, 3)).astype(np.float64)
    return a, docs, b_bytes, b_f64


class _DS:
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.rows[i]


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import torch
    import ffcv  # noqa: F401
    from ffcv.writer import DatasetWriter
    from ffcv.fields import IntField, BytesField, NDArrayField, TorchTensorField, JSONField
    a, docs, b_bytes, b_f64 = inputs()
    fields_a = {'index': IntField(), 'mat': NDArrayField(np.dtype('float32'), (5, 3)),
                'vec': NDArrayField(np.dtype('uint8'), (7,)), 'ten': TorchTensorField(torch.int16, (2, 2, 3)),
                'meta': JSONField()}
    fields_b = {'blob': BytesField(), 'xyz': NDArrayField(np.dtype('float64'), (3,))}
    rows_a = [(i, a['a_f32'][i], a['a_u8'][i], torch.from_numpy(a['a_i16'][i].copy()), docs[i]) for i in range(N_A)]
    rows_b = [(b_bytes[i], b_f64[i]) for i in range(N_B)]
    out = dict(a)
    out['a_json'] = np.array([json.dumps(d) for d in docs])
    out['b_f64'] = b_f64
    for i, b in enumerate(b_bytes):
        out[f'b_bytes_{i}'] = b
    with tempfile.TemporaryDirectory() as d:
        for tag, fields, rows in (('a', fields_a, rows_a), ('b', fields_b, rows_b)):
            fn = os.path.join(d, tag + '.beton')
            DatasetWriter(fn, fields, num_workers=1).from_indexed_dataset(_DS(rows))
            out['beton_' + tag] = np.fromfile(fn, np.uint8)
            for name, f in fields.items():
                out[f'args_{tag}_{name}'] = np.asarray(f.to_binary()[0], np.uint8).copy()
    path = os.path.join(HERE, 'ndarray.npz')
    np.savez_compressed(path, **out)
    print('ndarray.npz:', os.path.getsize(path), 'bytes;', {k: v.shape for k, v in out.items() if k.startswith('beton')})


if __name__ == '__main__':
    main()
