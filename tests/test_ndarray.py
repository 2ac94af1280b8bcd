"""NDArrayField, TorchTensorField and JSONField on the host (CPU).

tests/golden/ndarray.npz holds two files written by the REFERENCE's own
DatasetWriter (num_workers=1) under the stub harness, the reference fields'
to_binary() bytes and the samples that went in (make_ndarray.py).  Our Reader
must parse the files, our fields must describe themselves with the same
bytes, our DatasetWriter must reproduce the files byte for byte with one
worker and with a pool, and a CPU Loader must hand the samples back exactly.
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from ffcv_amd.fields import IntField, BytesField, NDArrayField, TorchTensorField, JSONField
from ffcv_amd.fields.decoders import NDArrayDecoder
from ffcv_amd.loader import Loader, OrderOption
from ffcv_amd.reader import Reader
from ffcv_amd.writer import DatasetWriter

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(GOLD, 'ndarray.npz'))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def files(gold, tmp_path_factory):
    d = tmp_path_factory.mktemp('ndarray')
    paths = {}
    for tag in 'ab':
        paths[tag] = str(d / f'{tag}.beton')
        gold['beton_' + tag].tofile(paths[tag])
    return paths


def fields_a():
    return {'index': IntField(), 'mat': NDArrayField(np.dtype('float32'), (5, 3)),
            'vec': NDArrayField(np.dtype('uint8'), (7,)), 'ten': TorchTensorField(torch.int16, (2, 2, 3)),
            'meta': JSONField()}


def fields_b():
    return {'blob': BytesField(), 'xyz': NDArrayField(np.dtype('float64'), (3,))}


class DS:
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.rows[i]


def rows_a(gold):
    docs = [json.loads(s) for s in gold['a_json']]
    return [(i, gold['a_f32'][i], gold['a_u8'][i], torch.from_numpy(gold['a_i16'][i].copy()), docs[i])
            for i in range(len(docs))]


def rows_b(gold):
    return [(gold[f'b_bytes_{i}'], gold['b_f64'][i]) for i in range(len(gold['b_f64']))]


# ------------------------------------------------------------ 1. reader --
def test_reader_parses_reference_files(gold, files):
    ra, rb = Reader(files['a']), Reader(files['b'])
    assert ra.num_samples == 11 and ra.field_names == ['index', 'mat', 'vec', 'ten', 'meta']
    assert rb.num_samples == 9 and rb.field_names == ['blob', 'xyz']
    want = {'mat': (np.dtype('<f4'), (5, 3)), 'vec': (np.dtype('u1'), (7,)), 'ten': (np.dtype('<i2'), (2, 2, 3))}
    for name, (dt, shape) in want.items():
        h = ra.handlers[name]
        assert type(h) is NDArrayField  # TorchTensorField inherits from_binary, as in the reference
        assert h.dtype == dt and tuple(h.shape) == shape and h.element_size == dt.itemsize * int(np.prod(shape))
        assert h.metadata_type == np.dtype('<u8')
    assert type(ra.handlers['index']) is IntField and type(ra.handlers['meta']) is JSONField
    assert isinstance(ra.handlers['meta'], BytesField)
    h = rb.handlers['xyz']
    assert type(h) is NDArrayField and h.dtype == np.dtype('<f8') and tuple(h.shape) == (3,)
    # the skewed pointers of file B really cover many residues mod 16
    assert len(set(int(p) % 16 for p in rb.metadata['f1'])) >= 6
    # data where the pointers say
    mm = np.memmap(files['b'], np.uint8, mode='r')
    for i, p in enumerate(rb.metadata['f1']):
        assert np.array_equal(mm[int(p):int(p) + 24].view('<f8'), gold['b_f64'][i])


def test_to_binary_equals_the_reference(gold):
    for tag, fields in (('a', fields_a()), ('b', fields_b())):
        for name, f in fields.items():
            ours = np.asarray(f.to_binary()[0], np.uint8)
            assert np.array_equal(ours, gold[f'args_{tag}_{name}']), (tag, name)
    # and from_binary(to_binary) round-trips dtype and shape, also for a dtype torch lacks
    for dt, shape in [('<f4', (5, 3)), ('>f4', (2, 9)), ('<i8', (1,)), ('|b1', (4, 1, 2))]:
        f = NDArrayField.from_binary(NDArrayField(np.dtype(dt), shape).to_binary()[0])
        assert f.dtype == np.dtype(dt) and tuple(f.shape) == shape


def test_uint16_warns():
    with pytest.warns(UserWarning, match='uint16'):
        NDArrayField(np.dtype('uint16'), (3,))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        NDArrayField(np.dtype('int16'), (3,))


# ------------------------------------------------------------ 2. writer --
@pytest.mark.parametrize('num_workers', [1, 3])
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_writer_reproduces_reference_bytes(gold, tmp_path, tag, num_workers):
    fields, rows = (fields_a(), rows_a(gold)) if tag == 'a' else (fields_b(), rows_b(gold))
    fn = str(tmp_path / 'x.beton')
    DatasetWriter(fn, fields, num_workers=num_workers).from_indexed_dataset(DS(rows), chunksize=4)
    ours = np.fromfile(fn, np.uint8)
    assert ours.shape == gold['beton_' + tag].shape
    assert np.array_equal(ours, gold['beton_' + tag])


# ------------------------------------------------------------ 3. loader --
@pytest.mark.parametrize('order', [OrderOption.SEQUENTIAL, OrderOption.RANDOM])
@pytest.mark.parametrize('os_cache', [True, False])
def test_cpu_loader_file_a(gold, files, hip_lib, os_cache, order):
    """Fails on the parent commit with NotImplementedError (no decoder)."""
    docs = [json.loads(s) for s in gold['a_json']]
    loader = Loader(files['a'], batch_size=4, num_workers=2, os_cache=os_cache, order=order, seed=7,
                    drop_last=False, device='cpu')
    seen = []
    sizes = []
    for index, mat, vec, ten, meta in loader:
        ids = index[:, 0].numpy()
        sizes.append(len(ids))
        seen.extend(int(i) for i in ids)
        for got, key, dt in ((mat, 'a_f32', torch.float32), (vec, 'a_u8', torch.uint8), (ten, 'a_i16', torch.int16)):
            assert isinstance(got, torch.Tensor) and got.dtype == dt and got.device.type == 'cpu'
            assert tuple(got.shape) == (len(ids),) + gold[key].shape[1:]
            assert np.array_equal(got.numpy(), gold[key][ids])
        assert meta.dtype == torch.uint8 and meta.shape[0] == len(ids)
        assert JSONField.unpack(meta) == [docs[i] for i in ids]
    assert sizes == [4, 4, 3] and sorted(seen) == list(range(11))
    if order == OrderOption.SEQUENTIAL:
        assert seen == list(range(11))


@pytest.mark.parametrize('order', [OrderOption.SEQUENTIAL, OrderOption.RANDOM])
@pytest.mark.parametrize('os_cache', [True, False])
def test_cpu_loader_file_b(gold, files, hip_lib, os_cache, order):
    loader = Loader(files['b'], batch_size=4, num_workers=2, os_cache=os_cache, order=order, seed=3,
                    drop_last=False, device='cpu')
    ids = np.asarray(loader.next_traversal_order()).astype(np.int64)
    if order == OrderOption.SEQUENTIAL:
        assert ids.tolist() == list(range(9))
    at = 0
    for blob, xyz in loader:
        b = ids[at:at + len(xyz)]
        at += len(b)
        assert xyz.dtype == torch.float64 and tuple(xyz.shape) == (len(b), 3)
        assert np.array_equal(xyz.numpy(), gold['b_f64'][b])
        for row, i in zip(blob.numpy(), b):
            want = gold[f'b_bytes_{i}']
            assert np.array_equal(row[:len(want)], want)
    assert at == 9


# -------------------------------------------------------------- 4. json --
def test_json_unpack(gold):
    docs = [json.loads(s) for s in gold['a_json']]
    enc = [(json.dumps(d) + '\0').encode('utf8') for d in docs]
    width = max(len(e) for e in enc) + 5
    batch = np.zeros((len(enc), width), np.uint8)
    for i, e in enumerate(enc):
        batch[i, :len(e)] = np.frombuffer(e, np.uint8)
        batch[i, len(e):] = 0x7B + i  # garbage behind the terminator ('{', '|', ...) must be ignored
    assert JSONField.unpack(batch) == docs
    assert JSONField.unpack(batch[3]) == docs[3]
    assert JSONField.unpack(torch.from_numpy(batch)) == docs
    assert JSONField.unpack(torch.from_numpy(batch)[0]) == docs[0]
    # what encode() writes is the document and one null byte
    got = {}

    def malloc(n):
        got['buf'] = np.zeros(n, np.uint8)
        return 1234, got['buf']
    md = np.zeros(1, JSONField().metadata_type)
    JSONField().encode(md, docs[5], malloc)
    assert got['buf'].tobytes() == enc[5] and md['ptr'][0] == 1234 and md['size'][0] == len(enc[5])


# ------------------------------------------- 5. a dtype torch cannot hold --
@pytest.mark.parametrize('os_cache', [True, False])
def test_big_endian_round_trips_as_numpy(tmp_path, hip_lib, os_cache):
    rng = np.random.default_rng(11)
    data = rng.normal(0, 1, (10, 3, 2)).astype('>f4')
    fn = str(tmp_path / 'be.beton')
    DatasetWriter(fn, {'index': IntField(), 'x': NDArrayField(np.dtype('>f4'), (3, 2))},
                  num_workers=1).from_indexed_dataset(DS([(i, data[i]) for i in range(10)]))
    assert Reader(fn).handlers['x'].dtype == np.dtype('>f4')
    loader = Loader(fn, batch_size=4, num_workers=1, os_cache=os_cache, order=OrderOption.RANDOM, seed=1,
                    drop_last=False, device='cpu', pipelines={'x': [NDArrayDecoder()]})
    n = 0
    for index, x in loader:
        ids = index[:, 0].numpy()
        assert isinstance(x, np.ndarray) and x.dtype == np.dtype('>f4') and x.shape == (len(ids), 3, 2)
        assert np.array_equal(x, data[ids])
        n += len(ids)
    assert n == 10


# ----------------------------------------------------------- 6. imports --
def test_reference_import_paths():
    from ffcv.fields.ndarray import NDArrayDecoder as A, NDArrayField as F, TorchTensorField as T
    from ffcv.fields.json import JSONField as J
    from ffcv.fields.decoders import NDArrayDecoder as B
    from ffcv.fields import NDArrayField as F2, TorchTensorField as T2, JSONField as J2
    assert A is B is NDArrayDecoder and F is F2 is NDArrayField and T is T2 is TorchTensorField
    assert J is J2 is JSONField
    assert F(np.dtype('<f4'), (2,)).get_decoder_class() is A
    from ffcv_amd.types import TYPE_ID_HANDLER
    assert TYPE_ID_HANDLER[4] is F and TYPE_ID_HANDLER[5] is J and TYPE_ID_HANDLER[6] is T
