"""ffcv_gather_rows and NDArrayDecoder on the MI355X.

The ABI sweep compares the kernel with numpy slicing, byte for byte, for row
sizes around every vector width and every dispatch threshold, with sources at
all 16 residues mod 16 (one row at offset 0, one ending exactly at
base_bytes), dense and strided outputs inside guarded buffers, shuffled ids
with a duplicate; ids and offsets out of range give zero rows and a non-zero
status and touch nothing else.  The Loader cases read NDArray / TorchTensor
fields on the HBM-resident path (launch groups of 1 and 3), on the PCIe
staging path and through a default pipeline, against the arrays written.
"""
import os

import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.fields import IntField, BytesField, NDArrayField, TorchTensorField, JSONField
from ffcv_amd.fields.decoders import NDArrayDecoder
from ffcv_amd.loader import Loader, OrderOption
from ffcv_amd.loader.epoch_iterator import launch_group
from ffcv_amd.transforms import ToTensor, ToDevice
from ffcv_amd.writer import DatasetWriter

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
POOL = 1 << 16      # bytes of the source buffer
GUARD = 64
FILL = 0xA5
EINVAL = -1
RANGE = 8           # FFCV_SAMPLE_RANGE


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def pool():
    """64 KiB of random bytes, on the host and on the device (one reference
    for every case; nothing writes to it)."""
    host = np.random.default_rng(2024).integers(0, 256, POOL, dtype=np.uint8)
    dev = ch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return host, dev


# row sizes: around every vector width, and around the two dispatch thresholds
# (read from the library when the test runs), and rows of more than one chunk
SIZES = [1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4099, 16384 + 16, 2 * 16384 + 77,
         'cut-1', 'cut', 'cut+1', 'sub-1', 'sub', 'sub+1']


def _size(rb):
    if isinstance(rb, int):
        return rb
    name, _, delta = rb.partition('+') if '+' in rb else rb.partition('-') if '-' in rb else (rb, '', '0')
    base = {'cut': L.gather_rows_cutover, 'sub': L.gather_rows_subwave}[name]()
    return base + (int(delta) if '+' in rb else -int(delta))


def _offsets(rng, rb):
    """base_bytes and 16 row offsets at the 16 residues mod 16: one at 0, one
    ending exactly at base_bytes (residue 5), the others anywhere."""
    base_bytes = POOL - ((POOL - rb - 5) % 16)
    assert base_bytes <= POOL and (base_bytes - rb) % 16 == 5 and base_bytes - rb > 32
    offs = []
    for r in range(16):
        if r == 0:
            offs.append(0)
        elif r == 5:
            offs.append(base_bytes - rb)
        else:
            hi = (base_bytes - rb - r) // 16       # largest q with 16 q + r + rb <= base_bytes
            offs.append(16 * int(rng.integers(0, hi + 1)) + r)
    offs = np.array(offs, np.uint64)
    assert sorted(int(o) % 16 for o in offs) == list(range(16)) and int((offs + np.uint64(rb)).max()) == base_bytes
    return base_bytes, offs


def _run(pool, rb, offs, ids, base_bytes, gap=0, lead=0, shape=None):
    """One call inside a guarded output buffer; returns (rows, status) after
    checking that guards and gaps still hold the fill pattern."""
    host, dev = pool
    B, stride = len(ids), rb + gap
    buf = ch.full((GUARD + lead + B * stride + GUARD,), FILL, dtype=ch.uint8, device=DEV)
    out = buf[GUARD + lead:GUARD + lead + B * stride]
    status = ch.full((B + 2,), 77, dtype=ch.int32, device=DEV)
    L.gather_rows(dev, base_bytes, ch.from_numpy(offs.view(np.int64)).to(DEV),
                  ch.from_numpy(np.asarray(ids, np.uint64).view(np.int64)).to(DEV), rb, out, stride, status[:B],
                  shape=shape)
    ch.cuda.synchronize()
    got = buf.cpu().numpy()
    st = status.cpu().numpy()
    assert (got[:GUARD + lead] == FILL).all() and (got[GUARD + lead + B * stride:] == FILL).all()
    assert (st[B:] == 77).all()
    rows = got[GUARD + lead:GUARD + lead + B * stride].reshape(B, stride)
    assert (rows[:, rb:] == FILL).all()
    return rows[:, :rb], st[:B]


def _want(host, rb, offs, ids):
    return np.stack([host[int(offs[i]):int(offs[i]) + rb] for i in ids])


@pytest.mark.parametrize('gap,lead', [(0, 0), (5, 9)], ids=['dense', 'strided'])
@pytest.mark.parametrize('rb', SIZES)
def test_rows_equal_numpy_slices(pool, rb, gap, lead):
    rb = _size(rb)
    rng = np.random.default_rng(rb * 2 + gap)
    base_bytes, offs = _offsets(rng, rb)
    ids = rng.permutation(16).tolist()
    ids.insert(int(rng.integers(0, 17)), ids[3])       # a duplicate
    got, st = _run(pool, rb, offs, ids, base_bytes, gap, lead)
    assert (st == 0).all()
    want = _want(pool[0], rb, offs, ids)
    bad = [k for k in range(len(ids)) if not np.array_equal(got[k], want[k])]
    assert not bad, (rb, bad)


@pytest.mark.parametrize('shape', [1, 2, 3])
@pytest.mark.parametrize('rb', [7, 48, 1000, 4099, 16384 + 16 + 9])
def test_every_dispatch_shape_at_every_size(pool, rb, shape):
    """The shapes the host would not pick for a size are correct too (the
    cut-over sweep times them)."""
    rng = np.random.default_rng(rb + shape)
    base_bytes, offs = _offsets(rng, rb)
    ids = rng.permutation(16).tolist() + [2]
    got, st = _run(pool, rb, offs, ids, base_bytes, gap=3, lead=1, shape=shape)
    assert (st == 0).all() and np.array_equal(got, _want(pool[0], rb, offs, ids))


@pytest.mark.parametrize('rb', [24, 1000, 'cut+40'])
def test_bad_rows_are_zero_with_status(pool, rb):
    """An id of n_rows, an offset one byte too far, one far past the end and
    one that wraps around: zero rows, status FFCV_SAMPLE_RANGE; all other rows
    correct with status 0; the process goes on (nothing out of bounds is
    touched: the kernel does not read a bad row)."""
    rb = _size(rb)
    rng = np.random.default_rng(rb)
    base_bytes, offs = _offsets(rng, rb)
    offs = np.concatenate([offs, np.array([base_bytes - rb + 1, base_bytes + 4096, 2 ** 64 - 8], np.uint64)])
    n_rows = len(offs)
    ids = [4, n_rows, 16, 0, 17, 5, 18, 9, 2 ** 63 + 1]
    bad = {1, 2, 4, 6, 8}
    got, st = _run(pool, rb, offs, ids, base_bytes, gap=5, lead=3)
    for k, i in enumerate(ids):
        if k in bad:
            assert st[k] == RANGE and not got[k].any(), k
        else:
            assert st[k] == 0 and np.array_equal(got[k], pool[0][int(offs[i]):int(offs[i]) + rb]), k
    # and the next call works
    got, st = _run(pool, rb, offs[:16], [3, 1], base_bytes)
    assert (st == 0).all() and np.array_equal(got, _want(pool[0], rb, offs, [3, 1]))


def test_more_rows_than_the_grid_is_high(pool):
    """70 000 rows through the 2-D grid (y is folded at 65 535), small rows."""
    host, dev = pool
    rng = np.random.default_rng(5)
    rb, B = 40, 70000
    offs = rng.integers(0, POOL - rb, 512).astype(np.uint64)
    ids = rng.integers(0, 512, B).astype(np.int64)
    out = ch.zeros((B, rb), dtype=ch.uint8, device=DEV)
    status = ch.ones(B, dtype=ch.int32, device=DEV)
    L.gather_rows(dev, POOL, ch.from_numpy(offs.view(np.int64)).to(DEV), ch.from_numpy(ids).to(DEV), rb, out, rb,
                  status, shape=3)
    ch.cuda.synchronize()
    assert not status.any()
    idx = (offs[ids].astype(np.int64)[:, None] + np.arange(rb)[None, :])
    assert np.array_equal(out.cpu().numpy(), host[idx])


def test_a_row_longer_than_the_grid_is_wide():
    """One 64 MiB + row: its chunks outnumber the grid's x dimension."""
    rb = (4096 * 16384) + 3 * 16384 + 21
    g = ch.Generator(device=DEV)
    g.manual_seed(3)
    src = ch.randint(0, 256, (rb + 64,), dtype=ch.uint8, device=DEV, generator=g)
    out = ch.full((rb + 32,), FILL, dtype=ch.uint8, device=DEV)
    status = ch.ones(1, dtype=ch.int32, device=DEV)
    L.gather_rows(src, rb + 19, ch.tensor([19], dtype=ch.int64, device=DEV), ch.zeros(1, dtype=ch.int64, device=DEV),
                  rb, out[7:], rb, status)
    ch.cuda.synchronize()
    assert int(status[0]) == 0 and ch.equal(out[7:7 + rb], src[19:19 + rb])
    assert bool((out[:7] == FILL).all()) and bool((out[7 + rb:] == FILL).all())


def test_argument_errors_return_einval_without_a_launch(pool):
    host, dev = pool
    lib = L.lib()
    off = ch.zeros(4, dtype=ch.int64, device=DEV)
    ids = ch.zeros(4, dtype=ch.int64, device=DEV)
    out = ch.full((4 * 32,), FILL, dtype=ch.uint8, device=DEV)
    st = ch.full((4,), 77, dtype=ch.int32, device=DEV)
    ch.cuda.synchronize()

    def call(base=dev.data_ptr(), nbytes=POOL, ro=off.data_ptr(), n=4, i=ids.data_ptr(), b=4, rb=24,
             o=out.data_ptr(), stride=32, s=st.data_ptr()):
        return lib.ffcv_gather_rows(None, base, nbytes, ro, n, i, b, rb, o, stride, s)
    for kw in (dict(base=None), dict(ro=None), dict(i=None), dict(o=None), dict(s=None), dict(rb=0),
               dict(stride=23), dict(stride=0), dict(base=dev.data_ptr() + 1), dict(base=dev.data_ptr() + 8),
               dict(b=-1)):
        assert call(**kw) == EINVAL and b'ffcv_gather_rows' in lib.ffcv_last_error(), kw
    assert call(b=0) == 0                                    # an empty batch: no launch
    ch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((st == 77).all())      # nothing was launched
    assert call() == 0
    ch.cuda.synchronize()
    assert not st.any() and np.array_equal(out.cpu().numpy().reshape(4, 32)[:, :24], np.tile(host[:24], (4, 1)))


# ------------------------------------------------------------------ Loader --
N = 37


class DS:
    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        return self.rows[i]


@pytest.fixture(scope='module')
def data_a():
    rng = np.random.default_rng(99)
    return {'mat': rng.normal(0, 3, (N, 5, 3)).astype(np.float32),
            'vec': rng.integers(0, 256, (N, 7), dtype=np.uint8),
            'ten': rng.integers(-32768, 32768, (N, 2, 2, 3)).astype(np.int16),
            'meta': [{'id': i, 'tags': ['x'] * (i % 5)} for i in range(N)]}


@pytest.fixture(scope='module')
def file_a(data_a, tmp_path_factory):
    """File A's fields, 37 samples, written here."""
    fn = str(tmp_path_factory.mktemp('nd') / 'a.beton')
    rows = [(i, data_a['mat'][i], data_a['vec'][i], ch.from_numpy(data_a['ten'][i].copy()), data_a['meta'][i])
            for i in range(N)]
    DatasetWriter(fn, {'index': IntField(), 'mat': NDArrayField(np.dtype('float32'), (5, 3)),
                       'vec': NDArrayField(np.dtype('uint8'), (7,)),
                       'ten': TorchTensorField(ch.int16, (2, 2, 3)), 'meta': JSONField()},
                  num_workers=1).from_indexed_dataset(DS(rows))
    return fn


def _device_pipelines():
    return {name: [NDArrayDecoder(), ToTensor(), ToDevice(ch.device(DEV))] for name in ('mat', 'vec', 'ten')}


def _check_epochs(loader, data_a, want_g, on_device=True):
    assert loader.graph.groupable()
    assert launch_group(loader, len(loader)) == want_g
    orders = []
    for _ in range(2):
        it = iter(loader)
        assert it.G == want_g                                # the iterator actually grouped
        seen, sizes = [], []
        for index, mat, vec, ten, meta in it:
            ids = index[:, 0].cpu().numpy()
            sizes.append(len(ids))
            seen.extend(int(i) for i in ids)
            for got, key, dt in ((mat, 'mat', ch.float32), (vec, 'vec', ch.uint8), (ten, 'ten', ch.int16)):
                assert isinstance(got, ch.Tensor) and got.dtype == dt
                assert got.device.type == ('cuda' if on_device else 'cpu')
                assert tuple(got.shape) == (len(ids),) + data_a[key].shape[1:]
                assert np.array_equal(got.cpu().numpy(), data_a[key][ids]), key
            assert JSONField.unpack(meta) == [data_a['meta'][i] for i in ids]
        assert sizes == [8, 8, 8, 8, 5] and sorted(seen) == list(range(N))
        orders.append(seen)
    assert orders[0] != orders[1]


@pytest.mark.parametrize('bpl', [1, 3])
def test_loader_device_cache(file_a, data_a, bpl):
    loader = Loader(file_a, batch_size=8, num_workers=2, order=OrderOption.RANDOM, seed=17, drop_last=False,
                    pipelines=_device_pipelines(), device=DEV, device_cache=True, batches_per_launch=bpl)
    _check_epochs(loader, data_a, bpl)


def test_loader_pcie_staging(file_a, data_a):
    loader = Loader(file_a, batch_size=8, num_workers=2, order=OrderOption.RANDOM, seed=17, drop_last=False,
                    pipelines=_device_pipelines(), device=DEV, device_cache=False, batches_per_launch=3)
    _check_epochs(loader, data_a, 3)


def test_loader_pcie_staging_process_cache(file_a, data_a):
    loader = Loader(file_a, batch_size=8, num_workers=2, os_cache=False, order=OrderOption.RANDOM, seed=17,
                    drop_last=False, pipelines=_device_pipelines(), device=DEV, device_cache=False)
    _check_epochs(loader, data_a, 5)                         # the default: all five batches in one launch


def test_loader_default_pipeline_returns_host_tensors(file_a, data_a):
    loader = Loader(file_a, batch_size=8, num_workers=2, order=OrderOption.RANDOM, seed=17, drop_last=False,
                    device=DEV, batches_per_launch=3)
    _check_epochs(loader, data_a, 3, on_device=False)


def test_loader_skewed_pointers(tmp_path):
    """File B of the golden set (a BytesField of 1..17 bytes in front of a
    float64 triple: pointers on many residues mod 16), written here."""
    g = np.load(os.path.join(GOLD, 'ndarray.npz'))
    xyz = g['b_f64']
    rows = [(g[f'b_bytes_{i}'], xyz[i]) for i in range(len(xyz))]
    fn = str(tmp_path / 'b.beton')
    DatasetWriter(fn, {'blob': BytesField(), 'xyz': NDArrayField(np.dtype('float64'), (3,))},
                  num_workers=1).from_indexed_dataset(DS(rows))
    assert np.array_equal(np.fromfile(fn, np.uint8), g['beton_b'])
    loader = Loader(fn, batch_size=4, num_workers=1, order=OrderOption.RANDOM, seed=5, drop_last=False,
                    pipelines={'xyz': [NDArrayDecoder(), ToTensor(), ToDevice(ch.device(DEV))]}, device=DEV,
                    device_cache=True)
    assert len(set(int(p) % 16 for p in loader.reader.metadata['f1'])) >= 6
    ids = np.asarray(loader.next_traversal_order()).astype(np.int64)
    at = 0
    for blob, got in loader:
        b = ids[at:at + len(got)]
        at += len(b)
        assert got.device.type == 'cuda' and got.dtype == ch.float64 and tuple(got.shape) == (len(b), 3)
        assert np.array_equal(got.cpu().numpy(), xyz[b])
        for row, i in zip(blob.numpy(), b):
            assert np.array_equal(row[:i % 17 + 1], g[f'b_bytes_{i}'])
    assert at == 9
