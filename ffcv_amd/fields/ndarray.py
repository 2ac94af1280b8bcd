"""Fixed-size array fields (ffcv/fields/ndarray.py): NDArrayField,
TorchTensorField and their decoder.

Same descriptors, metadata and file bytes as the reference: the metadata is
the sample's data pointer (``<u8``), the descriptor holds 32 shape slots, the
length of the dtype description and ``json.dumps(dtype.descr)`` in ASCII, and
the data region holds the array's ``element_size`` bytes as they lie in
memory.

The reference decodes with one ``my_memcpy`` per sample on the host
(ndarray.py:19-45).  Here the decoder runs where the Loader's bytes are:

* GPU Loader, ``device_cache=True``: the file is resident in HBM, and one
  launch of ``ffcv_gather_rows`` per launch group copies the batch's rows out
  of it into a device tensor of the field's shape and dtype (the sample ->
  offset lookup happens inside the kernel).  A pointer outside the file gives
  a zero row and a ``DecodeError``.
* GPU Loader, ``device_cache=False``: the rows are gathered on the host into
  a pinned buffer of the slot and copied in with one asynchronous transfer.
* ``device='cpu'``, or a dtype torch has no counterpart for (big-endian, or
  unsigned 16/32/64-bit on a torch without them): the reference's host
  decoder, a numpy batch of the field's dtype, filled by one native gather
  per batch (or ``memory_read`` + ``my_memcpy`` per sample).

``ToTensor`` / ``ToDevice`` behind a device decode pass the tensor through; a
pipeline without ``ToDevice`` gets it back on the host, as for images.
"""
import json
import warnings
from dataclasses import replace
from typing import Callable, Optional, Tuple, Type

import numpy as np
import torch as ch

from .base import Field, ARG_TYPE
from ..pipeline.operation import Operation
from ..pipeline.state import State
from ..pipeline.allocation_query import AllocationQuery

NDArrayArgsType = np.dtype([
    ('shape', '<u8', 32),    # numpy allows at most 32 dimensions
    ('type_length', '<u8'),  # bytes of the dtype description that follows
])


def torch_dtype_of(dtype) -> Optional[ch.dtype]:
    """The torch dtype that holds numpy ``dtype`` bit for bit, or None."""
    try:
        return ch.from_numpy(np.empty(0, dtype=dtype)).dtype
    except (TypeError, ValueError, RuntimeError):
        return None


class NDArrayDecoder(Operation):
    """Default decoder for :class:`NDArrayField` and :class:`TorchTensorField`."""
    device_aware = True
    per_sample = True

    def declare_state_and_memory(self, previous_state: State) -> Tuple[State, AllocationQuery]:
        from .rgb_image import _pipeline_device
        dev = _pipeline_device(self)
        shape = tuple(int(x) for x in self.field.shape)
        dtype = np.dtype(self.field.dtype)
        tdt = torch_dtype_of(dtype)
        self._on_device = dev.type == 'cuda' and tdt is not None
        if self._on_device:
            return (replace(previous_state, jit_mode=False, device=dev, shape=shape, dtype=tdt),
                    (AllocationQuery(shape, tdt, dev),
                     AllocationQuery((1,), ch.int32, dev)))  # gather status
        # host buffers are torch allocations: a dtype torch lacks is allocated
        # as its bytes and viewed as the dtype by the decoder
        self._as_bytes = tdt is None
        alloc_shape, alloc_dtype = (shape + (dtype.itemsize,), np.dtype('<u1')) if self._as_bytes else (shape, dtype)
        return (replace(previous_state, jit_mode=True, shape=shape, dtype=dtype),
                AllocationQuery(alloc_shape, alloc_dtype))

    def generate_code(self) -> Callable:
        from .. import libffcv as L
        shape = tuple(int(x) for x in self.field.shape)
        dtype = np.dtype(self.field.dtype)
        row_bytes = int(self.field.element_size)
        if not self._on_device:
            mem_read = self.memory_read
            as_bytes = self._as_bytes

            def decode_host(indices, destination, metadata, storage_state):
                B = len(indices)
                dst = destination[:B]
                if as_bytes:
                    dst = dst.view(dtype).reshape((B,) + shape)
                ptrs = metadata[np.asarray(indices, dtype=np.int64)].astype(np.uint64)
                mstate = getattr(storage_state, 'host_state', storage_state)  # BatchContext or the tuple
                if isinstance(mstate, tuple) and len(mstate) in (3, 4) and dst.flags['C_CONTIGUOUS']:
                    from ..memory_managers.process_cache import host_source
                    src, src_off = host_source(mstate, ptrs)
                    # a thread per 4 MB (the native gather spawns its threads per call)
                    L.host_gather(src, src_off, np.full(B, row_bytes, np.uint64),
                                  np.arange(B, dtype=np.uint64) * np.uint64(row_bytes), dst,
                                  nthreads=int(min(8, max(1, (B * row_bytes) >> 22))))
                    return dst
                for ix in range(B):  # ndarray.py:37-42
                    data = mem_read(ptrs[ix], storage_state)[:row_bytes]
                    if dst[ix].flags['C_CONTIGUOUS']:
                        L.memcpy(data, dst[ix].reshape(-1).view(np.uint8))
                    else:
                        dst[ix] = np.frombuffer(data, dtype=dtype).reshape(shape)
                return dst
            return decode_host

        f_ix = self._field_index

        def decode(indices, storage, metadata, ss):
            out, status = storage
            B = len(indices)
            ds = ss.dataset
            if ds.data is not None:
                L.gather_rows(ds.data, ds.data_bytes, ds.row_offsets(f_ix), ss.batch_ids, row_bytes, out, row_bytes,
                              status, ss.stream)
                ss.check_status(status[:B], 'NDArrayDecoder')
            else:
                ss.stage_rows(f_ix, row_bytes, out)
            return out[:B]
        return decode


class NDArrayField(Field):
    """A field of fixed-size arrays of any numpy dtype.

    Parameters
    ----------
    dtype : np.dtype
        Element type.
    shape : Tuple[int, ...]
        Shape of every sample's array.
    """

    def __init__(self, dtype: np.dtype, shape: Tuple[int, ...]):
        self.dtype = dtype
        self.shape = shape
        self.element_size = int(dtype.itemsize * np.prod(shape))
        if dtype == np.uint16:
            warnings.warn("Pytorch currently doesn't support uint16; "
                          "we recommend storing as int16 and reinterpreting your data later "
                          "in your pipeline")

    @property
    def metadata_type(self) -> np.dtype:
        return np.dtype('<u8')

    @staticmethod
    def from_binary(binary: ARG_TYPE) -> Field:
        binary = np.ascontiguousarray(binary).reshape(-1).view('<u1')
        head = NDArrayArgsType.itemsize
        args = binary[:head].view(NDArrayArgsType)[0]
        descr = json.loads(binary[head:head + int(args['type_length'])].tobytes().decode('ascii'))
        if len(descr) != 1:
            raise ValueError(f'NDArrayField: a plain dtype is required, got {descr}')
        dtype = np.dtype([tuple(x) for x in descr])['f0']
        shape = [int(x) for x in args['shape']]
        while shape and shape[-1] == 0:
            shape.pop()
        return NDArrayField(dtype, tuple(shape))

    def to_binary(self) -> ARG_TYPE:
        result = np.zeros(1, dtype=ARG_TYPE)[0]
        args = np.zeros(1, dtype=NDArrayArgsType)
        args['shape'][0][:len(self.shape)] = np.asarray(self.shape, dtype='<u8')
        descr = np.frombuffer(json.dumps(np.dtype(self.dtype).descr).encode('ascii'), dtype='<u1')
        args['type_length'][0] = descr.size
        packed = np.concatenate([args.view('<u1'), descr])
        result[0][:packed.size] = packed
        return result

    def encode(self, destination, field, malloc):
        destination[0], data_region = malloc(self.element_size)
        data_region[:] = field.reshape(-1).view('<u1')

    def get_decoder_class(self) -> Type[Operation]:
        return NDArrayDecoder


class TorchTensorField(NDArrayField):
    """A field of fixed-size tensors of any torch dtype (stored, and read
    back, as the numpy arrays they share memory with).

    Parameters
    ----------
    dtype : torch.dtype
        Element type.
    shape : Tuple[int, ...]
        Shape of every sample's tensor.
    """

    def __init__(self, dtype: ch.dtype, shape: Tuple[int, ...]):
        super().__init__(ch.zeros(0, dtype=dtype).numpy().dtype, shape)

    def encode(self, destination, field, malloc):
        return super().encode(destination, field.numpy(), malloc)
