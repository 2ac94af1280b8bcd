"""JSON field (ffcv/fields/json.py): a BytesField whose bytes are a JSON
document followed by a null byte.

The Loader hands out padded uint8 rows (the host ``BytesDecoder``);
:meth:`JSONField.unpack` turns them back into Python objects in the training
loop.  JSON stays on the host on purpose: the rows have a different length
for every sample and end in ``json.loads``, which is host work, so there is
nothing for the device to do with them.
"""
import json

import numpy as np
import torch as ch

from .bytes import BytesField

ENCODING = 'utf8'
SEPARATOR = '\0'  # ends the document inside its padded row


class JSONField(BytesField):
    """A :class:`BytesField` that stores JSON-compatible Python objects.

    The writer takes any object ``json.dumps`` accepts.  The Loader returns
    uint8 rows; call :meth:`unpack` on them to get the objects back.
    """

    @property
    def metadata_type(self) -> np.dtype:
        return np.dtype([('ptr', '<u8'), ('size', '<u8')])

    @staticmethod
    def from_binary(binary) -> 'JSONField':
        return JSONField()

    def encode(self, destination, field, malloc):
        content = (json.dumps(field) + SEPARATOR).encode(ENCODING)
        return super().encode(destination, np.frombuffer(content, dtype='uint8'), malloc)

    @staticmethod
    def unpack(batch):
        """The objects of a batch of rows (a list), or of one row (the object
        itself), from a tensor or an ndarray.  Each row is cut at its first
        null byte; what follows it (the padding up to the longest sample, or
        anything else) is ignored."""
        if isinstance(batch, ch.Tensor):
            batch = batch.cpu().numpy()
        batch = np.asarray(batch)
        single = batch.ndim == 1
        rows = [batch] if single else batch
        result = []
        for row in rows:
            end = np.flatnonzero(row == ord(SEPARATOR))
            text = row[:int(end[0])] if end.size else row
            result.append(json.loads(text.tobytes().decode(ENCODING)))
        return result[0] if single else result
