from .base import Field
from .basics import FloatField, IntField
from .rgb_image import RGBImageField
from .bytes import BytesField
from .ndarray import NDArrayField, TorchTensorField
from .json import JSONField

__all__ = ['Field', 'BytesField', 'IntField', 'FloatField', 'RGBImageField', 'NDArrayField',
           'JSONField', 'TorchTensorField']
