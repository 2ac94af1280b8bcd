from .basics import FloatDecoder, IntDecoder
from .rgb_image import (RandomResizedCropRGBImageDecoder, CenterCropRGBImageDecoder,
                        SimpleRGBImageDecoder)
from .bytes import BytesDecoder
from .ndarray import NDArrayDecoder

__all__ = ['FloatDecoder', 'IntDecoder', 'RandomResizedCropRGBImageDecoder',
           'CenterCropRGBImageDecoder', 'SimpleRGBImageDecoder', 'BytesDecoder', 'NDArrayDecoder']
