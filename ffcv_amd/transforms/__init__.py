from .cutout import Cutout
from .flip import RandomHorizontalFlip
from .translate import RandomTranslate
from .color_jitter import RandomBrightness, RandomContrast, RandomSaturation
from .mixup import ImageMixup, LabelMixup, MixupToOneHot
from .ops import ToTensor, ToDevice, ToTorchImage, Convert, View
from .normalize import NormalizeImage
from .module import ModuleWrapper
from .common import Squeeze

__all__ = ['ToTensor', 'ToDevice', 'ToTorchImage', 'NormalizeImage', 'Convert', 'Squeeze', 'View',
           'RandomHorizontalFlip', 'RandomTranslate', 'Cutout', 'ModuleWrapper',
           'RandomBrightness', 'RandomContrast', 'RandomSaturation',
           'ImageMixup', 'LabelMixup', 'MixupToOneHot']
