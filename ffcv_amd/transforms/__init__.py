from .cutout import Cutout
from .flip import RandomHorizontalFlip
from .translate import RandomTranslate
from .random_resized_crop import RandomResizedCrop
from .color_jitter import (RandomBrightness, RandomContrast, RandomSaturation, RandomGrayscale,
                           RandomSolarization)
from .gaussian_blur import GaussianBlur
from .sharpness import RandomAdjustSharpness
from .auto_augment import TrivialAugmentWide, RandAugment
from .hue import RandomHue, RandomColorJitter
from .affine import RandomAffine, RandomRotation
from .tone import RandomPosterize, RandomAutocontrast, RandomEqualize, RandomInvert
from .mixup import ImageMixup, LabelMixup, MixupToOneHot
from .cutmix import ImageCutMix, LabelCutMix, ImageMixupCutMix, LabelMixupCutMix
from .erase import RandomErasing
from .poison import Poison
from .replace_label import ReplaceLabel
from .ops import ToTensor, ToDevice, ToTorchImage, Convert, View
from .normalize import NormalizeImage
from .module import ModuleWrapper
from .common import Squeeze

__all__ = ['ToTensor', 'ToDevice', 'ToTorchImage', 'NormalizeImage', 'Convert', 'Squeeze', 'View',
           'RandomResizedCrop', 'RandomHorizontalFlip', 'RandomTranslate', 'Cutout', 'ModuleWrapper',
           'RandomBrightness', 'RandomContrast', 'RandomSaturation',
           'RandomGrayscale', 'RandomSolarization', 'GaussianBlur', 'RandomAdjustSharpness', 'RandomHue',
           'RandomColorJitter',
           'RandomAffine', 'RandomRotation', 'TrivialAugmentWide', 'RandAugment',
           'RandomPosterize', 'RandomAutocontrast', 'RandomEqualize', 'RandomInvert',
           'ImageMixup', 'LabelMixup', 'MixupToOneHot', 'ImageCutMix', 'LabelCutMix', 'ImageMixupCutMix',
           'LabelMixupCutMix', 'RandomErasing', 'Poison', 'ReplaceLabel']
