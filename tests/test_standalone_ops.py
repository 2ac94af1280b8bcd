"""Cutout, RandomHorizontalFlip and RandomTranslate refuse a device state that
is not a uint8 (H, W, 3) image (behind ToTorchImage their kernels would read
an NCHW view of channels-last storage as H = 3, W = H), declare what they
always declared on image states, and their ctypes wrappers refuse a tensor
the kernels would misread before the library is reached.  No GPU needed."""
import numpy as np
import pytest
import torch as ch

from ffcv_amd import libffcv as L
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder
from ffcv_amd.memory_managers import OSCacheManager
from ffcv_amd.pipeline import PipelineSpec
from ffcv_amd.pipeline.graph import Graph
from ffcv_amd.pipeline.state import State
from ffcv_amd.reader import Reader
from ffcv_amd.transforms import (Convert, Cutout, NormalizeImage, RandomHorizontalFlip, RandomInvert, RandomTranslate,
                                 ToDevice, ToTensor, ToTorchImage)
from tests.helpers import NaturalDS, write

OPS = {'Cutout': lambda: Cutout(2, (1, 2, 3)), 'RandomHorizontalFlip': lambda: RandomHorizontalFlip(0.5),
       'RandomTranslate': lambda: RandomTranslate(2, (1, 2, 3))}
CUDA = ch.device('cuda:0')


@pytest.fixture(scope='module')
def beton(tmp_path_factory):
    return write(str(tmp_path_factory.mktemp('standalone') / 'raw.beton'), NaturalDS(6, hw=(32, 32)),
                 {'image': RGBImageField(write_mode='raw'), 'label': IntField()})


def _graph(beton, ops):
    r = Reader(beton)
    return Graph({'image': PipelineSpec('image', transforms=ops)}, r.handlers, {'image': 0, 'label': 1}, r.metadata,
                 OSCacheManager(r).compile_reader(), device='cuda:0')


@pytest.mark.parametrize('name', sorted(OPS))
def test_behind_totorchimage_on_the_device_raises(beton, name):
    """[decoder, ToTensor, ToDevice, ToTorchImage, op]: the state is (3, 32, 32)."""
    g = _graph(beton, [SimpleRGBImageDecoder(), ToTensor(), ToDevice(CUDA), ToTorchImage(), OPS[name]()])
    with pytest.raises(TypeError, match=rf'{name} works on uint8 \(H, W, 3\) images, got torch.uint8 \(3, 32, 32\): '
                                        r'place it before ToTorchImage / NormalizeImage / Convert'):
        g.collect_requirements()


@pytest.mark.parametrize('name', sorted(OPS))
def test_behind_a_dtype_change_on_the_device_raises(beton, name):
    mean, std = np.array([125.3, 123.0, 113.9]), np.array([51.6, 50.8, 51.3])
    for middle in ([Convert(ch.float16)], [ToTorchImage(), NormalizeImage(mean, std, np.float32)]):
        g = _graph(beton, [SimpleRGBImageDecoder(), ToTensor(), ToDevice(CUDA)] + middle + [OPS[name]()])
        with pytest.raises(TypeError, match=f'{name} works on uint8'):
            g.collect_requirements()


@pytest.mark.parametrize('name', sorted(OPS))
def test_in_front_of_totorchimage_still_builds(beton, name):
    op = OPS[name]()       # behind RandomInvert, which ends the decoder's fused prefix: the operation runs itself
    g = _graph(beton, [SimpleRGBImageDecoder(), ToTensor(), ToDevice(CUDA), RandomInvert(), op, ToTorchImage()])
    g.collect_requirements()
    assert not op._absorbed
    last = g.states[g.outputs['image'].id]
    assert tuple(last.shape) == (3, 32, 32) and last.dtype == ch.uint8 and last.device.type == 'cuda'


def _declared(op, state):
    st, alloc = op.declare_state_and_memory(state)
    return ((st.jit_mode, str(st.device), tuple(st.shape), str(st.dtype)),
            None if alloc is None else (tuple(alloc.shape), str(alloc.dtype), str(alloc.device)))


# What the parent revision declared for (H, W, 3) states, recorded from it:
# a host numpy stage, a host tensor stage, and a device stage.
HOST_NP = State(True, ch.device('cpu'), (13, 10, 3), np.dtype('uint8'))
HOST_CH = State(False, ch.device('cpu'), (13, 10, 3), ch.uint8)
DEVICE = State(False, CUDA, (13, 10, 3), ch.uint8)
RECORDED = {
    ('Cutout', 'host_np'): ((True, 'cpu', (13, 10, 3), 'uint8'), None),
    ('Cutout', 'host_ch'): ((False, 'cpu', (13, 10, 3), 'torch.uint8'), None),
    ('Cutout', 'device'): ((False, 'cuda:0', (13, 10, 3), 'torch.uint8'), None),
    ('RandomHorizontalFlip', 'host_np'): ((True, 'cpu', (13, 10, 3), 'uint8'), ((13, 10, 3), 'uint8', 'None')),
    ('RandomHorizontalFlip', 'host_ch'): ((False, 'cpu', (13, 10, 3), 'torch.uint8'),
                                          ((13, 10, 3), 'torch.uint8', 'None')),
    ('RandomHorizontalFlip', 'device'): ((False, 'cuda:0', (13, 10, 3), 'torch.uint8'),
                                         ((13, 10, 3), 'torch.uint8', 'cuda:0')),
    ('RandomTranslate', 'host_np'): ((True, 'cpu', (13, 10, 3), 'uint8'), ((13, 10, 3), 'uint8', 'None')),
    ('RandomTranslate', 'host_ch'): ((False, 'cpu', (13, 10, 3), 'torch.uint8'),
                                     ((13, 10, 3), 'torch.uint8', 'None')),
    ('RandomTranslate', 'device'): ((False, 'cuda:0', (13, 10, 3), 'torch.uint8'),
                                    ((13, 10, 3), 'torch.uint8', 'cuda:0')),
}


@pytest.mark.parametrize('name', sorted(OPS))
def test_image_states_declare_what_they_declared(name):
    for key, state in (('host_np', HOST_NP), ('host_ch', HOST_CH), ('device', DEVICE)):
        assert _declared(OPS[name](), state) == RECORDED[name, key], (name, key)


def test_host_states_are_not_restricted():
    """The host (numpy) paths index whatever they are given, as before."""
    chw = State(True, ch.device('cpu'), (3, 13, 10), np.dtype('float32'))
    for name in sorted(OPS):
        st, _ = OPS[name]().declare_state_and_memory(chw)
        assert tuple(st.shape) == (3, 13, 10) and st.jit_mode


def test_wrappers_refuse_what_the_kernels_would_misread(monkeypatch):
    """A permuted view and a wrong trailing dimension raise TypeError naming the
    wrapper; the library is not reached."""
    def no_lib():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(L, 'lib', no_lib)
    monkeypatch.setattr(L, '_stream', lambda stream: None)
    hwc = ch.zeros((2, 8, 8, 3), dtype=ch.uint8)
    nchw = hwc.permute(0, 3, 1, 2)                     # what ToTorchImage hands on
    assert not nchw.is_contiguous()
    four = ch.zeros((2, 8, 8, 4), dtype=ch.uint8)
    half = ch.zeros((2, 8, 8, 3), dtype=ch.float16)
    yx = ch.zeros((2, 2), dtype=ch.int32)
    flips = ch.zeros(2, dtype=ch.uint8)
    for bad in (nchw, four, half, hwc.numpy(), hwc[:, :, ::2]):
        with pytest.raises(TypeError, match='cutout_batch: a contiguous uint8'):
            L.cutout_batch(bad, yx, 2, (1, 2, 3))
        with pytest.raises(TypeError, match='translate_batch: a contiguous uint8'):
            L.translate_batch(bad, ch.zeros_like(hwc), yx, 1, (1, 2, 3))
    with pytest.raises(TypeError, match='translate_batch: a contiguous uint8'):
        L.translate_batch(hwc, nchw, yx, 1, (1, 2, 3))
    for bad in (nchw, hwc[:, :, ::2], hwc.numpy()):
        with pytest.raises(TypeError, match='flip_batch: a contiguous device'):
            L.flip_batch(bad, ch.zeros_like(hwc), flips)
    with pytest.raises(TypeError, match='flip_batch: a contiguous device'):
        L.flip_batch(hwc, ch.zeros_like(hwc).permute(0, 2, 1, 3), flips)
    lut = ch.zeros((256, 3), dtype=ch.float16)
    out = ch.zeros((2, 8, 8, 3), dtype=ch.float16)
    for args in ((nchw, lut, out), (hwc, lut.t(), out), (hwc, lut, out.permute(0, 3, 1, 2))):
        with pytest.raises(TypeError, match='lut_batch: a contiguous device'):
            L.lut_batch(*args)
    # dense host tensors pass the layout checks and are refused for where they live
    for call in (lambda: L.cutout_batch(hwc, yx, 2, (1, 2, 3)), lambda: L.flip_batch(hwc, ch.zeros_like(hwc), flips),
                 lambda: L.translate_batch(hwc, ch.zeros_like(hwc), yx, 1, (1, 2, 3)),
                 lambda: L.lut_batch(hwc, lut, out)):
        with pytest.raises(TypeError, match='must be in device memory'):
            call()
