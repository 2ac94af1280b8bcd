"""One device Loader through every family of transforms at once, bit for bit
against the numpy statements applied one after another with the contract's
draws: [SimpleRGBImageDecoder, RandomBrightness, RandomSaturation, RandomHue,
GaussianBlur, RandomAffine, RandomPosterize, RandomInvert,
RandomHorizontalFlip, Cutout, ToTensor, ToDevice, ToTorchImage,
NormalizeImage(float32)] on 32 x 32 raw samples.

The colour operations end the decoder's fused prefix, so the standalone flip,
cutout and table-lookup kernels run behind the five transform launches
(brightness + saturation, hue, blur, affine, posterize + invert), all on one
stream.  What no per-family test sees: the draw streams of nine op ids live
together, the slot buffers of in-place and out-of-place operations across
batches in flight, and the order of the launches on the stream."""
import os
import tempfile

import numpy as np
import pytest
import torch as ch

from ffcv_amd.loader import Loader
from ffcv_amd.fields import RGBImageField, IntField
from ffcv_amd.fields.decoders import SimpleRGBImageDecoder, IntDecoder
from ffcv_amd.transforms import (ToTensor, ToDevice, ToTorchImage, NormalizeImage, Cutout, RandomHorizontalFlip,
                                 RandomBrightness, RandomSaturation, RandomHue, GaussianBlur, RandomAffine,
                                 RandomPosterize, RandomInvert)
from ffcv_amd.transforms.lut import make_lut
from tests import affine_ref as AR
from tests import blur_ref as BR
from tests import color_jitter_ref as CR
from tests import hue_ref as HR
from tests import tone_ref as TR
from tests.helpers import NaturalDS, write
from tests.standalone_ref import cutout_np, flip_np, lut_np
from tests.translate_ref import cutout_draw, flip_draw

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, HW, BATCH, EPOCHS = 48, (32, 32), 16, 2
SEED = 7                                  # chosen on the CPU: both guards hold, some samples flip (asserted below)
MEAN = np.array([125.307, 122.961, 113.8575])
STD = np.array([51.5865, 50.847, 51.255])
AFFINE = AR.CONFIGS[0]
AFFINE_P, AFFINE_FILL = 0.8, (11, 12, 13)
BRIGHT, SAT, HUE = (0.4, 0.6), (0.5, 0.5), (0.1, 0.5)          # (magnitude, p)
KSIZE, SIGMA, BLUR_P = 5, (0.1, 2.0), 0.5
BITS, POSTER_P, INVERT_P = 3, 0.5, 0.3
FLIP_P, CUT, CUT_FILL = 0.5, 8, (200, 201, 202)


def chain():
    return [SimpleRGBImageDecoder(), RandomBrightness(*BRIGHT), RandomSaturation(*SAT), RandomHue(*HUE),
            GaussianBlur(KSIZE, SIGMA, BLUR_P), RandomAffine(fill=AFFINE_FILL, p=AFFINE_P, **AFFINE),
            RandomPosterize(BITS, POSTER_P), RandomInvert(INVERT_P), RandomHorizontalFlip(FLIP_P),
            Cutout(CUT, CUT_FILL)]


def expected_u8(img, seed, epoch, sid):
    """One sample through the statements of the nine operations, in pipeline
    order, each with its own draw; returns (image, which operations applied)."""
    H, W = img.shape[:2]
    out = np.array(img, np.uint8)
    did = {}
    for kind, (mag, p), name in ((CR.BRIGHTNESS, BRIGHT, 'brightness'), (CR.SATURATION, SAT, 'saturation')):
        did[name], ratio = CR.jitter_draw(seed, epoch, sid, kind, p, mag)
        if did[name]:
            out = CR.jitter_np(out, kind, ratio)
    did['hue'], d = HR.hue_draw(seed, epoch, sid, HUE[1], HUE[0])
    if did['hue']:
        out = HR.hue_np(out, d)
    did['blur'], sigma = BR.uniform_draw(seed, epoch, sid, BR.OP_BLUR, BLUR_P, *SIGMA)
    assert BR.guard_holds(KSIZE, sigma), (seed, epoch, sid)
    if did['blur']:
        out = BR.blur(out, KSIZE, BR.weights_f32(KSIZE, sigma))
    out, did['affine'] = AR.expected(out, seed, epoch, sid, AR.BILINEAR, fill=AFFINE_FILL, p=AFFINE_P, **AFFINE)
    for kind, p, name in ((TR.POSTERIZE, POSTER_P, 'posterize'), (TR.INVERT, INVERT_P, 'invert')):
        did[name] = TR.draw(seed, epoch, sid, kind, p)
        if did[name]:
            out = TR.step_np(out, kind, BITS)
    did['flip'] = flip_draw(seed, epoch, sid, FLIP_P)
    out = flip_np(out, did['flip'])
    y, x = cutout_draw(seed, epoch, sid, H, W, CUT)
    return cutout_np(out, y, x, CUT, CUT_FILL), did


def expected_epochs(imgs, seed=SEED, epochs=EPOCHS):
    """Per epoch: uint8 (n, H, W, 3) and the per-sample decisions."""
    out = []
    for epoch in range(epochs):
        pairs = [expected_u8(im, seed, epoch, sid) for sid, im in enumerate(imgs)]
        out.append((np.stack([p[0] for p in pairs]), [p[1] for p in pairs]))
    return out


@pytest.fixture(scope='module', autouse=True)
def need_gpu(hip_lib):
    if not ch.cuda.is_available():
        pytest.skip('no HIP device')


@pytest.fixture(scope='module')
def data():
    """The .betons of 48 and of 43 natural images (the same first 43), and the
    expectation of both epochs, computed once."""
    d = tempfile.mkdtemp()
    ds = NaturalDS(N, hw=HW, seed=4)
    short = NaturalDS(43, hw=HW, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip(ds.imgs, short.imgs))
    fields = lambda: {'image': RGBImageField(write_mode='raw'), 'label': IntField()}  # noqa: E731
    fns = {N: write(os.path.join(d, 'chain48.beton'), ds, fields()),
           43: write(os.path.join(d, 'chain43.beton'), short, fields())}
    want = expected_epochs(ds.imgs)                 # asserts the affine and the blur guard for every sample and epoch
    for n in (N, 43):
        for u8, did in want:
            assert 1 <= sum(x['flip'] for x in did[:n]) <= n - 1
            for name in did[0]:                     # every operation applied to some samples and left others alone
                assert 1 <= sum(x[name] for x in did[:n]) <= n - 1, name
    assert not np.array_equal(want[0][0], want[1][0])
    return fns, want


def _loader(fn, **kw):
    return Loader(fn, batch_size=BATCH, seed=SEED, drop_last=False, pipelines={
        'image': chain() + [ToTensor(), ToDevice(DEV), ToTorchImage(), NormalizeImage(MEAN, STD, np.float32)],
        'label': [IntDecoder(), ToTensor(), ToDevice(DEV)]}, **kw)


@pytest.mark.parametrize('case', ('one_batch_per_launch', 'launch_groups', 'short_last_batch'))
def test_chain_through_every_family(data, case):
    fns, want = data
    n = 43 if case == 'short_last_batch' else N
    loader = _loader(fns[n], **(dict(batches_per_launch=1) if case == 'one_batch_per_launch' else {}))
    ops = {type(node.operation).__name__: node.operation for node in loader.graph.exec_nodes}
    assert loader.graph.groupable() and '_ToHost' not in ops
    absorbed = sorted(name for name, op in ops.items() if getattr(op, '_absorbed', False))
    assert absorbed == ['RandomInvert', 'RandomSaturation']       # the second of a colour run and of a tone run
    assert not loader.pipeline_specs['image'].decoder.fused       # flip, cutout and the table run their own kernels
    table = make_lut(MEAN, STD, np.float32)
    for epoch in range(EPOCHS):
        batches = [(im, lab) for im, lab in loader]
        assert [len(lab) for _, lab in batches] == [BATCH] * (n // BATCH) + ([n % BATCH] if n % BATCH else [])
        for im, _ in batches:
            assert im.dtype == ch.float32 and im.shape[1:] == (3,) + HW
            assert im.is_contiguous(memory_format=ch.channels_last)
        got = np.concatenate([im.permute(0, 2, 3, 1).cpu().numpy() for im, _ in batches])
        labels = np.concatenate([lab.cpu().numpy().reshape(-1) for _, lab in batches])
        assert np.array_equal(labels, np.arange(n) % 10)
        u8 = want[epoch][0][:n]
        want_f32 = lut_np(u8.reshape(-1), table).reshape(u8.shape)
        bad = [k for k in range(n) if not np.array_equal(got[k].view(np.uint32), want_f32[k].view(np.uint32))]
        assert not bad, (case, epoch, bad[:8], [want[epoch][1][k] for k in bad[:3]])
