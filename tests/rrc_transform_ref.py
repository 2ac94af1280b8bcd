"""What the RandomResizedCrop transform must give, from the oracle alone
(shared by test_rrc_transform.py and test_rrc_transform_gpu.py): the window is
the oracle's get_random_crop on the sample's MT19937 with op id 8, the pixels
are the oracle's resize_crop (rrc_batch for a batch), and flip / cutout / LUT
follow as numpy statements (tests/translate_ref.py)."""
import numpy as np

from tests.resize_ref import kind_of
from tests.translate_ref import apply_steps, cutout_draw, flip_draw

OP_ID = 8
SAMPLE_OK, SAMPLE_RANGE = 0, 8
DEFAULT_SCALE, DEFAULT_RATIO = (0.08, 1.0), (0.75, 4 / 3)


def crop_draw(oracle, seed, epoch, sid, H, W, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, op_id=OP_ID):
    return oracle.MT(oracle.sample_seed(int(seed), int(epoch), int(sid), op_id)).random_crop(H, W, scale, ratio)


def crop_valid(c, H, W):
    i, j, h, w = (int(x) for x in c)
    return h > 0 and w > 0 and i >= 0 and j >= 0 and i + h <= H and j + w <= W


def expected_resize(oracle, imgs, crops, out_h, out_w):
    """(images uint8 (B, out_h, out_w, 3), status int32 (B,)): the oracle's
    crop-resize of every image; an invalid crop gives zeros and status 8."""
    B = len(imgs)
    out = np.zeros((B, out_h, out_w, 3), np.uint8)
    status = np.zeros(B, np.int32)
    for k in range(B):
        i, j, h, w = (int(x) for x in crops[k])
        H, W = imgs[k].shape[:2]
        if not crop_valid(crops[k], H, W):
            status[k] = SAMPLE_RANGE
            continue
        out[k] = oracle.resize_crop(imgs[k], i, i + h, j, j + w, out_h, out_w)
    return out, status


def expected_epilogue(u8, flips=None, cyx=None, cut=0, fill=(0, 0, 0), cut_before_flip=False, lut=None,
                      status=None):
    """flip / cutout in the given order on the resized batch, then lut[u8]
    (float16 (256, 3)); rows with a nonzero status stay zero."""
    out = np.array(u8)
    chain = ('cf' if cut_before_flip else 'fc') if cut else 'f'
    for k in range(len(out)):
        if status is not None and status[k]:
            continue
        out[k] = apply_steps(out[k], chain, bool(flips[k]) if flips is not None else False,
                             None, cyx[k] if cut else None, cut=cut, cfill=fill)
    if lut is None:
        return out
    res = np.stack([lut[out[..., c], c] for c in range(3)], -1)
    if status is not None:
        res[np.asarray(status) != 0] = 0
    return res


def expected_transform(oracle, img, seed, epoch, sid, size, scale=DEFAULT_SCALE, ratio=DEFAULT_RATIO, chain='',
                       cut=0, fill=(0, 0, 0), flip_p=0.5):
    """One sample through RandomResizedCrop(scale, ratio, size) and then the
    operations of chain ('f' RandomHorizontalFlip, 'c' Cutout) with the
    contract's draws."""
    H, W = img.shape[:2]
    i, j, h, w = crop_draw(oracle, seed, epoch, sid, H, W, scale, ratio)
    out = oracle.resize_crop(img, i, i + h, j, j + w, size, size)
    flip = flip_draw(seed, epoch, sid, flip_p) if 'f' in chain else False
    cyx = cutout_draw(seed, epoch, sid, size, size, cut) if 'c' in chain else None
    return apply_steps(out, chain, flip, None, cyx, cut=cut, cfill=fill)


def forced_crops(H, W, n, seed=0):
    """n crop windows (i, j, h, w) of an H x W source: the full image, the
    special windows (1 x 1 at both corners, one row, one column, the
    bottom-right corner), windows of the sizes that make copies and integer
    scales of the tested outputs, a tall-narrow and a wide-short window, then
    random ones.  All valid."""
    rng = np.random.default_rng(seed)
    c = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (H // 2, 0, 1, W), (0, W // 3, H, 1),
         (H - (H + 1) // 2, W - (W + 1) // 2, (H + 1) // 2, (W + 1) // 2)]
    for s in (24, 30, 32, 33, 40, 48, 60, 64, 66, 96, 120):
        if s <= H and s <= W:
            c.append((int(rng.integers(0, H - s + 1)), int(rng.integers(0, W - s + 1)), s, s))
    for h, w in ((20, 50), (50, 20), (48, 40), (24, 40), (48, 80), (31, 17)):
        if h <= H and w <= W:
            c.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    while len(c) < n:
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        c.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w))
    return np.array(c[:n], np.int32)


def every_size_crops(H, W, seed=0):
    """One window of every size (h, w) of an H x W source (the taps depend on
    the size alone), each at a random origin (which moves the alignment)."""
    rng = np.random.default_rng(seed)
    return np.array([(int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w)
                     for h in range(1, H + 1) for w in range(1, W + 1)], np.int32)


def kinds(crops, out_h, out_w):
    return {kind_of(int(h), int(w), out_h, out_w) for _, _, h, w in crops}


def invalid_crops(H, W):
    """One window for each way of being invalid."""
    return np.array([(0, 0, 0, W), (0, 0, H, 0), (0, 0, -3, 5), (0, 0, 5, -3), (-1, 0, 4, 4), (0, -1, 4, 4),
                     (H - 3, 0, 4, 4), (0, W - 3, 4, 4), (0, 0, H + 1, W), (0, 0, H, W + 1),
                     (2 ** 31 - 2, 0, 4, 4), (0, 2 ** 31 - 2, 4, 4)], np.int32)


def natural_batch(n, H, W, seed=0):
    from ffcv_amd.synthetic import natural_image
    rng = np.random.default_rng(seed)
    return np.stack([natural_image(rng, H, W) for _ in range(n)])
