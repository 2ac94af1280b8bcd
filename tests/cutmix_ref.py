"""The CutMix semantics stated in numpy, independent of the package.  Shared by
test_cutmix.py (CPU) and test_cutmix_gpu.py.

For one batch of n samples of height H and width W with last dataset index
``last``::

    rs = np.random.RandomState(int(last))
    same_lambda:   lam = rs.beta(alpha, alpha);    cy = rs.randint(0, H);    cx = rs.randint(0, W)
    otherwise:     lam = rs.beta(alpha, alpha, n); cy = rs.randint(0, H, n); cx = rs.randint(0, W, n)
    r  = 0.5 * np.sqrt(1.0 - lam)                        # float64
    rh = floor(r * H); rw = floor(r * W)                 # float64 product, then floor
    y1 = max(cy - rh, 0); y2 = min(cy + rh, H); x1 = max(cx - rw, 0); x2 = min(cx + rw, W)
    out[i] = in[i];  out[i][y1:y2, x1:x2, :] = in[i-1][y1:y2, x1:x2, :]      # i = 0: the batch's last sample
    lam_adj = 1.0 - ((y2 - y1) * (x2 - x1)) / float64(H * W)                 # float64, stored as float32
    label row i = [label_i, label_{i-1}, lam_adj_i]                          # float32 (n, 3)

The draws come in the order beta, rows, columns.  The Mixup/CutMix switch
draws ``u = rs.random_sample()`` first on the same stream; ``u < switch_prob``
chooses CutMix with ``cutmix_alpha``, else Mixup with
``rs.beta(mixup_alpha, mixup_alpha[, n])``."""
import numpy as np

from tests.mixup_ref import mix_one_batch, segments


def boxes_from(rs, alpha, same_lambda, n, H, W):
    """One batch's draws on the stream rs: int64 (n, 4) boxes of
    (y1, x1, y2, x2) and float64 (n,) adjusted lambdas."""
    if same_lambda:
        lam = rs.beta(alpha, alpha)
        cy = rs.randint(0, H)
        cx = rs.randint(0, W)
    else:
        lam = rs.beta(alpha, alpha, n)
        cy = rs.randint(0, H, n)
        cx = rs.randint(0, W, n)
    lam = np.broadcast_to(np.asarray(lam, np.float64), (n,))
    cy = np.broadcast_to(np.asarray(cy, np.int64), (n,))
    cx = np.broadcast_to(np.asarray(cx, np.int64), (n,))
    r = 0.5 * np.sqrt(1.0 - lam)
    rh = np.floor(r * H).astype(np.int64)
    rw = np.floor(r * W).astype(np.int64)
    y1, y2 = np.maximum(cy - rh, 0), np.minimum(cy + rh, H)
    x1, x2 = np.maximum(cx - rw, 0), np.minimum(cx + rw, W)
    lam_adj = 1.0 - ((y2 - y1) * (x2 - x1)) / np.float64(H * W)
    return np.stack([y1, x1, y2, x2], 1), lam_adj


def draw_boxes(last_index, alpha, same_lambda, n, H, W):
    return boxes_from(np.random.RandomState(int(last_index)), alpha, same_lambda, n, H, W)


def cut_one_batch(images, boxes):
    """images (B, H, W, ...) of any dtype, boxes (B, 4) or (4,): python slices,
    so a box has to lie inside the image (see clamp)."""
    images = np.asarray(images)
    B = images.shape[0]
    boxes = np.broadcast_to(np.asarray(boxes, np.int64).reshape(-1, 4), (B, 4))
    out = images.copy()
    for i in range(B):
        y1, x1, y2, x2 = (int(v) for v in boxes[i])
        out[i][y1:y2, x1:x2] = images[i - 1][y1:y2, x1:x2]    # i = 0: the batch's last sample
    return out


def clamp(boxes, H, W):
    """What the kernel does to a box before use: every bound into the image."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4).copy()
    b[:, 0::2] = np.clip(b[:, 0::2], 0, H)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, W)
    return b


def cut_segments(images, boxes, batch_size, same_box):
    """A launch of several batches with given (clamped here) boxes, one per
    batch when same_box, else one per sample."""
    images = np.asarray(images)
    boxes = clamp(boxes, images.shape[1], images.shape[2])
    out = np.empty_like(images)
    for s, (lo, hi) in enumerate(segments(len(images), batch_size)):
        out[lo:hi] = cut_one_batch(images[lo:hi], boxes[s] if same_box else boxes[lo:hi])
    return out


def image_cutmix(images, indices, alpha, same_lambda, batch_size=None):
    """ImageCutMix of a launch of (n, H, W, ...) images: batches of batch_size
    (default: one batch), each drawn from its own last index."""
    images = np.asarray(images)
    n, H, W = images.shape[:3]
    out = np.empty_like(images)
    for lo, hi in segments(n, batch_size or n):
        out[lo:hi] = cut_one_batch(images[lo:hi], draw_boxes(indices[hi - 1], alpha, same_lambda, hi - lo, H, W)[0])
    return out


def label_cutmix(labels, indices, alpha, same_lambda, image_size, batch_size=None):
    """float32 (n, 3): [label_i, label_{i-1}, lam_adj_i] per batch."""
    labels = np.asarray(labels).reshape(len(indices), -1)[:, 0]
    n = len(labels)
    out = np.empty((n, 3), np.float32)
    for lo, hi in segments(n, batch_size or n):
        seg = labels[lo:hi]
        out[lo:hi, 0] = seg
        out[lo:hi, 1] = np.roll(seg, 1)
        out[lo:hi, 2] = draw_boxes(indices[hi - 1], alpha, same_lambda, hi - lo, *image_size)[1]
    return out


def switch_batch(images, labels, last_index, mixup_alpha, cutmix_alpha, switch_prob, same_lambda):
    """One batch of the Mixup/CutMix switch: (images, float32 (n, 3) label
    rows, True when CutMix was chosen)."""
    images = np.asarray(images)
    n, H, W = images.shape[:3]
    labels = np.asarray(labels).reshape(n, -1)[:, 0]
    rs = np.random.RandomState(int(last_index))
    u = rs.random_sample()
    rows = np.empty((n, 3), np.float32)
    rows[:, 0] = labels
    rows[:, 1] = np.roll(labels, 1)
    if u < switch_prob:
        boxes, lam_adj = boxes_from(rs, cutmix_alpha, same_lambda, n, H, W)
        rows[:, 2] = lam_adj
        return cut_one_batch(images, boxes), rows, True
    lam = rs.beta(mixup_alpha, mixup_alpha) if same_lambda else rs.beta(mixup_alpha, mixup_alpha, n)
    rows[:, 2] = lam
    return mix_one_batch(images, lam), rows, False


def switch_launch(images, labels, indices, mixup_alpha, cutmix_alpha, switch_prob, same_lambda, batch_size=None):
    """The switch over a launch: (images, label rows, [choice per batch])."""
    images = np.asarray(images)
    n = len(images)
    out = np.empty_like(images)
    rows = np.empty((n, 3), np.float32)
    picks = []
    for lo, hi in segments(n, batch_size or n):
        out[lo:hi], rows[lo:hi], cut = switch_batch(images[lo:hi], np.asarray(labels)[lo:hi], indices[hi - 1],
                                                    mixup_alpha, cutmix_alpha, switch_prob, same_lambda)
        picks.append(cut)
    return out, rows, picks


# ---- the shape / box cases shared by the CPU and the GPU tests ----
SIZES = ((1, 1), (1, 17), (5, 6), (9, 7), (32, 32), (33, 47))      # (H, W): row bytes around and off multiples of 16
ITEMSIZES = (1, 2, 4, 8)
FORMS = (('hwc', 1), ('hwc', 3), ('chw', 3))                       # (layout, channels)
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def random_images(rng, n, H, W, layout, C, itemsize):
    """Random bytes as (n, H, W, C) or planar (n, C, H, W) of an unsigned dtype of itemsize."""
    shape = (n, H, W, C) if layout == 'hwc' else (n, C, H, W)
    raw = rng.integers(0, 256, (int(np.prod(shape)) * itemsize,), dtype=np.uint8)
    return raw.view(DTYPES[itemsize]).reshape(shape)


def as_hwc(x, layout):
    """(n, H, W, C) view of either form, for the reference."""
    return x if layout == 'hwc' else x.transpose(0, 2, 3, 1)


def from_hwc(x, layout):
    return x if layout == 'hwc' else np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def random_boxes(rng, m, H, W):
    """m boxes drawn like CutMix's (alpha 1), every third replaced by an edge
    case: empty, full, out of range on every side, inverted."""
    lam = rng.beta(1.0, 1.0, m)
    cy, cx = rng.integers(0, H, m), rng.integers(0, W, m)
    r = 0.5 * np.sqrt(1.0 - lam)
    rh, rw = np.floor(r * H).astype(np.int64), np.floor(r * W).astype(np.int64)
    b = np.stack([np.maximum(cy - rh, 0), np.maximum(cx - rw, 0), np.minimum(cy + rh, H), np.minimum(cx + rw, W)], 1)
    special = [(0, 0, 0, 0), (0, 0, H, W), (-3, -2, H + 5, W + 1), (H, W, 0, 0)]
    for j in range(0, m, 3):
        b[j] = special[(j // 3) % len(special)]
    return b.astype(np.int32)


def hand_boxes(H, W):
    """The hand-made boxes: empty, full image, one pixel in each corner, one
    full row, one full column, out of range on every side, and (the sweep) x1
    over 0..W with x2 = W and with x2 = x1 + 1."""
    b = [(0, 0, 0, 0), (2, 3, 2, 9), (0, 0, H, W), (0, 0, 1, 1), (0, W - 1, 1, W), (H - 1, 0, H, 1),
         (H - 1, W - 1, H, W), (H // 2, 0, H // 2 + 1, W), (0, W // 2, H, W // 2 + 1),
         (-7, -9, H + 7, W + 9), (-2**31, -2**31, 2**31 - 1, 2**31 - 1), (H + 1, W + 1, H + 9, W + 9)]
    b += [(1, x1, H - 1, W) for x1 in range(W + 1)]
    b += [(0, x1, H, x1 + 1) for x1 in range(W + 1)]
    return np.array(b, np.int64).astype(np.int32)
