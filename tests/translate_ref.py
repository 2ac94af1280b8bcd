"""numpy statement of flip / translate / cutout under the seeding contract,
shared by test_translate.py and test_translate_gpu.py.  Translate is written
the reference's way (a filled canvas with the image at offset p, then the
window at (y, x)), not the way the package's host path or kernels compute it."""
import numpy as np

from ffcv_amd.transforms.rng import contract_seed


def translate_np(img, y, x, p, fill):
    h, w = img.shape[:2]
    canvas = np.empty((h + 2 * p, w + 2 * p, 3), np.uint8)
    canvas[:] = np.asarray(fill, np.uint8)
    canvas[p:p + h, p:p + w] = img
    return canvas[y:y + h, x:x + w].copy()


def translate_draw(seed, epoch, sid, p):
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), 4))
    y = rs.randint(2 * p + 1)
    x = rs.randint(2 * p + 1)
    return int(y), int(x)


def flip_draw(seed, epoch, sid, prob):
    return bool(np.random.RandomState(contract_seed(seed, epoch, int(sid), 3)).uniform(0, 1) < prob)


def cutout_draw(seed, epoch, sid, h, w, c):
    rs = np.random.RandomState(contract_seed(seed, epoch, int(sid), 2))
    y = rs.randint(h - c + 1)
    x = rs.randint(w - c + 1)
    return int(y), int(x)


def apply_steps(img, chain, flip, tyx, cyx, pad=0, tfill=(0, 0, 0), cut=0, cfill=(0, 0, 0)):
    """The operations of chain (a string of 'f' flip, 't' translate, 'c'
    cutout, in pipeline order) with the given decisions, one after another."""
    out = np.array(img, np.uint8)
    for s in chain:
        if s == 'f':
            if flip:
                out = out[:, ::-1].copy()
        elif s == 't':
            out = translate_np(out, int(tyx[0]), int(tyx[1]), pad, tfill)
        elif s == 'c':
            y, x = int(cyx[0]), int(cyx[1])
            out[y:y + cut, x:x + cut] = np.asarray(cfill, np.uint8)
        else:
            raise ValueError(s)
    return out


def apply_chain(img, chain, seed, epoch, sid, pad=0, tfill=(0, 0, 0), cut=0, cfill=(0, 0, 0), flip_p=0.5):
    """apply_steps with the contract's draws for sample sid.  Returns (image, flipped)."""
    h, w = np.asarray(img).shape[:2]
    flip = flip_draw(seed, epoch, sid, flip_p) if 'f' in chain else False
    tyx = translate_draw(seed, epoch, sid, pad) if 't' in chain else None
    cyx = cutout_draw(seed, epoch, sid, h, w, cut) if 'c' in chain else None
    return apply_steps(img, chain, flip, tyx, cyx, pad, tfill, cut, cfill), flip
