"""Per-sample seeding contract shared by the host paths of the transforms.

Each stochastic operation ``op`` applied to dataset sample ``s`` in epoch
``e`` of a Loader seeded with ``seed`` owns a fresh MT19937 seeded with
``low32(splitmix64(splitmix64(splitmix64(seed ^ op<<56) ^ e) ^ s))``;
op ids: 1 crop (the crop decoders), 2 cutout, 3 flip, 4 translate,
5 brightness, 6 contrast, 7 saturation, 8 crop transform (RandomResizedCrop:
its own id, so that a pipeline with a crop decoder and the transform does not
draw the same stream twice), 9 grayscale, 10 solarization, 11 blur, 12 hue,
13 joint colour jitter (RandomColorJitter: five draws from one stream),
14 affine (RandomAffine and RandomRotation: seven draws from one stream),
15 posterize, 16 autocontrast, 17 equalize, 18 invert, 19 sharpness
(RandomAdjustSharpness) (one draw each), 20 policy (TrivialAugmentWide: three
draws from one stream), 21 erase (RandomErasing: apply, then up to ten tries of
area and aspect ratio, then the box's origin), 22 erase noise (no MT19937: the
full 64-bit hash is the sample's key into RandomErasing's per-pixel noise,
transforms/erase.py), 23 rand augment (RandAugment: two draws per operation
slot from one stream).  The device kernels use the same function
(csrc/device_common.h sample_seed).  The reference itself draws from numba's
per-thread generators seeded from OS entropy (nondeterministic); see
DESIGN.md "RNG contract".
"""
M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def contract_seed(loader_seed, epoch, sample, op_id):
    h = splitmix64((int(loader_seed) & M64) ^ ((int(op_id) << 56) & M64))
    h = splitmix64(h ^ (int(epoch) & M64))
    h = splitmix64(h ^ (int(sample) & M64))
    return h & 0xFFFFFFFF
