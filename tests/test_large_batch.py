"""The conditions of tests/large_batch.py that need no device, over every
parametrisation of tests/test_large_batch_gpu.py: the host twins compute each
period, and the harness checks that the tiling cannot hide a wrapped offset."""
import numpy as np
import pytest

from tests import large_batch as LB


@pytest.mark.parametrize('name,regime', sorted({(n, r) for n, r, _ in LB.DENSE}), ids=lambda v: str(v))
def test_period_cannot_hide_a_wrapped_offset(hip_lib, name, regime):
    b = LB.built(name, regime)
    LB.check_conditions(b)
    case = LB.BY_NAME[name]
    for lim in LB.LIMITS.values():
        batch = LB.batch_for(lim, case.size_of(b))
        assert batch % LB.M == 0 and batch * case.size_of(b) > lim >= (batch - LB.M) * case.size_of(b)
        assert batch * max(b.src_img, b.dst_img) + (0 if b.inplace else batch * min(b.src_img, b.dst_img)) < 13.5e9
    if regime == 'many':
        assert LB.batch_for(1 << 32, case.size_of(b)) > 65535      # more images than a grid has rows


def test_a_narrowed_offset_lands_inside_the_guarded_batch():
    """What a kernel whose image offset were kept in 32 bits would touch: for
    every image past 2^32 of the small shape, a byte inside the batch (so the
    run compares unequal instead of faulting) and inside another image."""
    img = LB.SMALL[0] * LB.SMALL[1] * 3
    batch = LB.batch_for(1 << 32, img)
    for k in range((1 << 32) // img + 1, batch):
        off, at, inside = LB.wrapped(k, img, 32)
        assert 0 <= off < (batch - 1) * img and inside != 0, (k, off)


@pytest.mark.parametrize('name,regime,limit', LB.DENSE, ids=lambda v: str(v))
def test_a_narrowed_offset_of_each_case_compares_unequal(hip_lib, name, regime, limit):
    """The injected-fault argument per case, on the case's own image sizes:
    were the product k * img kept in 32 bits, every image past 2^32 would be
    read or written 2^32 bytes early, which is inside the guarded batch (no
    fault) and 2^32 % img bytes off an image boundary, so across two images of
    the period whose expected bytes differ.  Kept in a signed 32 bits, the
    offsets from 2^31 on turn negative: at most 2^31 bytes in front of the
    buffer, outside the guards, so that form is not to be run on a device."""
    b, case = LB.built(name, regime), LB.BY_NAME[name]
    batch = LB.batch_for(LB.LIMITS[limit], case.size_of(b))
    for img, period in ((b.src_img, b.base), (b.dst_img, b.want)):
        assert (1 << 32) % img != 0 and (1 << 31) % img != 0
        first = (1 << 32) // img + 1
        for k in (first, (first + batch) // 2, batch - 1):
            if k * img < 1 << 32:
                continue                                   # this batch stays below 2^32: the 2^31 argument only
            off, at, inside = LB.wrapped(k, img, 32)
            assert inside != 0 and off + img <= batch * img     # (a 2-byte output past 2^33 wraps twice)
            # the bytes found there: the tail of image `at` and the head of image `at + 1`
            there = np.concatenate([period[at % LB.M, inside:], period[(at + 1) % LB.M, :inside]])
            assert not np.array_equal(there, period[k % LB.M]), (k, at)
        k = (1 << 31) // img + 1
        assert k * img - (1 << 32) < 0                     # the signed form: in front of the buffer


@pytest.mark.parametrize('name,regime', LB.STRIDED, ids=lambda v: str(v))
def test_a_narrowed_stride_product_compares_unequal(hip_lib, name, regime):
    """k * 64 MiB kept in 32 bits sends image k >= 64 to the slot of image
    k - 64: that slot then holds another image's bytes, and slot k its fill."""
    b = LB.built(name, regime)
    for k in range(64, LB.STRIDE_BATCH):
        assert (k * LB.STRIDE_BYTES) % (1 << 32) == (k - 64) * LB.STRIDE_BYTES
        assert not np.array_equal(b.want[k], b.want[k - 64])
