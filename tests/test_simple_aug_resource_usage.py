"""Register and LDS budgets of the fused small-image augmentation
(csrc/ffcv_simple_aug.hip), from the compiler's own resource remarks of a
device-only compile with the library's flags (no GPU needed).

Both instantiations run at eight waves per SIMD without scratch or spills;
their static LDS is the 16 KB stage plus two chunks (the range's lead bytes
and the pixel read-ahead) and, for fp16, the LUT.  As written the compiler
reports, for gfx950:

  simple_aug_kernel<false>  (u8)    16 VGPRs, 16416 bytes of LDS
  simple_aug_kernel<true>   (fp16)  14 VGPRs, 17952 bytes of LDS

Each kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes)
BUDGET = {
    'simple_aug_kernelILb0E': (16, 8, 16416),
    'simple_aug_kernelILb1E': (14, 8, 17952),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_simple_aug.hip' in _build.SOURCES
    return kernel_usage('ffcv_simple_aug.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in usage) == 1, (frag, sorted(usage))


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_pinned_registers_and_lds(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] == occupancy
    assert u['LDS Size [bytes/block]'] == lds
