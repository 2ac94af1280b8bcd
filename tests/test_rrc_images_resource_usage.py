"""Register budgets of the RandomResizedCrop transform's kernels
(csrc/ffcv_rrc_images.hip), from the compiler's own resource remarks of a
device-only compile with the library's flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  crop_draw_kernel          (one lane per sample)       50 VGPRs, 8 waves/SIMD
  rrc_images_desc_kernel    (band regime front end)     20 VGPRs, 8 waves/SIMD
  rrc_images_kernel<false>  (u8, a workgroup per image) 80 VGPRs, 6 waves/SIMD
  rrc_images_kernel<true>   (fp16)                      84 VGPRs, 5 waves/SIMD

(the image kernel's occupancy in a launch is further bounded by its dynamic
LDS: the staged source, the taps and the LUT).  Each kernel is pinned to its
count, so that a change that costs registers or occupancy fails here; one
that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'crop_draw_kernel': (50, 8),
    'rrc_images_desc_kernel': (20, 8),
    'rrc_images_kernelILb0E': (80, 6),
    'rrc_images_kernelILb1E': (84, 5),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_rrc_images.hip' in _build.SOURCES
    return kernel_usage('ffcv_rrc_images.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in usage) == 1, (frag, sorted(usage))


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
