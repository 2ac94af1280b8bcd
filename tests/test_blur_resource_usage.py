"""Register budgets of the blur kernels (csrc/ffcv_blur.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  blur_draw_kernel      (one lane per sample, k exps)   42 VGPRs, 8 waves/SIMD
  gaussian_blur_kernel  (a workgroup per tile)          62 VGPRs, 8 waves/SIMD

(the blur kernel holds twelve float32 accumulators, four adjacent outputs of
three channels, and stays within the 64 registers of eight waves per SIMD; its
occupancy in a launch is bounded by its dynamic LDS: four workgroups per CU at
the largest tile, eight for a 32 x 32 image).  Each kernel
is pinned to its count, so that a change that costs registers or occupancy
fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'blur_draw_kernel': (42, 8),
    'gaussian_blur_kernel': (62, 8),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_blur.hip' in _build.SOURCES and 'blur_common.h' in _build.HEADERS
    return kernel_usage('ffcv_blur.hip')


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
