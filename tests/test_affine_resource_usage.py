"""Register budgets of the affine kernels (csrc/ffcv_affine.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  affine_draw_kernel  (one lane per sample, sin / cos / tan)  76 VGPRs, 6 waves/SIMD
  affine_warp_kernel  (a workgroup per tile)                   32 VGPRs, 8 waves/SIMD

(the draw kernel runs one lane per sample, a launch of a few waves whose
occupancy does not matter; the warp kernel stays within the 64 registers of
eight waves per SIMD, and its occupancy in a launch is bounded by its dynamic
LDS: eight workgroups per CU for a tile, four for the largest whole image).
Each kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'affine_draw_kernel': (76, 6),
    'affine_warp_kernel': (32, 8),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_affine.hip' in _build.SOURCES and 'affine_common.h' in _build.HEADERS
    return kernel_usage('ffcv_affine.hip')


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
