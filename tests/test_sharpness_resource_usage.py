"""Register budgets of the sharpness kernels (csrc/ffcv_sharpness.hip), from
the compiler's own resource remarks of a device-only compile with the
library's flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  sharpness_draw_kernel  (one lane per sample)       8 VGPRs, 8 waves/SIMD, no LDS
  sharpness_kernel       (a workgroup per tile)      42 VGPRs, 8 waves/SIMD, dynamic LDS only

(the pixel kernel holds three rows of ten products, thirty float32 values, and
stays within the 64 registers of eight waves per SIMD; its LDS is all dynamic,
at most 25,600 bytes a workgroup, which the plan of the launch decides: six
workgroups per CU at the largest tile, eight for a 32 x 32 image).  Each
kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, static LDS bytes)
BUDGET = {
    'sharpness_draw_kernel': (8, 8, 0),
    'sharpness_kernel': (42, 8, 0),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_sharpness.hip' in _build.SOURCES and 'sharpness_common.h' in _build.HEADERS
    return kernel_usage('ffcv_sharpness.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in usage) == 1, (frag, sorted(usage))


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds
