"""Register and LDS budgets of the colour kernels (csrc/ffcv_color.hip), from
the compiler's own resource remarks of a device-only compile with the
library's flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  uniform_draw_kernel  (one lane per sample)            9 VGPRs, 8 waves/SIMD, no LDS
  color_jitter_kernel  (a workgroup per image / tile)  40 VGPRs, 8 waves/SIMD, 16,688 bytes of LDS

The jitter kernel's LDS is 16 KiB of pixels + 32 B staging slack, the 256-byte
table and 16 bytes of gray-sum partials: eight 256-thread workgroups (all 32
waves of a CU) share its 160 KiB, so LDS never limits occupancy.  Each kernel
is pinned to its counts, so that a change that costs registers, LDS or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import find, kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes per workgroup)
BUDGET = {
    'uniform_draw_kernel': (9, 8, 0),
    'color_jitter_kernel': (40, 8, 16688),
}
WORKGROUPS_PER_CU = 8
LDS_LIMIT = 160 * 1024 // WORKGROUPS_PER_CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_color.hip' in _build.SOURCES
    assert {'color_common.h', 'lds_stage.h'} <= set(_build.HEADERS)
    return kernel_usage('ffcv_color.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        find(usage, frag)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_resources(usage, frag):
    u = find(usage, frag)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds <= LDS_LIMIT
    assert WORKGROUPS_PER_CU * lds <= 160 * 1024   # eight workgroups per CU: LDS never limits occupancy
