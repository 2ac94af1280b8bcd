"""Register budgets of the hue kernels (csrc/ffcv_hue.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  hue_draw_kernel                 (one lane per sample)            9 VGPRs, 8 waves/SIMD
  color_jitter_joint_draw_kernel  (one lane per sample, 5 draws)  18 VGPRs, 8 waves/SIMD
  hue_kernel                      (a workgroup per image / tile)  14 VGPRs, 8 waves/SIMD

(the hue kernel's 16,416 bytes of static LDS let eight 256-thread workgroups,
all 32 waves of a CU, share its 160 KiB).  Each kernel is pinned to its count,
so that a change that costs registers or occupancy fails here; one that saves
some lowers the bound.
"""
import pytest

from tests.resource_usage import find, kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'hue_draw_kernel': (9, 8),
    'color_jitter_joint_draw_kernel': (18, 8),
    'hue_kernel': (14, 8),
}
LDS_LIMIT = 160 * 1024 // 8   # eight workgroups per CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_hue.hip' in _build.SOURCES and 'hue_common.h' in _build.HEADERS
    return kernel_usage('ffcv_hue.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        find(usage, frag)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = find(usage, frag)
    print(frag, u)
    vgprs, occupancy = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= LDS_LIMIT
