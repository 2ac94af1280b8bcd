"""Register and LDS budgets of the tone kernels (csrc/ffcv_tone.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  tone_draw_kernel  (one lane per sample, up to 4 draws)   12 VGPRs, 8 waves/SIMD, no LDS
  tone_kernel       (a workgroup per image / tile)         40 VGPRs, 7 waves/SIMD, 21,168 bytes of LDS

The tone kernel's occupancy is set by its LDS: 16 KiB of pixels + 32 B staging
slack, 3 KiB of counters, two 768-byte tables and 144 bytes of scan partials
let seven 256-thread workgroups (28 of a CU's 32 waves) share its 160 KiB.
Each kernel is pinned to its counts, so that a change that costs registers,
LDS or occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import find, kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes per workgroup)
BUDGET = {
    'tone_draw_kernel': (12, 8, 0),
    'tone_kernel': (40, 7, 21168),
}
WORKGROUPS_PER_CU = 7
LDS_LIMIT = 160 * 1024 // WORKGROUPS_PER_CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_tone.hip' in _build.SOURCES and 'tone_common.h' in _build.HEADERS
    return kernel_usage('ffcv_tone.hip')


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
    if lds:   # seven workgroups per CU, not eight
        assert WORKGROUPS_PER_CU * lds <= 160 * 1024 < (WORKGROUPS_PER_CU + 1) * lds
