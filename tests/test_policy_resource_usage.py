"""Register budget of the policy draw kernel (csrc/ffcv_policy.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

The kernel must run without scratch and without VGPR or SGPR spills.  As
written the compiler reports, for gfx950:

  policy_draw_kernel  (one lane per sample)   66 VGPRs, 7 waves/SIMD, no LDS

(the MT19937 draws, one float64 affine matrix with its five trigonometric
calls, and nine output pointers; a launch is one 64-lane workgroup per 64
samples, so its occupancy is never the limit).  The kernel is pinned to its
count, so that a change that costs registers or occupancy fails here; one that
saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes)
BUDGET = {
    'policy_draw_kernel': (66, 7, 0),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_policy.hip' in _build.SOURCES
    return kernel_usage('ffcv_policy.hip')


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
