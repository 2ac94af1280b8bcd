"""Register and LDS budget of RandAugment's kernel for images up to 224 x 224
(csrc/ffcv_randaugment_large.hip), in the form of
test_randaugment_resource_usage.py: no scratch, no spills, and the compiler's
figures for the code as written, for gfx950:

  randaugment_large_kernel<1024 threads, 150,528 B>  114 VGPRs, 4 waves/SIMD, 154,720 B LDS

It holds a 224 x 224 image and is alone on a CU: its 16 waves are four per
SIMD, so it may use 128 VGPRs.  A thread's 39 warp dwords or 37 stencil dwords
are indexed by constants only, so none of them is in scratch.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes, workgroups per CU)
BUDGET = {
    'RalTierILi1024ELi150528EE': (114, 4, 154720, 1),
}
LDS_PER_CU = 163840


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_randaugment_large.hip' in _build.SOURCES
    return kernel_usage('ffcv_randaugment_large.hip')


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    assert len(usage) == len(BUDGET) and all('24randaugment_large_kernel' in k for k in usage), sorted(usage)
    (u,) = [v for k, v in usage.items() if frag in k]
    print(frag, u)
    vgprs, occupancy, lds, per_cu = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds and per_cu * lds <= LDS_PER_CU
