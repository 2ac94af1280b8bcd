"""Register and LDS budget of the AugMix kernels (csrc/ffcv_augmix.hip), in the
form of test_randaugment_resource_usage.py: no scratch, no spills, and the
compiler's figures for the code as written.  The fused kernel's LDS stays
under 53 KB: three workgroups per CU, which its 167 VGPRs (at most 170) allow.
The weight kernels (one per gamma branch) reach MT19937's words 227 .. 623
through inlined loops: a call of the out-of-line recursion of device_common.h
costs scratch and scalar registers saved around it.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes)
BUDGET = {
    'augmix_draw_kernel': (174, 2, 0),
    'augmix_kernel': (167, 3, 41040),
    'augmix_mix_kernel': (50, 8, 0),
    'augmix_weight_kernelILi0EE': (53, 8, 0),
    'augmix_weight_kernelILi1EE': (116, 4, 0),
    'augmix_weight_kernelILi2EE': (78, 6, 0),
}
LDS_LIMIT = 53 * 1024   # three workgroups per CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_augmix.hip' in _build.SOURCES and 'ra_slot.h' in _build.HEADERS
    return kernel_usage('ffcv_augmix.hip')


def _one(usage, frag):
    hits = [v for k, v in usage.items() if f'{len(frag.split("I")[0])}{frag}' in k]    # <length><name> of the mangled name
    assert len(hits) == 1, (frag, sorted(usage))
    return hits[0]


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    assert len(usage) == len(BUDGET), sorted(usage)
    u = _one(usage, frag)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds <= LDS_LIMIT
