"""Register and LDS budget of AugMix's kernel for images up to 224 x 224
(csrc/ffcv_augmix_large.hip), in the form of
test_randaugment_large_resource_usage.py.  Its 1024 threads are four waves per
SIMD: above 128 VGPRs the kernel cannot launch.  It shares the slot code of
randaugment_large_kernel (114 VGPRs); what its own loops over images and
chains need between two slots waits in LDS for that reason.
"""
import pytest

from tests.resource_usage import kernel_usage, find

LDS_PER_CU = 163840


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_augmix_large.hip' in _build.SOURCES
    return kernel_usage('ffcv_augmix_large.hip')


def test_no_scratch_no_spills_and_launchable(usage):
    assert len(usage) == 1, sorted(usage)
    u = find(usage, 'augmix_large_kernel')
    print(u)
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= 128 and u['Occupancy [waves/SIMD]'] >= 4
    assert u['LDS Size [bytes/block]'] <= LDS_PER_CU
