"""Register budget of the CutMix kernel (csrc/ffcv_cutmix.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

The kernel must run without LDS, without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  cutmix_kernel<4>   (runs of 4 samples)   62 VGPRs, 8 waves/SIMD

(four 16-byte pieces in flight with their 64-bit addresses, and the 16 bytes
of a piece that straddles a box edge, loaded before the first is stored).  The
kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'cutmix_kernelILi4E': (62, 8),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_cutmix.hip' in _build.SOURCES
    return kernel_usage('ffcv_cutmix.hip')


def test_every_cutmix_kernel_is_reported(usage):
    kernels = [k for k in usage if 'cutmix_' in k]
    assert len(kernels) == len(BUDGET) == len(usage), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in kernels) == 1, (frag, kernels)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['LDS Size [bytes/block]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
