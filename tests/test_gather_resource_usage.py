"""Register budgets of the row-gather kernels (csrc/ffcv_gather.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every gather kernel must run without scratch and without VGPR or SGPR spills.
As written the compiler reports, for gfx950:

  gather_rows_kernel<16>   (16 lanes per row)   20 VGPRs, 8 waves/SIMD
  gather_rows_kernel<64>   (a wave per row)     20 VGPRs, 8 waves/SIMD
  gather_rows_grid_kernel  (2-D grid)           68 VGPRs, 7 waves/SIMD
  gather_raw_kernel        (raw sample bytes)    5 VGPRs, 8 waves/SIMD
  gather_samples_kernel    (descriptors)        12 VGPRs, 8 waves/SIMD

(the grid kernel holds four vectors of five dwords per lane in flight; the
last two are the decoders' simple gathers).  Each
kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD)
BUDGET = {
    'gather_rows_kernelILi16E': (20, 8),
    'gather_rows_kernelILi64E': (20, 8),
    'gather_rows_grid_kernel': (68, 7),
    'gather_raw_kernel': (5, 8),
    'gather_samples_kernel': (12, 8),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_gather.hip' in _build.SOURCES
    return kernel_usage('ffcv_gather.hip')


def test_every_gather_kernel_is_reported(usage):
    kernels = [k for k in usage if 'gather_' in k]
    assert len(kernels) == len(BUDGET) == len(usage), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in kernels) == 1, (frag, kernels)


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
