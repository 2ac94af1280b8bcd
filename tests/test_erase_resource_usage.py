"""Register budget of the RandomErasing kernels (csrc/ffcv_erase.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel must run without scratch and without VGPR or SGPR spills.  As
written the compiler reports, for gfx950:

  erase_constant_kernel            20 VGPRs, 8 waves/SIMD, 96 bytes of LDS (one plane's pixel, expanded)
  erase_noise_kernel<1, staged>    24 VGPRs, 8 waves/SIMD,  4096 bytes of LDS (the table)
  erase_noise_kernel<2, staged>    19 VGPRs, 8 waves/SIMD,  8192
  erase_noise_kernel<4, staged>    24 VGPRs, 8 waves/SIMD, 16384
  erase_noise_kernel<1, cache>     36 VGPRs, 8 waves/SIMD, no LDS     (16 table entries per piece)
  erase_noise_kernel<2, cache>     28 VGPRs, 8 waves/SIMD, no LDS
  erase_noise_kernel<4, cache>     19 VGPRs, 8 waves/SIMD, no LDS
  erase_draw_kernel                66 VGPRs, 7 waves/SIMD, no LDS     (one lane per sample: log, exp, sqrt)

ffcv_erase_batch launches the `staged` form, whose LDS is the noise table's
size (4096 entries of the itemsize); the `cache` form, which reads the table
through the cache, is the one tools/erase_bench.py measures it against
(DESIGN.md s26).  The kernels are pinned to their counts, so that a change that costs
registers or occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes)
BUDGET = {
    'erase_constant_kernel': (20, 8, 96),
    'erase_noise_kernelILi1ELb0E': (36, 8, 0),
    'erase_noise_kernelILi2ELb0E': (28, 8, 0),
    'erase_noise_kernelILi4ELb0E': (19, 8, 0),
    'erase_noise_kernelILi1ELb1E': (24, 8, 4096),
    'erase_noise_kernelILi2ELb1E': (19, 8, 8192),
    'erase_noise_kernelILi4ELb1E': (24, 8, 16384),
    'erase_draw_kernel': (66, 7, 0),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_erase.hip' in _build.SOURCES and 'erase_common.h' in _build.HEADERS
    return kernel_usage('ffcv_erase.hip')


def test_every_erase_kernel_is_reported(usage):
    kernels = [k for k in usage if 'erase_' in k]
    assert len(kernels) == len(BUDGET) == len(usage), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in kernels) == 1, (frag, kernels)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['LDS Size [bytes/block]'] == lds
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
