"""Register budgets of the first-generation standalone transforms
(csrc/ffcv_standalone.hip), from the compiler's own resource remarks of a
device-only compile with the library's flags (no GPU needed).

Every kernel runs at eight waves per SIMD without spills, and without scratch
except translate_draw_kernel, which carries the 32 bytes of mt_new_at's call
frame.  As written the compiler reports, for gfx950:

  cutout_kernel            10 VGPRs      lut_kernel<u8>   36 VGPRs
  flip_kernel              19 VGPRs      lut_kernel<u16>  36 VGPRs
  translate_kernel         24 VGPRs      lut_kernel<u32>  28 VGPRs
  translate_draw_kernel    61 VGPRs      lut_kernel<u64>  34 VGPRs

Each kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, scratch bytes)
BUDGET = {
    'cutout_kernel': (10, 8, 0),
    'flip_kernel': (19, 8, 0),
    '16translate_kernel': (24, 8, 0),
    'translate_draw_kernel': (61, 8, 32),
    'lut_kernelIhE': (36, 8, 0),
    'lut_kernelItE': (36, 8, 0),
    'lut_kernelIjE': (28, 8, 0),
    'lut_kernelImE': (34, 8, 0),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_standalone.hip' in _build.SOURCES
    return kernel_usage('ffcv_standalone.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in usage) == 1, (frag, sorted(usage))


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_spills_and_pinned_registers(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy, scratch = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] <= scratch
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] == occupancy
