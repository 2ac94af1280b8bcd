"""Register, spill and LDS budgets of the raw crop + resize kernels and the
decoder draw (csrc/ffcv_rrc.hip), from the compiler's own resource remarks of
a device-only compile with the library's flags (no GPU needed).

rrc_raw_kernel is compiled for five waves per SIMD (its LDS allows five
workgroups per CU), which caps it at 96 VGPRs; it runs without scratch and
without VGPR spills, and what does not fit its SGPRs is spilled to VGPR lanes
(16 / 18 SGPRs).  Its static LDS is RrcLds: the source-row stage, the row taps
and, for fp16, the LUT.  draw_kernel carries the 32 bytes of scratch of
mt_new_at's call frame.  As written the compiler reports, for gfx950:

  rrc_raw_kernel<false>  (u8)       94 VGPRs, 5 waves/SIMD, 31184 bytes of LDS
  rrc_raw_kernel<true>   (fp16)     95 VGPRs, 5 waves/SIMD, 32704 bytes of LDS
  rrc_taps_kernel                   22 VGPRs, 8 waves/SIMD
  draw_kernel                       79 VGPRs, 6 waves/SIMD, 32 bytes of scratch

Each kernel is pinned to its count, so that a change that costs registers or
occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, scratch bytes, SGPR spills, LDS bytes or None)
BUDGET = {
    'rrc_raw_kernelILb0E': (94, 5, 0, 16, 31184),
    'rrc_raw_kernelILb1E': (95, 5, 0, 18, 32704),
    'rrc_taps_kernel': (22, 8, 0, 0, None),
    '11draw_kernel': (79, 6, 32, 16, None),
}


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_rrc.hip' in _build.SOURCES and 'resize_out.h' in _build.HEADERS
    return kernel_usage('ffcv_rrc.hip')


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        assert sum(frag in k for k in usage) == 1, (frag, sorted(usage))


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_pinned_registers_spills_and_lds(usage, frag):
    u = next(v for k, v in usage.items() if frag in k)
    print(frag, u)
    vgprs, occupancy, scratch, sgpr_spill, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] <= scratch
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] <= sgpr_spill
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    if lds is not None:
        assert u['LDS Size [bytes/block]'] == lds
