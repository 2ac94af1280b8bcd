"""Register and LDS budget of the RandAugment kernels
(csrc/ffcv_randaugment.hip), from the compiler's own resource remarks of a
device-only compile with the library's flags (no GPU needed).

Both kernels must run without scratch and without VGPR or SGPR spills.  As
written the compiler reports, for gfx950:

  randaugment_draw_kernel  (one lane per sample)         136 VGPRs, 3 waves/SIMD, no LDS
  randaugment_kernel       (one workgroup per image)      69 VGPRs, 5 waves/SIMD, 28,688 B LDS

The draw keeps its nine output pointers in vector registers across the slots'
loop (in scalar registers they spill beside the trigonometry's constants); a
launch is one 64-lane workgroup per 64 samples, so its occupancy is never the
limit.  The fused kernel is bounded by its LDS: two image buffers, 768
counters and the tables stay under 32 KiB, so five 256-thread workgroups (20
waves, five per SIMD) share a CU's 160 KiB, and 69 VGPRs leave that occupancy
alone.  The kernels are pinned to these counts, so that a change that costs
registers, LDS or occupancy fails here; one that saves some lowers the bound.
"""
import pytest

from tests.resource_usage import kernel_usage

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes)
BUDGET = {
    'randaugment_draw_kernel': (136, 3, 0),
    'randaugment_kernel': (69, 5, 28688),
}
LDS_LIMIT = 32768   # five workgroups per CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    assert 'ffcv_randaugment.hip' in _build.SOURCES
    return kernel_usage('ffcv_randaugment.hip')


def _one(usage, frag):
    hits = [v for k, v in usage.items() if f'{len(frag)}{frag}' in k]    # <length><name> of the mangled name
    assert len(hits) == 1, (frag, sorted(usage))
    return hits[0]


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        _one(usage, frag)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_registers(usage, frag):
    u = _one(usage, frag)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds <= LDS_LIMIT
