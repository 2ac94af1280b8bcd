"""Register budget of the elastic kernel (csrc/ffcv_elastic.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed), and the LDS its plan states.

As written the compiler reports, for gfx950: elastic_kernel 48 VGPRs, 8
waves/SIMD, no scratch, no spills, no static LDS (all of it is dynamic: the
plan's).  Pinned, so that a change that costs registers or occupancy fails
here; one that saves some lowers the bound.
"""
from tests.resource_usage import kernel_usage


def test_no_scratch_no_spills_and_pinned_registers():
    from ffcv_amd import _build
    assert 'ffcv_elastic.hip' in _build.SOURCES and 'elastic_common.h' in _build.HEADERS
    usage = kernel_usage('ffcv_elastic.hip')
    assert len(usage) == 1 and 'elastic_kernel' in next(iter(usage)), sorted(usage)
    u = next(iter(usage.values()))
    print(u)
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= 48 and u['Occupancy [waves/SIMD]'] >= 8
    assert u['LDS Size [bytes/block]'] == 0


def test_lds_plan(hip_lib):
    """16 | noise planes or the staging budget | horizontal-pass planes."""
    from ffcv_amd import libffcv as L
    def plan(th, tw, R):
        a = max(2 * (th + 2 * R) * ((tw + 1) // 2 + R) * 4, 16 + L.elastic_tile_lds() + 16)
        return 16 + (a + 15) // 16 * 16 + 2 * ((th + 1) // 2 + R) * 32 * 4
    assert L.elastic_lds_bytes(224, 224, 5.0) == plan(32, 32, 20) == 29968
    assert L.elastic_lds_bytes(5, 5, 1.0) == plan(5, 5, 4)
    assert L.elastic_lds_bytes(97, 131, 16.1) == plan(32, 32, 64) <= 160 * 1024
