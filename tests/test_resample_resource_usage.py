"""Register budget of csrc/ffcv_resample.hip from the compiler's resource
remarks (no GPU needed): its one kernel, resample_images_kernel, runs without
scratch or spills at 80 VGPRs and 6 waves/SIMD on gfx950, and is pinned there."""
from tests.resource_usage import find, kernel_usage


def test_no_scratch_no_spills_and_pinned_registers():
    usage = kernel_usage('ffcv_resample.hip')
    assert len(usage) == 1, sorted(usage)
    u = find(usage, 'resample_images_kernel')
    print(u)
    assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0 and u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= 80 and u['Occupancy [waves/SIMD]'] >= 6
