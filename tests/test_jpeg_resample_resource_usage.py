"""Register budget of the crop decoders' resample kernels from
the compiler's resource remarks (no GPU needed).

resample_raw_kernel is the transform kernel's shape: 80 VGPRs, 6 waves/SIMD.

jpeg_color_resample_kernel holds the image record's head, three components'
tile geometry and twelve prefetched tile dwords across its passes: 151 VGPRs,
3 waves/SIMD, no scratch and no VGPR spills (wave-uniform geometry spills to
lanes of a VGPR, as K2's did before its band records).  That occupancy is
what its LDS allows anyway: a workgroup of four waves takes 52.4 KiB at the
flagship shape (256 px -> 224, bicubic) and 53.6 KiB at 512 px, that is three
workgroups of a CU's 160 KiB, 3 waves/SIMD.  It runs behind
K1 on the stream, not beside it: K1's workgroups (38.8 KiB of LDS, one wave per
image) have left the CU's LDS before the band workgroups arrive, so this
kernel's registers do not take occupancy from K1."""
from tests.resource_usage import find, kernel_usage


def test_no_scratch_no_vgpr_spills_and_pinned_registers():
    for source, kernel, vgprs, waves in (('ffcv_jpeg.hip', 'jpeg_color_resample_kernel', 152, 3),
                                         ('ffcv_resample_raw.hip', 'resample_raw_kernel', 80, 6)):
        u = find(kernel_usage(source), kernel)
        print(kernel, u)
        assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0
        assert u['VGPRs'] <= vgprs and u['Occupancy [waves/SIMD]'] >= waves
    assert len(kernel_usage('ffcv_resample_raw.hip')) == 1
