"""K1's (`jpeg_entropy_kernel<0>`) resource budget with the chunked write
pass, from the compiler's own resource remarks of a device-only compile with
the library's flags (no GPU needed).

Four K1 workgroups share a CU with one K2 wave per SIMD: at
most 112 VGPRs (512 - 4 x 112 leaves K2's 64), at most 160 KB / 4 of LDS, and
no more scratch than the 32 bytes per lane of its out-of-line draw helpers.
"""
import pytest

from tests.resource_usage import kernel_usage

K1 = '_Z19jpeg_entropy_kernelILi0EEv8JpegArgs'


@pytest.fixture(scope='module')
def usage():
    return kernel_usage('ffcv_jpeg.hip')


def test_k1_budget(usage):
    u = usage[K1]
    print(u)
    assert u['VGPRs'] <= 112
    assert u['VGPRs Spill'] == 0
    assert u['LDS Size [bytes/block]'] <= 40960
    assert u['ScratchSize [bytes/lane]'] <= 32
    assert u['Occupancy [waves/SIMD]'] >= 4
