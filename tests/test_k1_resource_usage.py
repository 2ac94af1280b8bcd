"""K1's (`jpeg_entropy_kernel<0>`) resource budget with the chunked write
pass, from the compiler's own resource remarks of a device-only compile with
the library's flags (no GPU needed).

Four K1 workgroups share a CU with one K2 wave per SIMD: at
most 112 VGPRs (512 - 4 x 112 leaves K2's 64), at most 160 KB / 4 of LDS, and
no more scratch than the 32 bytes per lane of its out-of-line draw helpers.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ffcv_amd', 'csrc')
K1 = '_Z19jpeg_entropy_kernelILi0EEv8JpegArgs'


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    flags = [f for f in _build.FLAGS if f != '-shared']
    cmd = [hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-o', os.devnull,
                             'ffcv_jpeg.hip']
    err = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r'remark:\s+(.*?) \[-Rpass-analysis', line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(':')
        if key == 'Function Name':
            cur = out.setdefault(val.strip(), {})
        elif cur is not None and val.strip().lstrip('-').isdigit():
            cur[key.strip()] = int(val)
    return out


def test_k1_budget(usage):
    u = usage[K1]
    print(u)
    assert u['VGPRs'] <= 112
    assert u['VGPRs Spill'] == 0
    assert u['LDS Size [bytes/block]'] <= 40960
    assert u['ScratchSize [bytes/lane]'] <= 32
    assert u['Occupancy [waves/SIMD]'] >= 4
