"""Register and LDS budgets of the colour kernels (csrc/ffcv_color.hip), from
the compiler's own resource remarks of a device-only compile with the
library's flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  uniform_draw_kernel  (one lane per sample)            9 VGPRs, 8 waves/SIMD, no LDS
  color_jitter_kernel  (a workgroup per image / tile)  40 VGPRs, 8 waves/SIMD, 16,688 bytes of LDS

The jitter kernel's LDS is 16 KiB of pixels + 32 B staging slack, the 256-byte
table and 16 bytes of gray-sum partials: eight 256-thread workgroups (all 32
waves of a CU) share its 160 KiB, so LDS never limits occupancy.  Each kernel
is pinned to its counts, so that a change that costs registers, LDS or
occupancy fails here; one that saves some lowers the bound.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ffcv_amd', 'csrc')

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes per workgroup)
BUDGET = {
    'uniform_draw_kernel': (9, 8, 0),
    'color_jitter_kernel': (40, 8, 16688),
}
WORKGROUPS_PER_CU = 8
LDS_LIMIT = 160 * 1024 // WORKGROUPS_PER_CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    assert 'ffcv_color.hip' in _build.SOURCES
    assert {'color_common.h', 'lds_stage.h'} <= set(_build.HEADERS)
    flags = [f for f in _build.FLAGS if f != '-shared']
    cmd = [hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-o', os.devnull,
                             'ffcv_color.hip']
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


def _find(usage, frag):
    """The kernel whose mangled name carries exactly this name: <length><name>."""
    hits = [v for k, v in usage.items() if f'{len(frag)}{frag}' in k]
    assert len(hits) == 1, (frag, sorted(usage))
    return hits[0]


def test_every_kernel_is_reported(usage):
    assert len(usage) == len(BUDGET), sorted(usage)
    for frag in BUDGET:
        _find(usage, frag)


@pytest.mark.parametrize('frag', sorted(BUDGET))
def test_no_scratch_no_spills_and_pinned_resources(usage, frag):
    u = _find(usage, frag)
    print(frag, u)
    vgprs, occupancy, lds = BUDGET[frag]
    assert u['ScratchSize [bytes/lane]'] == 0
    assert u['VGPRs Spill'] == 0
    assert u['SGPRs Spill'] == 0
    assert u['VGPRs'] <= vgprs
    assert u['Occupancy [waves/SIMD]'] >= occupancy
    assert u['LDS Size [bytes/block]'] <= lds <= LDS_LIMIT
    assert WORKGROUPS_PER_CU * lds <= 160 * 1024   # eight workgroups per CU: LDS never limits occupancy
