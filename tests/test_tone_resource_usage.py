"""Register and LDS budgets of the tone kernels (csrc/ffcv_tone.hip), from the
compiler's own resource remarks of a device-only compile with the library's
flags (no GPU needed).

Every kernel of the file must run without scratch and without VGPR or SGPR
spills.  As written the compiler reports, for gfx950:

  tone_draw_kernel  (one lane per sample, up to 4 draws)   12 VGPRs, 8 waves/SIMD, no LDS
  tone_kernel       (a workgroup per image / tile)         40 VGPRs, 7 waves/SIMD, 21,168 bytes of LDS

The tone kernel's occupancy is set by its LDS: 16 KiB of pixels + 32 B staging
slack, 3 KiB of counters, two 768-byte tables and 144 bytes of scan partials
let seven 256-thread workgroups (28 of a CU's 32 waves) share its 160 KiB.
Each kernel is pinned to its counts, so that a change that costs registers,
LDS or occupancy fails here; one that saves some lowers the bound.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ffcv_amd', 'csrc')

# kernel name fragment -> (VGPRs, waves/SIMD, LDS bytes per workgroup)
BUDGET = {
    'tone_draw_kernel': (12, 8, 0),
    'tone_kernel': (40, 7, 21168),
}
WORKGROUPS_PER_CU = 7
LDS_LIMIT = 160 * 1024 // WORKGROUPS_PER_CU


@pytest.fixture(scope='module')
def usage():
    from ffcv_amd import _build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    assert 'ffcv_tone.hip' in _build.SOURCES and 'tone_common.h' in _build.HEADERS
    flags = [f for f in _build.FLAGS if f != '-shared']
    cmd = [hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-o', os.devnull,
                             'ffcv_tone.hip']
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
    if lds:   # seven workgroups per CU, not eight
        assert WORKGROUPS_PER_CU * lds <= 160 * 1024 < (WORKGROUPS_PER_CU + 1) * lds
