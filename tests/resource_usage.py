"""The compiler's kernel resource remarks of one csrc source, for the
test_*_resource_usage.py budgets: a device-only compile with the library's
flags (no GPU needed)."""
import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ffcv_amd', 'csrc')


@functools.lru_cache(maxsize=None)
def kernel_usage(source):
    """{mangled kernel name: {remark: int}} of csrc/<source>; compiled once per session."""
    from ffcv_amd import _build
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    flags = [f for f in _build.FLAGS if f != '-shared']
    cmd = [hipcc] + flags + ['--cuda-device-only', '-c', '-Rpass-analysis=kernel-resource-usage', '-o', os.devnull,
                             source]
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


def find(usage, frag):
    """The kernel whose mangled name carries exactly this name: <length><name>."""
    hits = [v for k, v in usage.items() if f'{len(frag)}{frag}' in k]
    assert len(hits) == 1, (frag, sorted(usage))
    return hits[0]
