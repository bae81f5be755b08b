"""The CafScored builds (csrc/stages.hip, caf_bucketed_body) keep the resources that let one
of their workgroups run on a CU beside a seed-loop workgroup, however many loads they keep in
flight: compiled for gfx950 with the library's flags (the compiler's kernel-resource-usage
remarks, as tools/resource_usage.py reads them),

- set A (caf_bucketed_kernel<false, true> and the ragged kernel): at most 37,440 B of LDS and
  128 VGPRs;
- set B (caf_bucketed_kernel<true, true>, the one-round form of the gated launches and the
  two-batch form of the ungated ones): at most 6,496 B of static LDS (the launch adds 4 B
  per cell) and 96 VGPRs, which is two waves per SIMD beside two seed-loop waves;
- no VGPR spills and no scratch in any of them.

Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from openpifpaf_amd import build as b

FIELDS = {'VGPRs': 'vgprs', 'VGPRs Spill': 'vgpr_spills', 'ScratchSize [bytes/lane]': 'scratch',
          'LDS Size [bytes/block]': 'lds'}
LIMITS = {  # mangled-name fragment: (LDS bytes, VGPRs)
    'caf_bucketed_kernelILb1ELb1ELb1EE': (6496, 96),
    'caf_bucketed_kernelILb1ELb1ELb0EE': (6496, 96),
    'caf_bucketed_kernelILb0ELb1ELb0EE': (37440, 128),
    'caf_bucketed_ragged_kernel': (37440, 128),
}


def _usage(stderr):
    """{mangled kernel name: {field: value}} from -Rpass-analysis=kernel-resource-usage."""
    out, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            out[name] = {}
        for label, key in FIELDS.items():
            m = re.search(r'\s' + re.escape(label) + r': (\d+)', line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


@pytest.fixture(scope='module')
def usage(tmp_path_factory):
    if not os.path.exists(b.HIPCC):
        pytest.skip('hipcc is not installed')
    obj = tmp_path_factory.mktemp('caf_rounds') / 'stages.o'
    cmd = [b.HIPCC] + b.CFLAGS + b.FILE_FLAGS.get('stages.hip', []) + [
        '--offload-device-only', '-Rpass-analysis=kernel-resource-usage',
        '-c', os.path.join(b.CSRC, 'stages.hip'), '-o', str(obj)]
    res = subprocess.run(cmd, capture_output=True, text=True, check=False)
    assert res.returncode == 0, res.stderr[-2000:]
    return _usage(res.stderr)


@pytest.mark.parametrize('kernel', list(LIMITS))
def test_caf_bucketed_resources(usage, kernel):
    found = [v for k, v in usage.items() if kernel in k]
    assert len(found) == 1, sorted(usage)
    u = found[0]
    print(kernel, u)
    lds, vgprs = LIMITS[kernel]
    assert u['lds'] <= lds
    assert u['vgprs'] <= vgprs
    assert u['vgpr_spills'] == 0
    assert u['scratch'] == 0
