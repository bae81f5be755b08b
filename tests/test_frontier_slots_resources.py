"""The one-slot frontier (csrc/grow_frontier.hpp) costs the seed loop no registers: compiled
for gfx950 with the library's flags, seed_loop_kernel<false, 1> spills no more VGPRs than
the two-slot seed_loop_kernel<false, 2> (the compiler's kernel-resource-usage remarks, as
tools/resource_usage.py reads them).  Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from openpifpaf_amd import build as b


def _vgpr_spills(stderr):
    """{mangled kernel name: VGPR spills} from -Rpass-analysis=kernel-resource-usage."""
    out, name = {}, None
    for line in stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'VGPRs Spill: (\d+)', line)
        if m and name:
            out[name] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(b.HIPCC), reason='hipcc is not installed')
def test_one_slot_seed_loop_spills_no_more_than_two_slot(tmp_path):
    cmd = [b.HIPCC] + b.CFLAGS + ['--offload-device-only', '-Rpass-analysis=kernel-resource-usage',
                                  '-c', os.path.join(b.CSRC, 'seed_loop.hip'),
                                  '-o', str(tmp_path / 'seed_loop.o')]
    res = subprocess.run(cmd, capture_output=True, text=True, check=False)
    assert res.returncode == 0, res.stderr[-2000:]
    spills = _vgpr_spills(res.stderr)
    one = [v for k, v in spills.items() if 'seed_loop_kernelILb0ELi1E' in k]
    two = [v for k, v in spills.items() if 'seed_loop_kernelILb0ELi2E' in k]
    assert len(one) == 1 and len(two) == 1, sorted(spills)
    print('VGPR spills: one slot', one[0], 'two slots', two[0])
    assert one[0] <= two[0]
