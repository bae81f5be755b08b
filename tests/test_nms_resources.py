"""The one-launch NMS (csrc/nms.hip, nms_kernel<W, 0>) keeps the resources that let a
workgroup of it run on a CU beside a seed-loop workgroup and a set-A workgroup, with both of its
paths (images of at most kNmsSmall annotations decided across lanes, the box lists above) in one
kernel: compiled for gfx950 with the library's flags (the compiler's kernel-resource-usage
remarks, as tools/resource_usage.py reads them),

- nms_kernel<4, 0>: at most 1,792 B of LDS, which is what a CU has left beside a seed-loop
  workgroup (124,608 B) and a set-A workgroup (37,440 B);
- nms_kernel<4, 0> and nms_kernel<8, 0>: at most 128 VGPRs (four waves per SIMD), no VGPR spill
  and no scratch.

Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from openpifpaf_amd import build as b

FIELDS = {'VGPRs': 'vgprs', 'VGPRs Spill': 'vgpr_spills', 'ScratchSize [bytes/lane]': 'scratch',
          'LDS Size [bytes/block]': 'lds'}
CU_LDS = 160 * 1024
NMS_LDS = CU_LDS - 124608 - 37440
LIMITS = {  # mangled-name fragment: (LDS bytes or None, VGPRs)
    'nms_kernelILi4ELi0EE': (NMS_LDS, 128),
    'nms_kernelILi8ELi0EE': (None, 128),
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
    obj = tmp_path_factory.mktemp('nms_resources') / 'nms.o'
    cmd = [b.HIPCC] + b.CFLAGS + b.FILE_FLAGS.get('nms.hip', []) + [
        '--offload-device-only', '-Rpass-analysis=kernel-resource-usage',
        '-c', os.path.join(b.CSRC, 'nms.hip'), '-o', str(obj)]
    res = subprocess.run(cmd, capture_output=True, text=True, check=False)
    assert res.returncode == 0, res.stderr[-2000:]
    return _usage(res.stderr)


def test_lds_left_beside_seed_loop_and_set_a():
    assert NMS_LDS == 1792


@pytest.mark.parametrize('kernel', list(LIMITS))
def test_nms_kernel_resources(usage, kernel):
    found = [v for k, v in usage.items() if kernel in k]
    assert len(found) == 1, sorted(usage)
    u = found[0]
    print(kernel, u)
    lds, vgprs = LIMITS[kernel]
    if lds is not None:
        assert u['lds'] <= lds
    assert u['vgprs'] <= vgprs
    assert u['vgpr_spills'] == 0
    assert u['scratch'] == 0
