"""A/B of the planar ingest kernels whose code changed with the refactor: this build against
the parent's library, same process, alternating, HIP events, median of 21 (min-max).  256
images, conv 40 x 41, quad 1, CIF 17 / CAF 19.  Cases: dense (ingest_kernel) and a channel
slice of a fused tensor (ingest_strided_kernel), plain and with the hflip tables, f32 / f16 /
bf16.  Outputs are compared byte for byte first.

    python tools/ingest_parent_ab.py PARENT_LIB     (a libpifpaf_amd.so built from the parent)"""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))
from openpifpaf_amd import _device, build, constants, heads  # noqa: E402
from openpifpaf_amd._lib import load  # noqa: E402

H, W, QUAD, N = 40, 41, 1, 256
HEADS = {'cif': (17, heads.cif_hflip(constants.COCO_KEYPOINTS)),
         'caf': (19, heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON))}
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def strided(lib):
    fn = lib.pp_fields_from_conv_strided
    fn.argtypes = ([ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p] + [ctypes.c_int32] * 7 +
                   [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 2 + [ctypes.c_void_p])
    fn.restype = ctypes.c_int

    def run(conv, kind, flip, out):
        n_fields = HEADS[kind][0]
        src, swap = flip.tables(n_fields) if flip else (None, None)
        rc = fn(conv.data_ptr(), DT[conv.dtype], (ctypes.c_int64 * 4)(*conv.stride()),
                conv.shape[0], n_fields, heads.LAYOUTS[kind][0], H, W, QUAD, int(flip is not None),
                src, swap, out.data_ptr(), n_fields, 0, _device.stream())
        assert rc == 0, rc
    return run


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    _device.require()
    new = strided(load())
    parent = strided(ctypes.CDLL(os.path.abspath(sys.argv[1])))
    for kind, (n_fields, flip) in HEADS.items():
        n_out = heads.LAYOUTS[kind][1]
        ch = n_fields * n_out * 4
        out_a = torch.empty((N, n_fields, n_out, 79, 81), device='cuda')
        out_b = torch.empty_like(out_a)
        for dtype in DT:
            fused = torch.randn((N, ch + 8, H, W), device='cuda').to(dtype)
            views = {'dense': fused[:, 4:4 + ch].contiguous(), 'slice': fused[:, 4:4 + ch]}
            for layout, conv in views.items():
                for fl in (None, flip):
                    out_a.fill_(1.0)
                    out_b.fill_(2.0)
                    new(conv, kind, fl, out_a)
                    parent(conv, kind, fl, out_b)
                    assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
                    cases = {'new': lambda: new(conv, kind, fl, out_a),
                             'parent': lambda: parent(conv, kind, fl, out_b)}
                    for _ in range(3):
                        for fn in cases.values():
                            fn()
                    torch.cuda.synchronize()
                    t = {k: [] for k in cases}
                    for _ in range(21):
                        for k, fn in cases.items():
                            t[k].append(timed(fn))
                    print(json.dumps(dict(
                        head=kind, dtype=str(dtype).split('.')[1], view=layout,
                        hflip=fl is not None, src_sha=build.source_digest(),
                        **{k + '_ms': [round(statistics.median(v), 4), round(min(v), 4),
                                       round(max(v), 4)] for k, v in t.items()})), flush=True)
            del fused, views


if __name__ == '__main__':
    main()
