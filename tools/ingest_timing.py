"""Ingest timing at the cfg3 head sizes: 256 images, CIF 17 / CAF 19 fields, quad 1, conv
40 x 41 (fields 79 x 81).  HIP events around each call, warm-up first, the cases of a group
in alternation, median of --runs (>= 20) per case.  One JSON line per case.

    python tools/ingest_timing.py [--baseline-lib PATH] [--runs 21] [--images 256]
                                  [--groups plain,nhwc-f16,...]

Groups (each: the new path against what a user of the earlier library did):
  plain   pp_fields_from_conv, f32         | the same symbol of --baseline-lib
  hflip   f32 with hflip (one pass)        | baseline ingest + torch composition
  f16     float16 conv read directly       | .float() + baseline ingest
  bf16    bfloat16 conv read directly      | .float() + baseline ingest
          (f16 and bf16 also time pp_fields_from_conv_ex on the half tensor through ctypes:
          `direct` is this build's, `parent` the baseline library's)
  nhwc-f32, nhwc-f16, nhwc-bf16
          channels-last conv read directly | .contiguous() + baseline ingest of that type
  slice   CIF and CAF as channel slices of one fused NCHW float32 tensor, read directly
                                           | .contiguous() + baseline ingest
--baseline-lib is a libpifpaf_amd.so built from the commit to compare against (its
pp_fields_from_conv and pp_fields_from_conv_ex are called through ctypes); without it the
baselines use this build's symbols, which says nothing about the first group.

The torch composition works on the ingested fields (index_select over the fields, flip of
the columns, x -> (W - 1) - x for the regression x channels, the end-point swap on a clone),
i.e. the memory traffic of the reference's PifHFlip / PafHFlip; it is timed, not compared.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, constants, heads  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._lib import load  # noqa: E402  pylint: disable=wrong-import-position

H, W, QUAD = 40, 41, 1
HEADS = {'cif': (17, heads.cif_hflip(constants.COCO_KEYPOINTS)),
         'caf': (19, heads.caf_hflip(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON))}


def old_symbol(lib):
    fn = lib.pp_fields_from_conv
    fn.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_void_p] * 2
    fn.restype = ctypes.c_int

    def ingest(conv, kind, out):
        n_fields = HEADS[kind][0]
        rc = fn(conv.data_ptr(), conv.shape[0], n_fields, heads.LAYOUTS[kind][0], H, W, QUAD,
                out.data_ptr(), _device.stream())
        assert rc == 0, rc
        return out
    return ingest


def ex_symbol(lib):
    """pp_fields_from_conv_ex of `lib` on a dense conv of any supported type, unflipped."""
    fn = lib.pp_fields_from_conv_ex
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int32] * 8 + [ctypes.c_void_p] * 3 +
                   [ctypes.c_int32] * 2 + [ctypes.c_void_p])
    fn.restype = ctypes.c_int
    dtypes = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

    def ingest(conv, kind, out):
        assert conv.is_contiguous()
        n_fields = HEADS[kind][0]
        rc = fn(conv.data_ptr(), dtypes[conv.dtype], conv.shape[0], n_fields,
                heads.LAYOUTS[kind][0], H, W, QUAD, 0, None, None, out.data_ptr(), n_fields, 0,
                _device.stream())
        assert rc == 0, rc
        return out
    return ingest


def torch_unflip(fields, kind, flip, idx):
    """PifHFlip / PafHFlip's work on ingested fields (B, F, 5 | 9, H, W)."""
    out = torch.index_select(fields, 1, idx)
    out = torch.flip(out, dims=[4])
    xs = (1,) if kind == 'cif' else (1, 5)
    for c in xs:
        out[:, :, c].neg_().add_(float(out.shape[4] - 1))
    if kind == 'caf':
        for f, s in enumerate(flip.swap_ends):
            if s:
                keep = out[:, f, 1:3].clone()
                out[:, f, 1:3] = out[:, f, 5:7]
                out[:, f, 5:7] = keep
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_group(cases, runs, warmup=3):
    """cases: {name: callable}.  Alternating runs; -> {name: (median ms, min, max)}."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(runs):
        for name, fn in cases.items():
            times[name].append(timed(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--runs', type=int, default=21)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--groups', default=None, help='comma-separated subset of the groups')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    this, this_ex = old_symbol(load()), ex_symbol(load())
    base_lib = ctypes.CDLL(os.path.abspath(args.baseline_lib)) if args.baseline_lib else load()
    base, base_ex = old_symbol(base_lib), ex_symbol(base_lib)
    wanted = args.groups.split(',') if args.groups else None
    fused = torch.randn((args.images, sum(n * heads.LAYOUTS[k][1] for k, (n, _) in HEADS.items())
                         * 4 ** QUAD, H, W), device='cuda')
    first = 0
    info = {'device': torch.cuda.get_device_name(0), 'images': args.images, 'runs': args.runs,
            'baseline_lib': args.baseline_lib}
    for kind, (n_fields, flip) in HEADS.items():
        n_out = heads.LAYOUTS[kind][1]
        conv = torch.randn((args.images, n_fields * n_out * 4 ** QUAD, H, W), device='cuda')
        out = torch.empty((args.images, n_fields, n_out, heads.fields_dim(H, QUAD),
                           heads.fields_dim(W, QUAD)), device='cuda')
        idx = torch.tensor(flip.src_field, device='cuda')
        groups = {
            'plain': {'new': lambda: this(conv, kind, out),
                      'baseline': lambda: base(conv, kind, out)},
            'hflip': {'new': lambda: heads.fields_from_conv(conv, n_fields, kind, QUAD,
                                                            hflip=flip, out=out),
                      'baseline': lambda: torch_unflip(base(conv, kind, out), kind, flip, idx)},
        }
        for name, dtype in (('f16', torch.float16), ('bf16', torch.bfloat16)):
            half = conv.to(dtype)
            groups[name] = {
                'new': lambda half=half: heads.fields_from_conv(half, n_fields, kind, QUAD,
                                                                out=out),
                'baseline': lambda half=half: base(half.float(), kind, out),
                'direct': lambda half=half: this_ex(half, kind, out),
                'parent': lambda half=half: base_ex(half, kind, out)}
        for name, dtype in (('nhwc-f32', torch.float32), ('nhwc-f16', torch.float16),
                            ('nhwc-bf16', torch.bfloat16)):
            nhwc = conv.to(dtype).contiguous(memory_format=torch.channels_last)
            assert nhwc.stride(1) == 1
            groups[name] = {
                'new': lambda nhwc=nhwc: heads.fields_from_conv(nhwc, n_fields, kind, QUAD,
                                                                out=out),
                'baseline': lambda nhwc=nhwc: base_ex(nhwc.contiguous(), kind, out)}
        part = fused[:, first:first + conv.shape[1]]
        first += conv.shape[1]
        assert not part.is_contiguous() and part.shape == conv.shape
        groups['slice'] = {
            'new': lambda: heads.fields_from_conv(part, n_fields, kind, QUAD, out=out),
            'baseline': lambda: base_ex(part.contiguous(), kind, out)}
        sizes = {'f16': 2, 'bf16': 2, 'nhwc-f16': 2, 'nhwc-bf16': 2}
        for group, cases in groups.items():
            if wanted is not None and group not in wanted:
                continue
            res = run_group(cases, args.runs)
            for case, (med, lo, hi) in res.items():
                print(json.dumps(dict(info, head=kind, group=group, case=case,
                                      median_ms=round(med, 4), min_ms=round(lo, 4),
                                      max_ms=round(hi, 4),
                                      conv_bytes=conv.nbytes * sizes.get(group, 4) // 4,
                                      out_bytes=out.nbytes)), flush=True)
        del conv, out, groups, part
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
