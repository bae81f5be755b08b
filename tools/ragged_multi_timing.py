"""Ragged multi-scale batches: planted images of mixed sizes under the ms2 and ms10
FieldConfigs (synthetic.MULTI_CASES), decoded three ways, and the one-launch packer against
per-head packs.

    python tools/ragged_multi_timing.py [--runs 20] [--warmup 3] [--images N] [--cases ms2,ms10]

The sizes (tools/ragged_sizes.json, fixed) are stride-8 field sizes of long-edge-641 inputs;
image i is synthetic.multi_case(case, seed i) at (h_i - 1) * 8 + 1 by (w_i - 1) * 8 + 1
pixels, 3 people, COCO skeleton, eval defaults.  HIP events around each route on the current
stream, --warmup runs first, the routes in alternation, median and min-max of --runs (>= 20).
One JSON line per case and route:

  ragged          (a) engine.RaggedHeadSet (tables, containers, the one pack launch) + the
                  checked decode (pp_decode_multi_ragged, overflow check included)
  per-image       (b) the same images one checked pp_decode_multi each, every size with an
                  engine (workspace) of its own, so no route allocates a workspace
  ceiling         (c) a batch of as many images all at the container size, one checked
                  pp_decode_multi
  pack            the pack alone with its host side (RaggedHeadSet: tables, allocations, launch)
  pack-kernels    its staging copy and launch alone (RaggedHeadSet.pack), with the bytes
                  (sources read + containers written) per second
  pack-per-head   the same heads through one pp_fields_pack_ragged per head, host side
                  included (tables and containers per head, as engine.RaggedFields builds them)
  pack-per-head-kernels  its copies and launches alone
and a line with the ratios.  The ragged route's records are compared with the per-image
route's, and the per-head pack's containers with the one-launch pack's, before anything is
timed."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, constants, decoder, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._abi import EVAL_CONFIG, make_config  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._lib import call, load  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import DecodeEngine, HeadSet, RaggedHeadSet  # noqa: E402  pylint: disable=wrong-import-position

SKEL = constants.COCO_PERSON_SKELETON


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class PerHeadPack:
    """The heads of `fields_list` packed by one pp_fields_pack_ragged call per head."""

    def __init__(self, fields_list, index):
        lib = load()
        n = len(fields_list)
        size, self.ext_off = lib.pp_ragged_tables_size(n), lib.pp_ragged_extents_offset(n)
        self.n, self.size, self.heads = n, size, []
        for j in index:
            row = [f[j] for f in fields_list]
            if not all(_device.is_device(t) and t.dtype == torch.float32 and t.is_contiguous()
                       and t.dim() == 4 for t in row):  # as RaggedFields checks its images
                raise ValueError('not a contiguous float32 device tensor')
            ext = np.array([t.shape[2:] for t in row], np.int32)
            h, w = (int(v) for v in ext.max(axis=0))
            out = torch.empty((n,) + tuple(row[0].shape[:2]) + (h, w), dtype=torch.float32,
                              device=row[0].device)
            host = torch.empty(size, dtype=torch.uint8, pin_memory=True)
            tables = torch.empty(size, dtype=torch.uint8, device=row[0].device)
            hn = host.numpy()
            hn[:self.ext_off].view(np.uint64)[:] = [t.data_ptr() for t in row]
            hn[self.ext_off:].view(np.int32)[:] = ext.reshape(-1)
            self.heads.append((out, host, tables, h, w))
        self.pack()

    def pack(self):
        for out, host, tables, h, w in self.heads:
            call('pp_fields_pack_ragged', ctypes.c_void_p(host.data_ptr()),
                 ctypes.c_void_p(host.data_ptr() + self.ext_off), self.n, out.shape[1],
                 out.shape[2], h, w, _device.ptr(out), _device.ptr(tables),
                 ctypes.c_size_t(self.size), _device.stream())


def run_case(case, sizes, args, info):
    n = len(sizes)
    cfg = make_config(**EVAL_CONFIG)
    fields_list, kw = [], None
    for i, (h, w) in enumerate(sizes):
        fields, kw = synthetic.multi_case(case, i, (h - 1) * 8 + 1, (w - 1) * 8 + 1, n_people=3)
        fields_list.append([_device.to_device(f) for f in fields])
    fc = decoder.FieldConfig(**kw)
    index = list(fc.cif_indices) + list(fc.caf_indices)
    hc, wc = (max(s[d] for s in sizes) for d in (0, 1))
    full = [synthetic.multi_case(case, i, (hc - 1) * 8 + 1, (wc - 1) * 8 + 1, n_people=3)[0]
            for i in range(n)]
    ceiling_heads = HeadSet([_device.to_device(np.stack([f[m] for f in full]))
                             for m in range(len(full[0]))], fc)
    per_image_heads = [HeadSet([f[None] for f in fields], fc) for fields in fields_list]

    eng, ceiling_eng = DecodeEngine(), DecodeEngine()
    per_shape = {s: DecodeEngine() for s in set(sizes)}

    def ragged():
        return eng.launch_checked(None, None, SKEL, cfg, ragged=RaggedHeadSet(fields_list, fc))

    def per_image():
        return [per_shape[s].launch_checked(None, None, SKEL, cfg, heads=hs)
                for s, hs in zip(sizes, per_image_heads)]

    def ceiling():
        return ceiling_eng.launch_checked(None, None, SKEL, cfg, heads=ceiling_heads)

    # the routes agree before they are timed
    recs, offsets = DecodeEngine.fetch(ragged())
    for i, (s, hs) in enumerate(zip(sizes, per_image_heads)):
        one, _ = DecodeEngine.fetch(per_shape[s].launch_checked(None, None, SKEL, cfg, heads=hs))
        got = recs[offsets[i]:offsets[i + 1]]
        assert len(got) == len(one), (i, len(got), len(one))
        for name in ('data', 'joint_scales', 'score', 'decoding_pairs', 'decoding_xyv'):
            assert got[name].tobytes() == one[name].tobytes(), (i, name)
    packed = RaggedHeadSet(fields_list, fc)
    per_head = PerHeadPack(fields_list, index)
    torch.cuda.synchronize()
    for a, (b, *_) in zip(packed.cifs + packed.cafs, per_head.heads):
        assert torch.equal(a, b)
    pack_bytes = 4 * (sum(fields[j].numel() for fields in fields_list for j in index) +
                      sum(t.numel() for t in packed.cifs + packed.cafs))

    routes = {'ragged': ragged, 'per-image': per_image, 'ceiling': ceiling,
              'pack': lambda: RaggedHeadSet(fields_list, fc), 'pack-kernels': packed.pack,
              'pack-per-head': lambda: PerHeadPack(fields_list, index),
              'pack-per-head-kernels': per_head.pack}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, fn in routes.items():
            times[name].append(events(fn))
    info = dict(info, case=case, images=n, heads=len(index), annotations=int(offsets[-1]))
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        line = dict(info, route=name, median_ms=round(med[name], 4), min_ms=round(min(t), 4),
                    max_ms=round(max(t), 4),
                    images_per_s=None if name.startswith('pack') else round(n / med[name] * 1e3, 1))
        if name in ('pack-kernels', 'pack-per-head-kernels'):
            line.update(bytes=pack_bytes, tb_per_s=round(pack_bytes / med[name] / 1e9, 3))
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(
        info, route='ratios',
        speedup_over_per_image=round(med['per-image'] / med['ragged'], 2),
        ragged_over_ceiling=round(med['ragged'] / med['ceiling'], 4),
        pack_over_per_head=round(med['pack'] / med['pack-per-head'], 4),
        pack_kernels_over_per_head_kernels=round(med['pack-kernels'] / med['pack-per-head-kernels'], 4))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--images', type=int, default=0, help='the first N sizes (default: all)')
    ap.add_argument('--cases', default='ms2,ms10')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ragged_sizes.json')) as f:
        sizes = [tuple(s) for s in json.load(f)['sizes']]
    if args.images:
        sizes = sizes[:args.images]
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'runs': args.runs, 'warmup': args.warmup, 'clock': 'events'}
    for case in args.cases.split(','):
        run_case(case, sizes, args, info)


if __name__ == '__main__':
    main()
