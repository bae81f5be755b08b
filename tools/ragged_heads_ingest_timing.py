"""Conv outputs of every head of a ragged multi-scale batch into its containers, timed six ways.

    python tools/ragged_heads_ingest_timing.py [--runs 20] [--warmup 3] [--images 64]
                                               [--cases ms2,ms10] [--dtypes float32,float16]

The setup is that of tools/ragged_multi_timing.py: the first --images sizes of
tools/ragged_sizes.json (stride-8 field sizes of long-edge-641 inputs), image i is
synthetic.multi_case(case, seed i) at (h_i - 1) * 8 + 1 by (w_i - 1) * 8 + 1 pixels, 3 people.
Every head's planted field is turned into the conv output it is ingested from at quad 0 (the
inverse of the head's tail: logit, minus the index grid, log), so the ingested fields are the
planted fields again.  HIP events around each route on the current stream, --warmup runs first,
the routes in alternation, median and min-max of --runs (>= 20).  One JSON line per case, dtype
and route:

  per-image          (a) one fields_from_conv per image per head (n * heads calls), then
                     engine.RaggedHeadSet (the pack of all heads)
  per-entry          (b) one heads.RaggedIngest per head (tables, container, launch): one
                     pp_fields_from_conv_ragged call per head
  from-conv          (c) engine.RaggedHeadSet.from_conv(one_launch=True): one pinned block, the
                     containers, one pp_fields_from_conv_ragged_heads call
  from-conv-default  engine.RaggedHeadSet.from_conv as it is called by default: (b) with the
                     joint extent table, the K and C checks and the pp_scale array
  from-conv-kernels  (c') its library call alone (the staging copy and the launch), with the
                     bytes read + written per second
  per-entry-kernels  (b') the per-head library calls alone
and a line with c / a, b' - c' and the larger min-max spread of the two.  The containers of
(a), (b) and (c) are compared byte for byte before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, decoder, heads, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import RaggedHeadSet  # noqa: E402  pylint: disable=wrong-import-position

PERM = {'cif': (0, 1, 2, 3, 4), 'caf': (0, 1, 2, 5, 7, 3, 4, 6, 8)}


def conv_from_fields(field, kind):
    """Decoder fields (n_fields, 5 | 9, h, w) -> the quad-0 conv output (channels, h, w) grouped
    as conf, vectors, logb, scales: the inverse of the head's tail."""
    f = np.asarray(field, np.float64)
    _, _, h, w = f.shape
    nv = 1 if kind == 'cif' else 2
    cat = np.empty_like(f)
    cat[:, list(PERM[kind])] = f
    conf = np.clip(cat[:, :1], 1e-6, 1 - 1e-6)
    yy, xx = np.indices((h, w), dtype=np.float64)
    vec = cat[:, 1:1 + 2 * nv].copy()
    vec[:, 0::2] -= xx
    vec[:, 1::2] -= yy
    groups = (np.log(conf / (1 - conf)), vec, cat[:, 1 + 2 * nv:1 + 3 * nv],
              np.log(np.maximum(cat[:, 1 + 3 * nv:], 1e-6)))
    return np.nan_to_num(np.concatenate([g.reshape(-1, h, w) for g in groups])).astype(np.float32)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def same_bytes(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_case(case, sizes, dtype_name, args, info):
    n = len(sizes)
    dtype = getattr(torch, dtype_name)
    host, kw = [], None
    for i, (h, w) in enumerate(sizes):
        fields, kw = synthetic.multi_case(case, i, (h - 1) * 8 + 1, (w - 1) * 8 + 1, n_people=3)
        host.append(fields)
    fc = decoder.FieldConfig(**kw)
    index = list(fc.cif_indices) + list(fc.caf_indices)
    kinds = {j: 'cif' if j in fc.cif_indices else 'caf' for j in index}
    # convs[j][i]: head j of image i
    convs = {j: [torch.from_numpy(conv_from_fields(img[j], kinds[j])).to('cuda', dtype)
                 for img in host] for j in index}
    n_fields = {j: host[0][j].shape[0] for j in index}
    n_heads = max(index) + 1

    def per_image():
        return RaggedHeadSet(
            [[heads.fields_from_conv(convs[j][i][None], n_fields[j], kinds[j], 0)[0]
              if j in convs else None for j in range(n_heads)] for i in range(n)], fc)

    def per_entry():
        return [heads.RaggedIngest(convs[j], n_fields[j], kinds[j], 0).launch() for j in index]

    items = [convs.get(j) for j in range(n_heads)]

    def from_conv():
        return RaggedHeadSet.from_conv(items, fc, quad=0, one_launch=True)

    def from_conv_default():
        return RaggedHeadSet.from_conv(items, fc, quad=0)

    # the routes agree before they are timed
    packed, entries, ingested, default = per_image(), per_entry(), from_conv(), from_conv_default()
    torch.cuda.synchronize()
    for a, b, c, d in zip(packed.cifs + packed.cafs, entries, ingested.cifs + ingested.cafs,
                          default.cifs + default.cafs):
        assert a.shape == b.out.shape == c.shape == d.shape
        assert same_bytes(a, b.out) and same_bytes(a, c) and same_bytes(a, d)
    assert torch.equal(packed.extents, ingested.extents)
    assert torch.equal(packed.extents, default.extents)
    assert ingested.shape_key == packed.shape_key

    def entry_kernels():
        for e in entries:
            e.enqueue()

    routes = {'per-image': per_image, 'per-entry': per_entry, 'from-conv': from_conv,
              'from-conv-kernels': ingested._ingests[0].enqueue,  # pylint: disable=protected-access
              'per-entry-kernels': entry_kernels, 'from-conv-default': from_conv_default}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, fn in routes.items():
            times[name].append(events(fn))
    read = sum(t.numel() * t.element_size() for row in convs.values() for t in row)
    written = 4 * sum(t.numel() for t in ingested.cifs + ingested.cafs)
    info = dict(info, case=case, dtype=dtype_name, images=n, heads=len(index),
                launches_per_image_route=n * len(index))
    med, lo, hi = {}, {}, {}
    for name, t in times.items():
        med[name], lo[name], hi[name] = statistics.median(t), min(t), max(t)
        line = dict(info, route=name, median_ms=round(med[name], 4), min_ms=round(lo[name], 4),
                    max_ms=round(hi[name], 4))
        if name.endswith('-kernels'):
            line.update(bytes_read=read, bytes_written=written,
                        tb_per_s=round((read + written) / med[name] / 1e9, 3))
        print(json.dumps(line), flush=True)
    spread = max(hi[k] - lo[k] for k in ('from-conv-kernels', 'per-entry-kernels'))
    print(json.dumps(dict(
        info, route='ratios',
        from_conv_over_per_image=round(med['from-conv'] / med['per-image'], 4),
        from_conv_over_per_entry=round(med['from-conv'] / med['per-entry'], 4),
        from_conv_default_over_per_image=round(med['from-conv-default'] / med['per-image'], 4),
        per_entry_kernels_minus_from_conv_kernels_ms=round(
            med['per-entry-kernels'] - med['from-conv-kernels'], 4),
        larger_spread_ms=round(spread, 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--images', type=int, default=64, help='the first N sizes (0: all)')
    ap.add_argument('--cases', default='ms2,ms10')
    ap.add_argument('--dtypes', default='float32,float16')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ragged_sizes.json')) as f:
        sizes = [tuple(s) for s in json.load(f)['sizes']]
    if args.images:
        sizes = sizes[:args.images]
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'runs': args.runs, 'warmup': args.warmup, 'clock': 'events', 'quad': 0}
    for case in args.cases.split(','):
        for dtype_name in args.dtypes.split(','):
            run_case(case, sizes, dtype_name, args, info)


if __name__ == '__main__':
    main()
