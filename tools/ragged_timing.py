"""Ragged batches: 256 planted images of mixed field sizes, decoded three ways.

    python tools/ragged_timing.py [--runs 20] [--warmup 3]

The sizes (tools/ragged_sizes.json, fixed) follow the aspect ratios of long-edge-641
inputs: the long side 81 cells, the short one 41 to 81.  Image i is
synthetic.generate('planted', h_i, w_i, seed i), COCO skeleton, eval defaults.  HIP events
around each route on the current stream, --warmup runs first, the routes in alternation,
median and min-max of --runs (>= 20).  One JSON line per route:

  ragged      (a) engine.RaggedFields (the pack of both containers) + the checked decode
              (pp_decode_ragged, overflow check included)
  pack        the pack alone (RaggedFields: tables, allocations and both launches)
  pack-kernels  its two launches alone (RaggedFields.pack), with their bytes (sources read +
              containers written) per second
  per-image   (b) the same images one checked decode_batch launch sequence each, every
              shape with an engine (workspace) of its own, so no route allocates
  ceiling     (c) a uniform 81x81 planted batch of 256, one checked decode
and a last line with the ratios a / b and a / c.  The ragged route's records are compared
with the per-image route's before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, constants, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._abi import EVAL_CONFIG, make_config  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import DecodeEngine, RaggedFields  # noqa: E402  pylint: disable=wrong-import-position

SKEL = constants.COCO_PERSON_SKELETON


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ragged_sizes.json')) as f:
        sizes = [tuple(s) for s in json.load(f)['sizes']]
    n = len(sizes)
    cfg = make_config(**EVAL_CONFIG)
    fields = []
    for i, (h, w) in enumerate(sizes):
        cif, caf = synthetic.generate('planted', h, w, i, skeleton=SKEL)
        fields.append((_device.to_device(cif), _device.to_device(caf)))
    cif81, caf81 = (_device.to_device(a) for a in synthetic.batch('planted', n, 81, 81))

    eng = DecodeEngine()
    per_shape = {s: DecodeEngine() for s in set(sizes)}
    ceiling_eng = DecodeEngine()

    def ragged():
        return eng.launch_checked(None, None, SKEL, cfg, ragged=RaggedFields(fields))

    def per_image():
        return [per_shape[s].launch_checked(cif[None], caf[None], SKEL, cfg)
                for s, (cif, caf) in zip(sizes, fields)]

    def ceiling():
        return ceiling_eng.launch_checked(cif81, caf81, SKEL, cfg)

    # the routes agree before they are timed
    recs, offsets = DecodeEngine.fetch(ragged())
    for i, (s, (cif, caf)) in enumerate(zip(sizes, fields)):
        one, _ = DecodeEngine.fetch(per_shape[s].launch_checked(cif[None], caf[None], SKEL, cfg))
        got = recs[offsets[i]:offsets[i + 1]]
        assert len(got) == len(one), (i, len(got), len(one))
        for name in ('data', 'joint_scales', 'score', 'decoding_pairs', 'decoding_xyv'):
            assert got[name].tobytes() == one[name].tobytes(), (i, name)
    planes = 17 * 5 + len(SKEL) * 9
    pack_bytes = 4 * planes * (sum(h * w for h, w in sizes) + n * 81 * 81)

    packed = RaggedFields(fields)
    routes = {'ragged': ragged, 'pack': lambda: RaggedFields(fields), 'pack-kernels': packed.pack,
              'per-image': per_image, 'ceiling': ceiling}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, fn in routes.items():
            times[name].append(events(fn))
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'images': n, 'annotations': int(offsets[-1]), 'runs': args.runs,
            'warmup': args.warmup, 'clock': 'events'}
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        line = dict(info, route=name, median_ms=round(med[name], 4), min_ms=round(min(t), 4),
                    max_ms=round(max(t), 4),
                    images_per_s=None if name.startswith('pack') else round(n / med[name] * 1e3, 1))
        if name == 'pack-kernels':
            line.update(bytes=pack_bytes, tb_per_s=round(pack_bytes / med[name] / 1e9, 3))
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(info, route='ratios',
                          ragged_over_per_image=round(med['ragged'] / med['per-image'], 4),
                          ragged_over_ceiling=round(med['ragged'] / med['ceiling'], 4),
                          speedup_over_per_image=round(med['per-image'] / med['ragged'], 2))),
          flush=True)


if __name__ == '__main__':
    main()
