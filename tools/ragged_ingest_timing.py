"""Conv outputs of 256 images of mixed sizes into a ragged batch's containers, timed five ways.

    python tools/ragged_ingest_timing.py [--runs 21] [--warmup 3] [--dtypes float32,float16]

The sizes are those of tools/ragged_sizes.json at quad 1: a field side s comes from a conv
side (s + 1) // 2 and becomes 2 * ((s + 1) // 2) - 1.  COCO CIF (17) and CAF (19) heads.
Image i's conv is the inverse of the head's tail and of the dequad on
synthetic.generate('planted', H_i, W_i, seed i) at its field size, so that the ingested
fields are planted fields again and decode to poses.  HIP events around each route on the current
stream, --warmup runs first, the routes in alternation, median and min-max of --runs.  One
JSON line per route and dtype:

  per-image     (a) the route before pp_fields_from_conv_ragged: one fields_from_conv per
                image per head (512 calls), then engine.RaggedFields (the pack)
  from-conv     (b) engine.RaggedFields.from_conv: tables, allocations, both launches
  from-conv-kernels  (b') its two library calls alone, with bytes read + written per second
  dense         (c) one fields_from_conv per head of a uniform (256, ch, 41, 41) batch: the
                same stores, more loads
  pack-kernels  (d) the pack's two launches alone
  decode-per-image, decode-from-conv  (a) and (b) followed by the checked ragged decode
and a last line per dtype with (b') against (c) + (d) and (b) against (a).  The containers of
(a) and (b) are compared byte for byte before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, constants, heads, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._abi import EVAL_CONFIG, make_config  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import DecodeEngine, RaggedFields  # noqa: E402  pylint: disable=wrong-import-position

SKEL = constants.COCO_PERSON_SKELETON
QUAD = 1
PERM = {'cif': (0, 1, 2, 3, 4), 'caf': (0, 1, 2, 5, 7, 3, 4, 6, 8)}


def conv_from_fields(field, kind):
    """Fields (n_fields, 5 | 9, 2 h - 1, 2 w - 1) -> the quad-1 conv output (4 * channels, h, w)
    they are ingested from: the inverse of the head's tail (logit, minus the index grid, log),
    then of the dequad (field pixel (Y, X) of channel c lies at conv channel 4 c + 2 (Y & 1) +
    (X & 1), pixel (Y >> 1, X >> 1); the cropped row and column are 0)."""
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
    base = np.nan_to_num(np.concatenate([g.reshape(-1, h, w) for g in groups]))
    ch, hc, wc = len(base), (h + 1) // 2, (w + 1) // 2
    full = np.zeros((ch, 2 * hc, 2 * wc))
    full[:, :h, :w] = base
    conv = full.reshape(ch, hc, 2, wc, 2).transpose(0, 2, 4, 1, 3).reshape(4 * ch, hc, wc)
    return conv.astype(np.float32)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=21)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtypes', default='float32,float16')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ragged_sizes.json')) as f:
        sizes = [((h + 1) // 2, (w + 1) // 2) for h, w in json.load(f)['sizes']]
    n = len(sizes)
    cfg = make_config(**EVAL_CONFIG)
    host = []
    for i, (h, w) in enumerate(sizes):
        cif, caf = synthetic.generate('planted', 2 * h - 1, 2 * w - 1, i, skeleton=SKEL)
        host.append((conv_from_fields(cif, 'cif'), conv_from_fields(caf, 'caf')))
    n_cif, n_caf = 17, len(SKEL)
    planes = n_cif * 5 + n_caf * 9
    hmax, wmax = (max(s[d] for s in sizes) for d in (0, 1))
    big_h, big_w = heads.fields_dim(hmax, QUAD), heads.fields_dim(wmax, QUAD)
    for dtype_name in args.dtypes.split(','):
        dtype = getattr(torch, dtype_name)
        cifs = [torch.from_numpy(a).to('cuda', dtype) for a, _ in host]
        cafs = [torch.from_numpy(b).to('cuda', dtype) for _, b in host]
        dense = (torch.randn((n, n_cif * 20, hmax, wmax), device='cuda').to(dtype),
                 torch.randn((n, n_caf * 36, hmax, wmax), device='cuda').to(dtype))
        dense_out = (torch.empty((n, n_cif, 5, big_h, big_w), device='cuda'),
                     torch.empty((n, n_caf, 9, big_h, big_w), device='cuda'))
        eng_a, eng_b = DecodeEngine(), DecodeEngine()

        def per_image():
            return RaggedFields([(heads.fields_from_conv(c[None], n_cif, 'cif', QUAD)[0],
                                  heads.fields_from_conv(a[None], n_caf, 'caf', QUAD)[0])
                                 for c, a in zip(cifs, cafs)])

        def from_conv():
            return RaggedFields.from_conv(cifs, cafs, n_cif, n_caf, QUAD)

        def dense_ingest():
            heads.fields_from_conv(dense[0], n_cif, 'cif', QUAD, out=dense_out[0])
            heads.fields_from_conv(dense[1], n_caf, 'caf', QUAD, out=dense_out[1])

        # the routes agree before they are timed
        packed, ingested = per_image(), from_conv()
        assert (packed.h, packed.w) == (ingested.h, ingested.w) == (big_h, big_w)
        assert torch.equal(packed.cif.view(torch.int32), ingested.cif.view(torch.int32))
        assert torch.equal(packed.caf.view(torch.int32), ingested.caf.view(torch.int32))
        assert torch.equal(packed.extents, ingested.extents)
        _, offsets = DecodeEngine.fetch(eng_b.launch_checked(None, None, SKEL, cfg,
                                                             ragged=ingested))

        def kernels():
            for ing in ingested._ingests:  # pylint: disable=protected-access
                ing.enqueue()

        routes = {
            'per-image': per_image, 'from-conv': from_conv, 'from-conv-kernels': kernels,
            'dense': dense_ingest, 'pack-kernels': packed.pack,
            'decode-per-image': lambda: eng_a.launch_checked(None, None, SKEL, cfg,
                                                             ragged=per_image()),
            'decode-from-conv': lambda: eng_b.launch_checked(None, None, SKEL, cfg,
                                                             ragged=from_conv()),
        }
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():
                times[name].append(events(fn))
        elem = cifs[0].element_size()
        read = elem * 4 * planes * sum(h * w for h, w in sizes)
        written = 4 * planes * n * big_h * big_w
        info = {'device': torch.cuda.get_device_name(0), 'src_sha': build.source_digest(),
                'dtype': dtype_name, 'images': n, 'container': [big_h, big_w],
                'annotations': int(offsets[-1]), 'runs': args.runs, 'warmup': args.warmup,
                'clock': 'events'}
        med, lo, hi = {}, {}, {}
        for name, t in times.items():
            med[name], lo[name], hi[name] = statistics.median(t), min(t), max(t)
            line = dict(info, route=name, median_ms=round(med[name], 4),
                        min_ms=round(lo[name], 4), max_ms=round(hi[name], 4))
            if name == 'from-conv-kernels':
                line.update(bytes_read=read, bytes_written=written,
                            gb_per_s=round((read + written) / med[name] / 1e6, 1))
            print(json.dumps(line), flush=True)
        spread = max(hi[k] - lo[k] for k in ('dense', 'pack-kernels'))
        print(json.dumps(dict(
            info, route='ratios',
            dense_plus_pack_ms=round(med['dense'] + med['pack-kernels'], 4),
            from_conv_kernels_ms=round(med['from-conv-kernels'], 4),
            margin_ms=round(med['dense'] + med['pack-kernels'] - med['from-conv-kernels'], 4),
            larger_spread_ms=round(spread, 4),
            from_conv_over_per_image=round(med['from-conv'] / med['per-image'], 4),
            decode_from_conv_over_per_image=round(
                med['decode-from-conv'] / med['decode-per-image'], 4))), flush=True)
        del cifs, cafs, dense, dense_out, packed, ingested, routes
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
