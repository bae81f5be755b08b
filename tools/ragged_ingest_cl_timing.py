"""Channels-last conv outputs of 256 images of mixed sizes into a ragged batch's containers.

    python tools/ragged_ingest_cl_timing.py [--runs 21] [--warmup 3] [--dtypes float32,float16]

The workload of tools/ragged_ingest_timing.py (the 256 sizes of tools/ragged_sizes.json at quad
1, container 81x81, COCO CIF and CAF heads, planted fields turned back into conv outputs), each
image's conv a channels-last tensor of its own.  HIP events around each route on the current
stream, --warmup runs first, the routes in alternation, median and min-max of --runs.  One
JSON line per route and dtype:

  copy          (a) the route before pp_fields_from_conv_ragged_interleaved for these inputs:
                .contiguous() per image, then engine.RaggedFields.from_conv (planar symbol)
  in-place      (b) engine.RaggedFields.from_conv on the channels-last tensors
  in-place-kernels  (b') its two library calls alone, with bytes read + written per second
  dense         (c) one fields_from_conv (pp_fields_from_conv_strided) per head of a uniform
                dense channels-last (256, ch, 41, 41) batch
  planar-kernels, planar-dense  (b') and (c) of the NCHW form of the same values, the pair
                (b') against (c) is to be compared with
and a last line per dtype with (b) against (a) and both (b') / (c) ratios.  The containers of
(a) and (b) are compared byte for byte before anything is timed."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, constants, heads, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import RaggedFields  # noqa: E402  pylint: disable=wrong-import-position
from ragged_ingest_timing import QUAD, conv_from_fields, events  # noqa: E402  pylint: disable=wrong-import-position

SKEL = constants.COCO_PERSON_SKELETON


def channels_last(conv):
    """(ch, h, w) values in (h, w, ch) memory order, a tensor of its own"""
    ch, h, w = conv.shape
    out = torch.empty((h, w, ch), dtype=conv.dtype, device=conv.device).permute(2, 0, 1)
    out.copy_(conv)
    return out


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
        planar = ([torch.from_numpy(a).to('cuda', dtype) for a, _ in host],
                  [torch.from_numpy(b).to('cuda', dtype) for _, b in host])
        cifs, cafs = ([channels_last(c) for c in head] for head in planar)
        dense = (torch.randn((n, n_cif * 20, hmax, wmax), device='cuda').to(dtype),
                 torch.randn((n, n_caf * 36, hmax, wmax), device='cuda').to(dtype))
        dense_cl = tuple(d.contiguous(memory_format=torch.channels_last) for d in dense)
        dense_out = (torch.empty((n, n_cif, 5, big_h, big_w), device='cuda'),
                     torch.empty((n, n_caf, 9, big_h, big_w), device='cuda'))

        def copy_route():
            return RaggedFields.from_conv([c.contiguous() for c in cifs],
                                          [c.contiguous() for c in cafs], n_cif, n_caf, QUAD)

        def in_place():
            return RaggedFields.from_conv(cifs, cafs, n_cif, n_caf, QUAD)

        def dense_ingest(pair):
            heads.fields_from_conv(pair[0], n_cif, 'cif', QUAD, out=dense_out[0])
            heads.fields_from_conv(pair[1], n_caf, 'caf', QUAD, out=dense_out[1])

        # the routes agree before they are timed
        copied, ingested = copy_route(), in_place()
        from_planar = RaggedFields.from_conv(planar[0], planar[1], n_cif, n_caf, QUAD)
        assert (copied.h, copied.w) == (ingested.h, ingested.w) == (big_h, big_w)
        for other in (copied, from_planar):
            assert torch.equal(other.cif.view(torch.int32), ingested.cif.view(torch.int32))
            assert torch.equal(other.caf.view(torch.int32), ingested.caf.view(torch.int32))
            assert torch.equal(other.extents, ingested.extents)
        assert all(i.interleaved for i in ingested._ingests)  # pylint: disable=protected-access
        assert not any(i.interleaved for i in copied._ingests + from_planar._ingests)  # pylint: disable=protected-access

        def kernels(ragged):
            for ing in ragged._ingests:  # pylint: disable=protected-access
                ing.enqueue()

        routes = {
            'copy': copy_route, 'in-place': in_place,
            'in-place-kernels': lambda: kernels(ingested),
            'dense': lambda: dense_ingest(dense_cl),
            'planar-kernels': lambda: kernels(from_planar),
            'planar-dense': lambda: dense_ingest(dense),
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
                'runs': args.runs, 'warmup': args.warmup, 'clock': 'events'}
        med, lo, hi = {}, {}, {}
        for name, t in times.items():
            med[name], lo[name], hi[name] = statistics.median(t), min(t), max(t)
            line = dict(info, route=name, median_ms=round(med[name], 4),
                        min_ms=round(lo[name], 4), max_ms=round(hi[name], 4))
            if name in ('in-place-kernels', 'planar-kernels'):
                line.update(bytes_read=read, bytes_written=written,
                            gb_per_s=round((read + written) / med[name] / 1e6, 1))
            print(json.dumps(line), flush=True)
        spread = max(hi[k] - lo[k] for k in ('copy', 'in-place'))
        print(json.dumps(dict(
            info, route='ratios',
            copy_minus_in_place_ms=round(med['copy'] - med['in-place'], 4),
            larger_spread_ms=round(spread, 4),
            in_place_over_copy=round(med['in-place'] / med['copy'], 4),
            kernels_over_dense=round(med['in-place-kernels'] / med['dense'], 4),
            planar_kernels_over_planar_dense=round(
                med['planar-kernels'] / med['planar-dense'], 4))), flush=True)
        del planar, cifs, cafs, dense, dense_cl, dense_out, copied, ingested, from_planar, routes
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
