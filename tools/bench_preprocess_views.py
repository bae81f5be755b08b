"""The ten inputs of a multi-scale model on the device: 256 images of 480x640, long_edge 641,
CenterPad, the five reductions and their mirror images.

    python tools/bench_preprocess_views.py [--runs 20] [--warmup 3] [--images 256] [--reps 3]
                                           [--out profiles/preprocess_views_bench.jsonl]

The images are seeded random uint8 device tensors.  Two outputs: float32 planar and bfloat16
channels-last.  Two routes to the same ten contiguous tensors, compared bit for bit before
anything is timed:

  sliced   what was there before EvalViews: EvalPreprocess.batch, then the slicing, mask
           indexing and flip of network/nets.py:116-128 as torch operations, each result made
           contiguous (the baseline; it does not run the code under test)
  views    EvalViews.batch: one pp_preprocess_views launch
  launch   pp_preprocess_views alone over the gathered source buffer (the staged tables and
           the kernel).  bytes = the source bytes plus the bytes of the ten views, each
           counted once; tb_per_s = bytes over the median; roofline = tb_per_s over the
           8 TB/s HBM figure
  launch_rot1  the same launch with every image turned by 90 degrees (rot = 1), where a
           wave's source reads run down a column of the source image

Per route HIP events on the current stream, --warmup runs first, then the median and min-max
of --runs; the routes alternate and the whole round is repeated --reps times, one JSON line
per route and round.  A last line per output gives sliced over views from the medians of the
rounds and the spread of each route between its rounds: the ratio counts as a speed-up only
where it exceeds those spreads.  The lines are printed and written to --out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.transforms import EvalPreprocess, EvalViews  # noqa: E402  pylint: disable=wrong-import-position

H, W, LONG_EDGE = 480, 640, 641
HBM_TB_PER_S = 8.0
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def sliced(x):
    """nets.py:116-128 on the normalised input, every result contiguous (bool masks where the
    reference has ByteTensor masks)."""
    out = []
    for flip in (False, True):
        for reduction in [1, 1.5, 2, 3, 5]:
            if reduction == 1.5:
                x_red = torch.tensor([i % 3 != 2 for i in range(x.shape[3])], device=x.device)
                y_red = torch.tensor([i % 3 != 2 for i in range(x.shape[2])], device=x.device)
                reduced = x[:, :, y_red, :]
                reduced = reduced[:, :, :, x_red]
            else:
                reduced = x[:, :, ::reduction, ::reduction]
            if flip:
                reduced = torch.flip(reduced, dims=[3])
            fmt = torch.channels_last if x.stride(1) == 1 else torch.contiguous_format
            out.append(reduced.contiguous(memory_format=fmt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'preprocess_views_bench.jsonl'))
    args = ap.parse_args()
    dev = _device.require()
    rng = np.random.default_rng(3)
    n = args.images
    dev_images = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
                  for _ in range(n)]
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'images': n, 'source': [H, W], 'long_edge': LONG_EDGE, 'runs': args.runs,
            'warmup': args.warmup, 'clock': 'events'}
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    for dtype, channels_last in ((torch.float32, False), (torch.bfloat16, True)):
        base = EvalPreprocess(LONG_EDGE, dtype=dtype, channels_last=channels_last)
        pp = EvalViews(LONG_EDGE, multi_scale=True, dtype=dtype, channels_last=channels_last)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        want = sliced(base.batch(dev_images[:4])[0])
        got, _ = pp.batch(dev_images[:4])
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.stride() == w.stride(), 'views != sliced (layout)'
            assert torch.equal(g.contiguous().view(bits), w.contiguous().view(bits)), \
                'views != sliced'
        del want, got

        _, _, descs, offsets, src_bytes, out_elems, _ = pp._plan(dev_images, None)
        out_bytes = out_elems * torch.empty(0, dtype=dtype).element_size()
        turned = descs.copy()
        turned['rot'] = 1
        pp.batch(dev_images)  # gathers the source buffer and sizes the kept output
        routes = {'sliced': lambda: sliced(base.batch(dev_images)[0]),
                  'views': lambda: pp.batch(dev_images),
                  'launch': lambda: pp._launch(descs, offsets, src_bytes, pp._out, out_elems),
                  'launch_rot1': lambda: pp._launch(turned, offsets, src_bytes, pp._out,
                                                    out_elems)}
        medians = {name: [] for name in routes}
        for rep in range(args.reps):
            for name, fn in routes.items():
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                t = [events(fn) for _ in range(args.runs)]
                med = statistics.median(t)
                medians[name].append(med)
                line = dict(info, route=name, round=rep, dtype=str(dtype).replace('torch.', ''),
                            channels_last=channels_last, median_ms=round(med, 4),
                            min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                            us_per_image=round(med / n * 1e3, 3))
                if name.startswith('launch'):
                    tb = (src_bytes + out_bytes) / med / 1e9
                    line.update(bytes=src_bytes + out_bytes, tb_per_s=round(tb, 3),
                                roofline=round(tb / HBM_TB_PER_S, 4))
                emit(line)
        spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in medians.items()}
        emit(dict(info, route='sliced/views', dtype=str(dtype).replace('torch.', ''),
                  channels_last=channels_last,
                  ratio=round(statistics.median(medians['sliced']) /
                              statistics.median(medians['views']), 3),
                  ratio_min=round(min(medians['sliced']) / max(medians['views']), 3),
                  spread_between_rounds=spread))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
