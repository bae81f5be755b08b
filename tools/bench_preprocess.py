"""Eval preprocessing on the device: 256 images of 480x640, long_edge 641, CenterPad.

    python tools/bench_preprocess.py [--runs 20] [--warmup 3] [--images 256]

The images are seeded random uint8.  Two outputs: float32 planar and bfloat16 channels-last.
Per output, HIP events on the current stream, --warmup runs first, median and min-max of
--runs, one JSON line per route:

  launch   pp_preprocess_images alone over the gathered source buffer (the staged tables and
           the kernel).  bytes = the source bytes plus the output bytes, each counted once;
           tb_per_s = bytes over the median; roofline = tb_per_s over the 8 TB/s HBM figure
  device   EvalPreprocess.batch of device tensors (planning and metas on the host, the
           gather on the device, the launch)
  host     EvalPreprocess.batch of host arrays (pinned staging and one host-to-device copy
           besides)
and one line for the host: the per-image time of the reference's chain on one core for the
same image (`scipy-chain`: scipy.ndimage.zoom, a constant-fill paste, ToTensor and Normalize
as torch ops) when scipy imports, else the host twin's (`host-twin`).  The device output is
compared with the host twin's on four images before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, preprocess  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.transforms import EvalPreprocess  # noqa: E402  pylint: disable=wrong-import-position

H, W, LONG_EDGE = 480, 640, 641
HBM_TB_PER_S = 8.0


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_chain(image):
    """Seconds per image of the host route and its label."""
    try:
        import scipy.ndimage  # pylint: disable=import-outside-toplevel
    except ImportError:
        pp = EvalPreprocess(LONG_EDGE)
        pp.batch_cpu([image])
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            pp.batch_cpu([image])
            t.append(time.perf_counter() - t0)
        return statistics.median(t), 'host-twin'
    torch.set_num_threads(1)
    th, tw = preprocess.rescaled_size(H, W, LONG_EDGE)
    left, top, _, _ = preprocess.center_pad(th, tw, LONG_EDGE, LONG_EDGE)
    mean = torch.tensor(preprocess.MEAN)[:, None, None]
    std = torch.tensor(preprocess.STD)[:, None, None]

    def chain():
        im = scipy.ndimage.zoom(image, (th / H, tw / W, 1), order=1)
        out = np.empty((LONG_EDGE, LONG_EDGE, 3), np.uint8)
        out[:] = np.uint8(preprocess.FILL)
        out[top:top + th, left:left + tw] = im
        return torch.from_numpy(out).permute(2, 0, 1).contiguous().float().div(255) \
            .sub_(mean).div_(std)

    chain()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        chain()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), 'scipy-chain'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--images', type=int, default=256)
    args = ap.parse_args()
    dev = _device.require()
    rng = np.random.default_rng(3)
    n = args.images
    host_images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    dev_images = [torch.from_numpy(im).to(dev) for im in host_images]
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'images': n, 'source': [H, W], 'long_edge': LONG_EDGE, 'runs': args.runs,
            'warmup': args.warmup, 'clock': 'events'}

    for dtype, channels_last in ((torch.float32, False), (torch.bfloat16, True)):
        pp = EvalPreprocess(LONG_EDGE, dtype=dtype, channels_last=channels_last)
        got, _ = pp.batch(dev_images[:4])
        want, _ = pp.batch_cpu(host_images[:4])
        g = got.contiguous().cpu()
        g = g.view(torch.int16).numpy().astype(np.uint16) if dtype == torch.bfloat16 else g.numpy()
        assert np.array_equal(g.view(want.dtype), np.ascontiguousarray(want)), 'device != host twin'

        _, _, rows, offsets, src_bytes, out_elems, _ = pp._plan(dev_images, None)
        descs = preprocess.image_descs(rows, offsets)
        out_bytes = out_elems * torch.empty(0, dtype=dtype).element_size()
        pp.batch(dev_images)  # gathers the source buffer and sizes the kept output
        routes = {'launch': lambda: pp._launch_descs(descs, src_bytes, pp._out, out_elems),
                  'device': lambda: pp.batch(dev_images),
                  'host': lambda: pp.batch(host_images)}
        for _ in range(args.warmup):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():
                times[name].append(events(fn))
        for name, t in times.items():
            med = statistics.median(t)
            line = dict(info, route=name, dtype=str(dtype).replace('torch.', ''),
                        channels_last=channels_last, median_ms=round(med, 4),
                        min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                        images_per_s=round(n / med * 1e3, 1),
                        us_per_image=round(med / n * 1e3, 3))
            if name == 'launch':
                tb = (src_bytes + out_bytes) / med / 1e9
                line.update(bytes=src_bytes + out_bytes, tb_per_s=round(tb, 3),
                            roofline=round(tb / HBM_TB_PER_S, 4))
            print(json.dumps(line), flush=True)

    sec, label = host_chain(host_images[0])
    print(json.dumps(dict(info, route=label, threads=1, ms_per_image=round(sec * 1e3, 3))),
          flush=True)


if __name__ == '__main__':
    main()
