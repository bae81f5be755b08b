"""CIF / CAF target encoders: time per batch on the device and on the host twin.

    python tools/encoder_timing.py [--images 256] [--size 80] [--people 8] [--threads 16]
    python tools/encoder_timing.py --reference 8      # build container only, no GPU

The workload: --images images of --size x --size cells at stride 8, --people people each
(the upright COCO pose at seeded places and sizes), COCO skeleton and sigmas.  Per encoder,
one JSON line:

  device_ms   HIP events around the staging copy and the launch of one batch, the call made
              while the stream spins so that no host work lies between them (3 warm-ups,
              median and min-max of --runs >= 20)
  call_ms     wall clock of `Cif.batch` / `Caf.batch` on an idle stream up to a
              synchronisation: the Python marshalling and the library's host plan included
  twin_ms     wall clock of `batch_cpu` on --threads host threads
  tb_per_s    bytes of the batch's tensors / device_ms (a plain float32 store stream
              reaches 6.0-6.2 TB/s on this card)

--reference N measures, on the CPU alone, the reference's own encoders (imported through
oracle/ref_loader.py) against the twin on one thread over N images of the workload, and
prints the per-image times and their ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, REPO)

from openpifpaf_amd import constants, encoder  # noqa: E402  pylint: disable=wrong-import-position

COCO_SIGMAS = [0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062,
               0.107, 0.107, 0.087, 0.087, 0.089, 0.089]
STRIDE = 8


def scene(size_px, n_people, seed):
    rng = np.random.default_rng(seed)
    pose = constants.COCO_UPRIGHT_POSE
    anns = []
    for _ in range(n_people):
        unit = rng.uniform(0.02, 0.07) * size_px
        cx, cy = rng.uniform(0.1, 0.9) * size_px, rng.uniform(0.05, 0.5) * size_px
        kps = np.zeros((17, 3), np.float32)
        kps[:, 0] = cx + unit * pose[:, 0] + rng.normal(0.0, 0.02 * unit, 17)
        kps[:, 1] = cy - unit * (pose[:, 1] - 10.0) + rng.normal(0.0, 0.02 * unit, 17)
        kps[:, 2] = 2.0
        x0, y0 = kps[:, 0].min(), kps[:, 1].min()
        bbox = np.array([x0, y0, kps[:, 0].max() - x0, kps[:, 1].max() - y0], np.float32)
        anns.append({'keypoints': kps, 'bbox': bbox, 'iscrowd': False})
    meta = {'valid_area': np.array([0.0, 0.0, size_px - 1.0, size_px - 1.0])}
    return (size_px, size_px), anns, meta


def encoders(module):
    rescaler = module.AnnRescaler(STRIDE, 17, np.array(constants.COCO_UPRIGHT_POSE, np.float64))
    return {'cif': module.Cif(rescaler, sigmas=COCO_SIGMAS),
            'caf': module.Caf(rescaler, skeleton=constants.COCO_PERSON_SKELETON,
                              sigmas=COCO_SIGMAS)}


def summary(ms):
    return {'median': round(statistics.median(ms), 4), 'min': round(min(ms), 4),
            'max': round(max(ms), 4)}


def device_run(args, scenes):
    import torch  # pylint: disable=import-outside-toplevel
    sizes, anns, metas = zip(*scenes)
    # cycles of torch.cuda._sleep per millisecond, by events
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(20_000_000)
    e1.record()
    torch.cuda.synchronize()
    cycles_per_ms = 20_000_000 / e0.elapsed_time(e1)
    for which, enc in encoders(encoder).items():
        call_ms, dev_ms, twin_ms = [], [], []
        for run in range(args.warmup + args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = enc.batch(sizes, anns, metas)
            torch.cuda.synchronize()
            if run >= args.warmup:
                call_ms.append((time.perf_counter() - t0) * 1e3)
        # the staging copy and the kernel alone: the call is made while the stream spins, so
        # the marshalling and the host plan are over before the first event is reached
        spin = int(2.0 * max(call_ms) * cycles_per_ms)
        for run in range(args.warmup + args.runs):
            torch.cuda.synchronize()
            torch.cuda._sleep(spin)
            e0.record()
            enc.batch(sizes, anns, metas)
            e1.record()
            torch.cuda.synchronize()
            if run >= args.warmup:
                dev_ms.append(e0.elapsed_time(e1))
        for run in range(1 + 5):
            t0 = time.perf_counter()
            enc.batch_cpu(sizes, anns, metas, n_threads=args.threads)
            if run:
                twin_ms.append((time.perf_counter() - t0) * 1e3)
        n_bytes = 4 * sum(t.numel() for t in out)
        line = {'encoder': which, 'images': len(scenes), 'field': args.size,
                'people': args.people, 'device_ms': summary(dev_ms), 'call_ms': summary(call_ms),
                'twin_ms': dict(summary(twin_ms), threads=args.threads), 'bytes': n_bytes,
                'tb_per_s': round(n_bytes / (statistics.median(dev_ms) * 1e-3) / 1e12, 3),
                'twin_over_device': round(statistics.median(twin_ms) /
                                          statistics.median(dev_ms), 1),
                'twin_over_call': round(statistics.median(twin_ms) /
                                        statistics.median(call_ms), 1)}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')


def reference_run(args, scenes):
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    for alias, typ in (('int', int), ('bool', bool)):
        if not hasattr(np, alias):
            setattr(np, alias, typ)
    import ref_loader  # pylint: disable=import-outside-toplevel
    ref_loader.load()
    from openpifpaf import encoder as ref_encoder  # pylint: disable=import-outside-toplevel

    class NoVisualizer:
        def processed_image(self, image):
            pass

        def targets(self, fields, *, keypoint_sets):
            pass
    ours, theirs = encoders(encoder), encoders(ref_encoder)
    for which in ('cif', 'caf'):
        theirs[which].visualizer = NoVisualizer()
        ref_ms, twin_ms = [], []
        for size, anns, meta in scenes[:args.reference]:
            image = np.zeros((3,) + size, np.float32)
            t0 = time.perf_counter()
            theirs[which](image, anns, meta)
            t1 = time.perf_counter()
            ours[which].batch_cpu([size], [anns], [meta], n_threads=1)
            t2 = time.perf_counter()
            ref_ms.append((t1 - t0) * 1e3)
            twin_ms.append((t2 - t1) * 1e3)
        line = {'encoder': which, 'reference_ms_per_image': summary(ref_ms),
                'twin_ms_per_image': summary(twin_ms),
                'reference_over_twin': round(statistics.median(ref_ms) /
                                             statistics.median(twin_ms), 2)}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(json.dumps(line) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--size', type=int, default=80)
    ap.add_argument('--people', type=int, default=8)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reference', type=int, default=0)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    size_px = (args.size - 1) * STRIDE + 1
    scenes = [scene(size_px, args.people, seed) for seed in range(args.images)]
    if args.reference:
        reference_run(args, scenes)
    else:
        device_run(args, scenes)


if __name__ == '__main__':
    main()
