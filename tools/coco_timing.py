"""COCO prediction records: time from a finished decode to finished records, per batch.

    python tools/coco_timing.py [--runs 21] [--images 256] [--size 80]

A planted batch (--images images of --size x --size cells, COCO skeleton, eval defaults) is
decoded once; every route below then starts from that decode's device records.  Wall clock
around work that ends in a synchronisation, warm-up first, the routes in alternation, median
and min-max of --runs (>= 20).  One JSON line per route.

  per-image   what the library offered before: fetch the records (compact, as decode_batch
              does), build the Annotation lists, eval_coco.coco_predictions image by image
              (two copies and one synchronisation per image)
  batch       DecodeEngine.fetch_coco_async(...).result(), metas_device included: the
              CocoRecords (structured array in pinned memory)
  batch+dicts the same plus CocoRecords.predictions() (the list of dicts)
  launches    pp_coco_keypoints alone (both launches) by HIP events, records written to
              device memory (`device`) or to mapped pinned memory (`pinned`)
  inverse     transforms.inverse_records (pp_annotations_inverse, in place) by HIP events, on
              a fresh device copy of the records made before the first event
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _abi, _device, constants, decoder, eval_coco, synthetic, transforms  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._lib import call, load  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import engine  # noqa: E402  pylint: disable=wrong-import-position


def metas_for(n):
    base = {'offset': np.array((3.5, -2.25)), 'scale': np.array((0.5, 0.75)),
            'rotation': {'angle': 0.0, 'width': None, 'height': None}, 'hflip': False,
            'width_height': np.array((641, 427))}
    swap = transforms._HorizontalSwap(constants.COCO_KEYPOINTS, constants.HFLIP)
    kinds = [base, dict(base, hflip=True, horizontal_swap=swap),
             dict(base, rotation={'angle': 12.5, 'width': 481, 'height': 361},
                  offset=np.array((-1.0, 4.5)), scale=np.array((1.25, 0.8)))]
    return [dict(kinds[i % 3], image_id=1000 + i) for i in range(n)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--size', type=int, default=80)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    _device.require()
    decoder.CifHr.v_threshold = 0.1
    decoder.CafScored.default_score_th = 0.1
    decoder.CifSeeds.threshold = 0.2
    decoder.CifCaf.force_complete = True
    dec = decoder.CifCaf(decoder.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                         skeleton=constants.COCO_PERSON_SKELETON)
    n, k = args.images, 17
    cif, caf = synthetic.batch('planted', n, args.size, args.size)
    cif, caf = _device.to_device(cif), _device.to_device(caf)
    metas = metas_for(n)
    skel, cfg = _abi.skeleton_array(dec.skeleton), dec.config()
    b = engine().launch_checked(cif, caf, skel, cfg)
    torch.cuda.synchronize()

    def per_image():
        recs, offsets = engine().fetch(b, (k, len(skel), _abi.PACK_ALL))
        out = []
        for anns, m in zip(dec.annotations_from_records(recs, offsets), metas):
            out += eval_coco.coco_predictions(anns, m)
        return out

    def batch():
        d_metas, d_ids, d_swap = eval_coco.metas_device(metas, k)
        return engine().fetch_coco_async(b, d_metas, d_ids, hswap=d_swap).result()

    want = per_image()
    got = batch()
    assert json.dumps(got.predictions()) == json.dumps(want), 'the routes disagree'

    d_metas, d_ids, d_swap = eval_coco.metas_device(metas, k)
    width = _abi.coco_dtype(k).itemsize
    est = 20 * n
    params = _abi.CocoParams(0.0, 20, 1)
    ws = torch.empty(int(load().pp_coco_workspace_size(n)), dtype=torch.uint8, device='cuda')
    heads = {'device': torch.empty(8 * n, dtype=torch.uint8, device='cuda'),
             'pinned': torch.empty(8 * n, dtype=torch.uint8, pin_memory=True)}
    outs = {'device': torch.empty(est * width, dtype=torch.uint8, device='cuda'),
            'pinned': torch.empty(est * width, dtype=torch.uint8, pin_memory=True)}

    def launches(where):
        h, o = heads[where], outs[where]
        call('pp_coco_keypoints', _device.ptr(b.anns), _device.ptr(b.counts), n, b.cap, k,
             _device.ptr(d_metas), _device.ptr(d_ids), _device.ptr(d_swap), ctypes.byref(params),
             ctypes.c_void_p(o.data_ptr()), est, ctypes.c_void_p(h.data_ptr()),
             ctypes.c_void_p(h.data_ptr() + 4 * n), _device.ptr(ws), _device.stream())

    def events_on_copy(fn):
        recs = b.anns.view(n, b.cap, -1).clone()  # made before the first event
        return events(lambda: fn(recs))

    routes = {
        'per-image': (wall, per_image),
        'batch': (wall, batch),
        'batch+dicts': (wall, lambda: batch().predictions()),
        'launches-device': (events, lambda: launches('device')),
        'launches-pinned': (events, lambda: launches('pinned')),
        'inverse': (events_on_copy, lambda recs: transforms.inverse_records(
            recs, b.counts, d_metas, k=k, hswap=d_swap)),
    }
    for _ in range(2):
        for clock, fn in routes.values():
            clock(fn)
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.runs):
        for name, (clock, fn) in routes.items():
            times[name].append(clock(fn))
    info = {'device': torch.cuda.get_device_name(0), 'images': n, 'size': args.size,
            'runs': args.runs, 'records': len(want), 'input_records': int(b.counts.sum())}
    for name, t in times.items():
        print(json.dumps(dict(info, route=name, clock=routes[name][0].__name__,
                              median_ms=round(statistics.median(t), 4),
                              min_ms=round(min(t), 4), max_ms=round(max(t), 4))), flush=True)


if __name__ == '__main__':
    main()
