"""CifDet timing: the uniform entry point against a parent build, and the ragged route.

    python tools/cifdet_timing.py --baseline-lib PATH [--new-first] [--runs 21] [--images 256]
    python tools/cifdet_timing.py --ragged [--runs 21]
    python tools/cifdet_timing.py --fetch [--baseline-package DIR] [--runs 21] [--batches 20]

--baseline-lib and --ragged: HIP events around each call on the current stream, 3 warm-ups first, the cases of a group in
alternation, median and min-max of --runs (>= 20).  One JSON line per case.  3 categories,
CifHr.v_threshold 0.1, seed threshold 0.3 (planted, synthetic.det_planted) or 0.1 (uniform,
synthetic.det_uniform).

--baseline-lib: pp_cifdet_decode of a libpifpaf_amd.so built from the commit to compare
against and of this build, through ctypes on the same 256 images of 80x80, each library with
the workspace its own pp_cifdet_workspace_size asks for.  The records of the two are compared
before anything is timed.

--ragged: the 256 sizes of tools/ragged_sizes.json (long side 81 cells), three routes:
  ragged      (a) engine.RaggedDetFields (tables, container, the pack launch) + the checked
              decode (pp_cifdet_decode_ragged, overflow check included)
  per-image   (b) one checked CifDet.decode_device per image, every shape with a CifDet
              (workspace) of its own, so no route allocates a workspace
  ceiling     (c) one checked uniform decode_device of 256 images of 81x81
and a last line with the ratios a / b and a / c.  The ragged route's records are compared with
the per-image route's before anything is timed.

--fetch: the user-facing call, CifDet.decode_records on the 256 images of 80x80 (decode, record
hand-over to the host and every synchronisation the call makes).  The path under test is host
work and PCIe, so the clock is wall time around the call (time.perf_counter, the device idle
before it), not HIP events.  With --baseline-package DIR (a checkout of the commit to compare
against, built: DIR/openpifpaf_amd with its own libpifpaf_amd.so) that package is loaded
beside this one under another name and the two alternate, parent first and then new first;
their records are compared before anything is timed.  Then, this build only: --batches
batches through engine.DetPipeline (all submitted, then all read) against the same number of
sequential decode_records calls, alternating, per batch."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), '..')))

from openpifpaf_amd import _device, build, decoder, synthetic  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._abi import DET_DTYPE, make_config  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd._lib import _SIGNATURES, load  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.decoder.generator.cifdet import det_nms_config  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd.engine import RaggedDetFields  # noqa: E402  pylint: disable=wrong-import-position

K, H, W = 3, 80, 80
SEED_THRESHOLD = {'planted': 0.3, 'uniform': 0.1}


def events(fn):
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
            times[name].append(events(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def decode_symbol(lib, n, cap, cfg):
    """pp_cifdet_decode of `lib` on (n, K, 7, H, W) fields with buffers of its own; ->
    (callable(det), records of the last call as (out, counts))."""
    for name in ('pp_cifdet_decode', 'pp_cifdet_workspace_size'):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _SIGNATURES[name]
    z = det_nms_config()
    ws = torch.empty(int(lib.pp_cifdet_workspace_size(n, K, H, W, ctypes.byref(cfg), cap)),
                     dtype=torch.uint8, device='cuda')
    out = torch.empty((n, cap, DET_DTYPE.itemsize), dtype=torch.uint8, device='cuda')
    counts = torch.empty(n, dtype=torch.int32, device='cuda')
    status = torch.empty(n, dtype=torch.int32, device='cuda')

    def decode(det):
        rc = lib.pp_cifdet_decode(det.data_ptr(), n, K, H, W, ctypes.byref(cfg), ctypes.byref(z),
                                  None, out.data_ptr(), cap, counts.data_ptr(), status.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _device.stream())
        assert rc == 0, rc
    return decode, (out, counts, status), ws.numel()


def against_parent(args, info):
    base_lib = ctypes.CDLL(os.path.abspath(args.baseline_lib))
    n, cap = args.images, H * W
    for kind in ('planted', 'uniform'):
        cfg = make_config(cif_threshold=0.1, seed_threshold=SEED_THRESHOLD[kind])
        det = _device.to_device(synthetic.det_batch(kind, n, H, W, n_categories=K))
        new, new_out, new_ws = decode_symbol(load(), n, cap, cfg)
        old, old_out, old_ws = decode_symbol(base_lib, n, cap, cfg)
        new(det)
        old(det)
        torch.cuda.synchronize()
        assert not new_out[2].any() and not old_out[2].any()
        assert torch.equal(new_out[1], old_out[1])
        cnt = new_out[1].cpu().numpy()
        a, b = new_out[0].cpu().numpy(), old_out[0].cpu().numpy()
        assert all(a[i, :cnt[i]].tobytes() == b[i, :cnt[i]].tobytes() for i in range(n))
        cases = {'parent': lambda: old(det), 'new': lambda: new(det)}
        if args.new_first:
            cases = dict(reversed(list(cases.items())))
        res = run_group(cases, args.runs)
        for case, (med, lo, hi) in res.items():
            print(json.dumps(dict(info, group='uniform-entry', kind=kind, case=case, images=n,
                                  first='new' if args.new_first else 'parent',
                                  detections=int(cnt.sum()),
                                  workspace_bytes=old_ws if case == 'parent' else new_ws,
                                  median_ms=round(med, 4), min_ms=round(lo, 4),
                                  max_ms=round(hi, 4))), flush=True)
        inside = res['parent'][1] <= res['new'][0] <= res['parent'][2]
        print(json.dumps(dict(info, group='uniform-entry', kind=kind, case='verdict',
                              new_over_parent=round(res['new'][0] / res['parent'][0], 4),
                              new_median_inside_parent_range=bool(inside))), flush=True)
        del det, new, old, new_out, old_out
        torch.cuda.empty_cache()


def ragged_routes(args, info):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ragged_sizes.json')) as f:
        sizes = [tuple(s) for s in json.load(f)['sizes']]
    n = len(sizes)
    hmax, wmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    cats = ['c%d' % i for i in range(K)]
    decoder.CifHr.v_threshold = 0.1
    for kind in ('planted', 'uniform'):
        decoder.CifSeeds.threshold = SEED_THRESHOLD[kind]
        gen = {'planted': synthetic.det_planted, 'uniform': synthetic.det_uniform}[kind]
        fields = [_device.to_device(gen(h, w, n_categories=K, seed=i))
                  for i, (h, w) in enumerate(sizes)]
        full = _device.to_device(synthetic.det_batch(kind, n, hmax, wmax, n_categories=K))
        cd = decoder.CifDet(decoder.FieldConfig(), cats)
        per_shape = {s: decoder.CifDet(decoder.FieldConfig(), cats) for s in set(sizes)}
        ceiling_cd = decoder.CifDet(decoder.FieldConfig(), cats)

        def ragged():
            return cd.decode_ragged_device(RaggedDetFields(fields))

        def per_image():
            return [per_shape[s].decode_device(f[None]) for s, f in zip(sizes, fields)]

        def ceiling():
            return ceiling_cd.decode_device(full)

        out, counts = ragged()
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
        for i, (one, cnt) in enumerate(per_image()):
            assert int(cnt[0]) == counts[i], (i, int(cnt[0]), counts[i])
            got = np.frombuffer(out[i, :counts[i]].tobytes(), dtype=DET_DTYPE)
            want = np.frombuffer(one.cpu().numpy()[0, :counts[i]].tobytes(), dtype=DET_DTYPE)
            for name in ('field', 'score', 'bbox'):
                assert got[name].tobytes() == want[name].tobytes(), (i, name)
        res = run_group({'ragged': ragged, 'per-image': per_image, 'ceiling': ceiling}, args.runs)
        for route, (med, lo, hi) in res.items():
            print(json.dumps(dict(info, group='ragged', kind=kind, route=route, images=n,
                                  container=[hmax, wmax], detections=int(counts.sum()),
                                  median_ms=round(med, 4), min_ms=round(lo, 4),
                                  max_ms=round(hi, 4),
                                  images_per_s=round(n / med * 1e3, 1))), flush=True)
        a, b, c = res['ragged'], res['per-image'], res['ceiling']
        print(json.dumps(dict(info, group='ragged', kind=kind, route='ratios',
                              ragged_over_per_image=round(a[0] / b[0], 4),
                              ragged_over_ceiling=round(a[0] / c[0], 4),
                              speedup_over_per_image=round(b[0] / a[0], 2),
                              gap_ms=round(b[0] - a[0], 4),
                              spread_ragged_ms=round(a[2] - a[1], 4),
                              spread_per_image_ms=round(b[2] - b[1], 4),
                              beats_per_image_by_more_than_either_spread=bool(
                                  b[0] - a[0] > max(a[2] - a[1], b[2] - b[1])))), flush=True)
        del fields, full, cd, per_shape, ceiling_cd
        torch.cuda.empty_cache()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_group_wall(cases, runs, warmup=3):
    """run_group on the wall clock; every case synchronises itself."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    times = {name: [] for name in cases}
    for _ in range(runs):
        for name, fn in cases.items():
            times[name].append(wall(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def load_parent_package(directory):
    """DIR/openpifpaf_amd as the package `openpifpaf_amd_parent` (its imports are relative,
    and its _lib loads the library beside it)."""
    path = os.path.join(os.path.abspath(directory), 'openpifpaf_amd')
    spec = importlib.util.spec_from_file_location(
        'openpifpaf_amd_parent', os.path.join(path, '__init__.py'),
        submodule_search_locations=[path])
    module = importlib.util.module_from_spec(spec)
    sys.modules['openpifpaf_amd_parent'] = module
    spec.loader.exec_module(module)
    return importlib.import_module('openpifpaf_amd_parent.decoder')


def fetch_routes(args, info):
    from openpifpaf_amd.engine import DetPipeline  # pylint: disable=import-outside-toplevel
    n = args.images
    cats = ['c%d' % i for i in range(K)]
    packages = {'new': decoder}
    if args.baseline_package:
        packages['parent'] = load_parent_package(args.baseline_package)
    for kind in ('planted', 'uniform'):
        for pkg in packages.values():
            pkg.CifHr.v_threshold = 0.1
            pkg.CifSeeds.threshold = SEED_THRESHOLD[kind]
        det = _device.to_device(synthetic.det_batch(kind, n, H, W, n_categories=K))
        cds = {name: pkg.CifDet(pkg.FieldConfig(), cats) for name, pkg in packages.items()}
        recs, offsets = cds['new'].decode_records(det)
        common = dict(info, kind=kind, images=n, detections=int(offsets[-1]),
                      record_bytes=int(offsets[-1]) * DET_DTYPE.itemsize)
        if 'parent' in cds:
            old, old_offsets = cds['parent'].decode_records(det)
            assert old_offsets.tolist() == offsets.tolist()
            assert old.tobytes() == recs.tobytes()
            for first in ('parent', 'new'):
                order = [first] + [name for name in cds if name != first]
                cases = {name: (lambda cd=cds[name]: cd.decode_records(det)) for name in order}
                res = run_group_wall(cases, args.runs)
                for case, (med, lo, hi) in res.items():
                    print(json.dumps(dict(common, group='fetch', case=case, first=first,
                                          median_ms=round(med, 4), min_ms=round(lo, 4),
                                          max_ms=round(hi, 4))), flush=True)
                print(json.dumps(dict(
                    common, group='fetch', case='verdict', first=first,
                    new_over_parent=round(res['new'][0] / res['parent'][0], 4),
                    new_median_at_or_below_parent_range=bool(
                        res['new'][0] <= res['parent'][1]))), flush=True)
        # the pipeline against the sequential engine, this build only
        cd, steps = cds['new'], args.batches
        pipe, piped = DetPipeline(), decoder.CifDet(decoder.FieldConfig(), cats)

        def sequential():
            for _ in range(steps):
                cd.decode_records(det)

        def pipeline():
            pending = [pipe.submit(piped, det) for _ in range(steps)]
            return [p.result() for p in pending]

        got = pipeline()
        assert all(r.tobytes() == recs.tobytes() and o.tolist() == offsets.tolist()
                   for r, o in got)
        del got
        res = run_group_wall({'sequential': sequential, 'pipeline': pipeline}, args.runs)
        for case, (med, lo, hi) in res.items():
            print(json.dumps(dict(common, group='pipeline', case=case, batches=steps,
                                  median_ms_per_batch=round(med / steps, 4),
                                  min_ms_per_batch=round(lo / steps, 4),
                                  max_ms_per_batch=round(hi / steps, 4),
                                  images_per_s=round(n * steps / med * 1e3, 1))), flush=True)
        seq, pip = res['sequential'], res['pipeline']
        print(json.dumps(dict(common, group='pipeline', case='verdict', batches=steps,
                              pipeline_over_sequential=round(pip[0] / seq[0], 4),
                              pipeline_median_below_sequential_range=bool(pip[0] < seq[1]))),
              flush=True)
        del det, cds, cd, pipe, piped
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--ragged', action='store_true')
    ap.add_argument('--fetch', action='store_true')
    ap.add_argument('--baseline-package', default=None,
                    help='--fetch: a built checkout of the commit to compare against')
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--new-first', action='store_true',
                    help='--baseline-lib: this build before the parent in every alternation')
    ap.add_argument('--runs', type=int, default=21)
    ap.add_argument('--images', type=int, default=256)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be at least 20')
    if not args.baseline_lib and not args.ragged and not args.fetch:
        ap.error('nothing to time: give --baseline-lib PATH, --ragged and / or --fetch')
    _device.require()
    info = {'device': torch.cuda.get_device_name(0), 'library': build.source_digest(),
            'runs': args.runs, 'warmup': 3, 'clock': 'events'}
    if args.baseline_lib:
        against_parent(args, dict(info, baseline_lib=os.path.basename(args.baseline_lib)))
    if args.ragged:
        ragged_routes(args, info)
    if args.fetch:
        fetch_routes(args, dict(info, clock='wall'))


if __name__ == '__main__':
    main()
