"""Times the batched connection_value / p2p_value entry points (csrc/edges.hip) against the
one-launch-per-query route they replace.  Not part of bench.py.

    python tools/edge_values_time.py              on a box with an MI355X
    python tools/edge_values_time.py --reference  on a box with the reference (CPU only)

Sets: CafScored at 0.1 of the planted 80x80 image (seed 0).  Queries: Q = 1024 and 16384,
query i reads set i % 2C from a source on one of that set's own columns (joint scale = the
column's source scale, at least 1) towards that column's target.  Reported per Q and entry:
the median of 5 event-timed launches over a device-resident query table, and the median of 5
wall-clock calls of the Python API (upload, launch, read-back).  The comparator is Q = 1024
calls of functional.grow_connection_blend, wall-clock: the only route to the forward half of
connection_value before these entries.  Exits 1 if the batched forward half (the API call
with reverse_match=False, wall-clock) is not at least 10 times faster than it.

--reference: the reference's own Python loop (CifCaf.connection_value and p2p_value per
query) for Q = 1024 on this box's CPU, over the host twin's sets of the same image.
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openpifpaf_amd import _edges, constants, synthetic  # noqa: E402  pylint: disable=wrong-import-position

SKELETON = list(constants.COCO_PERSON_SKELETON)
QS = (1024, 16384)


def make_queries(sets, n_q):
    """sets: host (9, N) arrays in (backward, forward) pairs -> pp_edge_query table."""
    used = [i for i, s in enumerate(sets) if s.shape[1]]
    src, tgt, idx = [], [], []
    for i in range(n_q):
        si = used[i % len(used)]
        s = sets[si]
        k = (i // len(used)) % s.shape[1]
        src.append((s[1, k], s[2, k], 0.8, max(1.0, s[4, k])))
        tgt.append((s[5, k], s[6, k], s[8, k]))
        idx.append(si)
    return _edges.queries(np.array(src, np.float32), idx, np.array(tgt, np.float32))


def src4(q):
    return np.stack([q['x'], q['y'], q['v'], q['s']], axis=1)


def tgt3(q):
    return np.stack([q['tx'], q['ty'], q['ts']], axis=1)


def median_wall(fn, n=5):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times) * 1e3


def on_device():
    import torch  # pylint: disable=import-outside-toplevel
    from openpifpaf_amd import _device, decoder, functional  # pylint: disable=import-outside-toplevel
    from openpifpaf_amd._lib import call  # pylint: disable=import-outside-toplevel
    cif, caf = synthetic.planted(80, 80, n_people=8, seed=0, skeleton=SKELETON)
    cif, caf = torch.from_numpy(cif).cuda(), torch.from_numpy(caf).cuda()
    fc = decoder.FieldConfig()
    hr = decoder.CifHr(fc).fill([cif, caf]).accumulated
    cs = decoder.CafScored(hr, fc, SKELETON).fill([cif, caf])
    packed = cs.packed
    host = _edges.pack_sets(packed)
    sets = [host.cols[i, :, :host.counts[i]] for i in range(host.n_sets)]
    res = {'device': torch.cuda.get_device_name(0), 'sets': host.n_sets,
           'columns': int(host.counts.sum()), 'cap': host.cap}

    def event_ms(name, qd, n_q, extra, out):
        def launch():
            call(name, _device.ptr(packed.cols), ctypes.c_int64(9 * packed.cap),
                 ctypes.c_int64(packed.cap), _device.ptr(packed.counts),
                 ctypes.c_int32(packed.n_sets), _device.ptr(qd), ctypes.c_int64(n_q),
                 ctypes.c_int32(0), *extra, _device.ptr(out), _device.stream())
        launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return statistics.median(times)

    for n_q in QS:
        q = make_queries(sets, n_q)
        qd = torch.from_numpy(q.view(np.uint8)).cuda()
        out4 = torch.empty((n_q, 4), dtype=torch.float32, device='cuda')
        out1 = torch.empty(n_q, dtype=torch.float32, device='cuda')
        for tag, rm in (('connection', 1), ('connection_forward_only', 0)):
            res['%s_q%d_event_ms' % (tag, n_q)] = event_ms(
                'pp_connection_values', qd, n_q, (ctypes.c_float(0.0), ctypes.c_int32(rm)), out4)
            res['%s_q%d_api_wall_ms' % (tag, n_q)] = median_wall(
                lambda rm=rm: functional.connection_values(packed, src4(q), q['set'],
                                                           reverse_match=bool(rm)))
        res['p2p_q%d_event_ms' % n_q] = event_ms('pp_p2p_values', qd, n_q, (), out1)
        res['p2p_q%d_api_wall_ms' % n_q] = median_wall(
            lambda: functional.p2p_values(packed, src4(q), tgt3(q), q['set']))
        if n_q == 1024:
            nonzero = functional.connection_values(packed, src4(q), q['set']).any(axis=1).sum()
            res['connection_q1024_nonzero'] = int(nonzero)

    # the comparator: one launch, one 16-byte read-back and one sync per query
    q = make_queries(sets, 1024)
    dsets = [cs.backward[i // 2] if i % 2 == 0 else cs.forward[i // 2]
             for i in range(host.n_sets)]
    dsets = [s.contiguous() for s in dsets]

    def loop():
        for e in q:
            functional.grow_connection_blend(dsets[e['set']], e['x'], e['y'], max(0.0, e['s']))
    loop()
    t0 = time.perf_counter()
    loop()
    res['grow_connection_blend_loop_q1024_wall_ms'] = (time.perf_counter() - t0) * 1e3
    res['ratio_forward_q1024_wall'] = (res['grow_connection_blend_loop_q1024_wall_ms'] /
                                       res['connection_forward_only_q1024_api_wall_ms'])
    res['ratio_forward_q1024_event'] = (res['grow_connection_blend_loop_q1024_wall_ms'] /
                                        res['connection_forward_only_q1024_event_ms'])
    print(json.dumps(res))
    return 0 if res['ratio_forward_q1024_wall'] >= 10.0 else 1


def on_reference():
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import ref_loader  # pylint: disable=import-outside-toplevel
    from openpifpaf_amd import stages_cpu  # pylint: disable=import-outside-toplevel
    from openpifpaf_amd._abi import make_config  # pylint: disable=import-outside-toplevel
    op = ref_loader.load()
    cif, caf = synthetic.planted(80, 80, n_people=8, seed=0, skeleton=SKELETON)
    cfg = make_config()
    hr = stages_cpu.cifhr(cif[None], cfg)
    fwd, bwd = stages_cpu.caf_scored(caf[None], hr, SKELETON, 0.1, cfg)[0]
    sets = [s for pair in zip(bwd, fwd) for s in pair]
    q = make_queries(sets, 1024)

    class Sets:
        def directed(self, caf_i, forward):
            return (fwd[caf_i], bwd[caf_i]) if forward else (bwd[caf_i], fwd[caf_i])

    class Joint:
        def __init__(self, e):
            self.data = np.array([[e['x'], e['y'], e['v']]], np.float32)
            self.joint_scales = np.array([e['s']], np.float32)

    op.decoder.CifCaf.keypoint_threshold = 0.0
    op.decoder.CifCaf.connection_method = 'blend'
    d = op.decoder.CifCaf(op.decoder.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                          skeleton=SKELETON)
    cs = Sets()
    res = {}
    with np.errstate(all='ignore'):
        for tag, rm in (('connection', True), ('connection_forward_only', False)):
            t0 = time.perf_counter()
            for e in q:
                d.by_source = {0: {0: (int(e['set']) // 2, bool(e['set'] % 2))}}
                d.connection_value(Joint(e), cs, 0, 0, reverse_match=rm)
            res['reference_%s_q1024_wall_ms' % tag] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for e in q:
            d.p2p_value((e['x'], e['y'], e['v']), cs, e['s'], (e['tx'], e['ty'], e['ts'], 1.0),
                        int(e['set']) // 2, bool(e['set'] % 2))
        res['reference_p2p_q1024_wall_ms'] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(res))
    return 0


if __name__ == '__main__':
    sys.exit(on_reference() if '--reference' in sys.argv else on_device())
