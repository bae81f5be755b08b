"""Writes tests/golden/edges.npz: CifCaf.connection_value and CifCaf.p2p_value
(cifcaf.py:194-245) of the reference over reference-decoded poses (data only).

  python tests/golden/gen_edges.py        (needs the reference; see oracle/ref_loader.py)

Per case (CASES, all COCO skeleton) the reference decodes the synthetic fields, builds its
CafScored at 0.1, and is asked for
  conn_rm1 / conn_rm0  connection_value with / without reverse_match for every annotation and
                       directed edge, (n_ann, 2C, 4): [a, 2 c] the forward edge of CAF c (start
                       j1, end j2), [a, 2 c + 1] the backward one (start j2, end j1); unset
                       start joints included
  p2p                  p2p_value for every ordered annotation pair (a pair of an annotation
                       with itself included) and directed edge, (n_ann, n_ann, C, 2):
                       [s, t, c, 0] source joint j1 against target joint j2, [s, t, c, 1]
                       source j2 against target j1
with the annotations' data and joint_scales and the inputs' SHA-256; the tests rebuild the
fields from openpifpaf_amd.synthetic.  Stored as <case>_<key>.

`edge_*`: the first n columns, n in EDGE_NS, of one real forward / backward set pair (stored),
queried with points on and off its columns.  `corner_*`: p2p_value's corners on that pair:
source scale zero and negative, target scale zero off every column (a divide warning), a NaN
result (the target on the FIRST kept column's target with target scale zero) and the same on a
later kept column (a finite result).  `blend_returns`: how often each of _target_with_blend's
four returns was taken by the stored connection_value queries.  The generator asserts the
conditions the tests re-assert from the stored arrays (check_conditions).
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden  # noqa: E402  pylint: disable=wrong-import-position
from gen_golden import configure, make_inputs, ref_loader, sha  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd import constants  # noqa: E402  pylint: disable=wrong-import-position

# (name, generator, H, W, seed, mode, extra)
CASES = [
    ('p40_s0_predict', 'planted', 40, 40, 0, 'predict', {}),
    ('p40_s3_max', 'planted', 40, 40, 3, 'eval', {'connection_method': 'max'}),
    ('u10_s0_eval', 'uniform', 10, 10, 0, 'eval', {}),
    ('p31x41_kth', 'planted', 31, 41, 0, 'eval', {'n_people': 3, 'keypoint_threshold': 0.3}),
    # every connection score of the planted image above is over 0.70 in the reference, so its
    # threshold of 0.3 zeroes nothing; the uniform image's weak scores are what it cuts
    ('u10_kth', 'uniform', 10, 10, 0, 'eval', {'keypoint_threshold': 0.3}),
]
EDGE_NS = (0, 1, 2, 63, 64, 65)


class Counter:
    """Counts which of _target_with_blend's four returns (cifcaf.py:165-192) each call takes,
    from the call's arguments and result (the wrapped method runs unchanged)."""

    def __init__(self, cls):
        self.counts = np.zeros(4, np.int64)
        self.active = False  # only the calls behind a stored result are counted
        self.cls = cls
        self.inner = cls._target_with_blend

    def __call__(self, target_coordinates, scores):
        res = self.inner(target_coordinates, scores)
        if not self.active:
            return res
        if len(scores) == 1:
            self.counts[0] += 1
        else:
            top = np.argsort(scores)
            e1, e2 = target_coordinates[:, top[-1]], target_coordinates[:, top[-2]]
            s1, s2 = scores[top[-1]], scores[top[-2]]
            if s2 < 0.01 or s2 < 0.5 * s1:
                self.counts[1] += 1
            elif np.linalg.norm(e1[:2] - e2[:2]) > e1[3] / 2.0:
                self.counts[2] += 1
            else:
                self.counts[3] += 1
        return res

    def __enter__(self):
        self.cls._target_with_blend = staticmethod(self)
        return self

    def __exit__(self, *exc):
        self.cls._target_with_blend = staticmethod(self.inner)


def f4(t):
    return np.array([float(v) for v in t], np.float32)


def run_case(decoder, gen, h, w, seed, mode, extra):
    """The reference's decode and CafScored of one image."""
    skel = list(constants.COCO_PERSON_SKELETON)
    configure(decoder, mode, extra)
    decoder.CifCaf.keypoint_threshold = extra.get('keypoint_threshold',
                                                  decoder.CifCaf.keypoint_threshold)
    cif, caf = make_inputs(gen, h, w, seed, skel, extra)
    fc = decoder.FieldConfig()
    dec = decoder.CifCaf(fc, keypoints=constants.COCO_KEYPOINTS, skeleton=skel)
    anns = dec([cif, caf])
    hr = decoder.CifHr(fc).fill([cif, caf]).accumulated
    cs = decoder.CafScored(hr, fc, skel).fill([cif, caf])
    return dec, anns, cs, (cif, caf), skel


def edge_tables(dec, anns, cs):
    """conn_rm1, conn_rm0, p2p of one case."""
    skel = dec.skeleton_m1
    n, c = len(anns), len(skel)
    conn = {rm: np.zeros((n, 2 * c, 4), np.float32) for rm in (True, False)}
    p2p = np.zeros((n, n, c, 2), np.float32)
    for a, ann in enumerate(anns):
        for ci, (j1, j2) in enumerate(skel):
            for d, (start, end) in enumerate(((j1, j2), (j2, j1))):
                for rm in (True, False):
                    conn[rm][a, 2 * ci + d] = f4(dec.connection_value(ann, cs, start, end,
                                                                      reverse_match=rm))
                for t, tgt in enumerate(anns):
                    target = (tgt.data[end, 0], tgt.data[end, 1], tgt.joint_scales[end],
                              tgt.data[end, 2])
                    p2p[a, t, ci, d] = dec.p2p_value(ann.data[start], cs, ann.joint_scales[start],
                                                     target, ci, d == 0)
    return conn[True], conn[False], p2p


class TwoSets:
    """directed() over one forward / backward pair cut to n columns."""

    def __init__(self, fwd, bwd, n):
        self.fwd, self.bwd = np.ascontiguousarray(fwd[:, :n]), np.ascontiguousarray(bwd[:, :n])

    def directed(self, caf_i, forward):
        return (self.fwd, self.bwd) if forward else (self.bwd, self.fwd)


class Joint:
    """The two members of an annotation that connection_value reads."""

    def __init__(self, x, y, v, s):
        self.data = np.array([[x, y, v]], np.float32)
        self.joint_scales = np.array([s], np.float32)


def gen_edge_sets(out, dec, cs):
    """Sets of 0 .. 65 columns, and p2p_value's corners."""
    from openpifpaf.functional import caf_center_s  # pylint: disable=import-outside-toplevel
    ci = next(i for i in range(len(cs.forward))
              if cs.forward[i].shape[1] >= 65 and cs.backward[i].shape[1] >= 65)
    fwd = np.ascontiguousarray(cs.forward[ci][:, :65])
    bwd = np.ascontiguousarray(cs.backward[ci][:, :65])
    out['edge_fwd'], out['edge_bwd'], out['edge_ns'] = fwd, bwd, np.array(EDGE_NS, np.int32)
    # sources on columns 0, 1, 62, 63, 64 (their own scale row as the joint scale), the same
    # moved off the columns, and one far from every column; targets near each column's target
    cols = (0, 1, 62, 63, 64)
    src, tgt = [], []
    for k in cols:
        for dx, dy in ((0.0, 0.0), (0.375, -0.25)):
            src.append((fwd[1, k] + dx, fwd[2, k] + dy, 0.75, max(1.0, fwd[4, k])))
            tgt.append((fwd[5, k] + 0.5 * dx, fwd[6, k] - dy, max(1.0, fwd[8, k])))
    src.append((-500.0, -500.0, 0.75, 2.0))
    tgt.append((10.0, 10.0, 2.0))
    src, tgt = np.array(src, np.float32), np.array(tgt, np.float32)
    out['edge_sources'], out['edge_targets'] = src, tgt
    dec.by_source = {0: {0: (0, True)}}  # start 0 -> end 0 along "CAF 0", forward
    for n in EDGE_NS:
        two = TwoSets(fwd, bwd, n)
        for rm in (True, False):
            out['edge_conn_rm%d_n%d' % (rm, n)] = np.stack(
                [f4(dec.connection_value(Joint(*s), two, 0, 0, reverse_match=rm)) for s in src])
        out['edge_p2p_n%d' % n] = np.array(
            [dec.p2p_value(s[:3], two, s[3], (t[0], t[1], t[2], 1.0), 0, True)
             for s, t in zip(src, tgt)], np.float32)
        if n == 0:
            assert not out['edge_conn_rm1_n0'].any() and not out['edge_p2p_n0'].any()

    # corners: a source whose box keeps at least two columns
    two = TwoSets(fwd, bwd, 65)
    # (a planted person's columns share one target: the later column is the first kept one
    # with another target, which takes a box wide enough to reach a second person)
    k0, kept, later = None, None, None
    for ss in (np.float32(8.0), np.float32(16.0), np.float32(32.0), np.float32(64.0)):
        for k in range(65):
            kept = caf_center_s(fwd, fwd[1, k], fwd[2, k], sigma=2.0 * ss)
            differs = np.flatnonzero((kept[5:7] != kept[5:7, :1]).any(axis=0))
            if len(differs):
                k0, later = k, int(differs[0])
                break
        if k0 is not None:
            break
    assert k0 is not None, 'no source keeps two columns with different targets'
    sx, sy = fwd[1, k0], fwd[2, k0]
    off = (np.float32(kept[5, 0] + 0.3125), np.float32(kept[6, 0] + 0.4375))
    corners = [  # (name, source (x, y, v, s), target (x, y, s))
        ('source_scale_zero', (sx + 0.3125, sy, 0.75, 0.0), (off[0], off[1], 2.0)),
        ('source_scale_negative', (sx + 0.3125, sy, 0.75, -1.5), (off[0], off[1], 2.0)),
        ('target_scale_zero_off', (sx, sy, 0.75, ss), (off[0], off[1], 0.0)),
        ('nan_first_kept', (sx, sy, 0.75, ss), (kept[5, 0], kept[6, 0], 0.0)),
        ('nan_later_kept', (sx, sy, 0.75, ss), (kept[5, later], kept[6, later], 0.0)),
    ]
    res, warned = [], []
    for _, s, t in corners:
        s, t = np.array(s, np.float32), np.array(t, np.float32)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            res.append(dec.p2p_value(s[:3], two, s[3], (t[0], t[1], t[2], np.float32(1.0)), 0,
                                     True))
        warned.append(any('divide by zero' in str(c.message) for c in caught))
    res = np.array(res, np.float32)
    names = [c[0] for c in corners]
    assert res[0] == 0.0 and res[1] == 0.0, res
    assert res[2] == 0.0 and warned[2], (res, warned)
    assert np.isnan(res[3]), res
    assert np.isfinite(res[4]), res
    out['corner_names'] = np.array(names)
    out['corner_sources'] = np.array([c[1] for c in corners], np.float32)
    out['corner_targets'] = np.array([c[2] for c in corners], np.float32)
    out['corner_p2p'] = res
    out['corner_divide_warning'] = np.array(warned)
    print('edge sets from CAF', ci, 'corners', dict(zip(names, res.tolist())))


def start_set(out, name):
    """[a, e]: the start joint of directed edge e of annotation a is set (v > 0)."""
    skel = np.asarray(constants.COCO_PERSON_SKELETON).reshape(-1, 2) - 1
    return out[name + '_ann_data'][:, skel.reshape(-1), 2] > 0


def check_conditions(out):
    """What the tests rely on, from the stored arrays alone (tests/test_edges_cpu.py
    re-asserts the same).  The connection counts are over the edges whose start joint is set:
    an unset start joint (0, 0, v = 0, scale 0) has an empty box."""
    st = start_set(out, 'p40_s0_predict')
    nz = out['p40_s0_predict_conn_rm1'].any(axis=2)
    assert nz[st].sum() >= 0.9 * st.sum(), (nz[st].sum(), st.sum())
    assert (out['p40_s0_predict_p2p'] > 1e-3).sum() >= 100
    rm1 = out['u10_s0_eval_conn_rm1'].any(axis=2)
    rm0 = out['u10_s0_eval_conn_rm0'].any(axis=2)
    assert (rm0 & ~rm1).sum() >= 10 and rm1.sum() >= 10, ((rm0 & ~rm1).sum(), rm1.sum())
    assert (out['blend_returns'] > 0).all(), out['blend_returns']
    assert out['p31x41_kth_zeroed_by_threshold'] + out['u10_kth_zeroed_by_threshold'] >= 1
    assert not out['edge_conn_rm1_n0'].any() and not out['edge_conn_rm0_n0'].any()
    assert not out['edge_p2p_n0'].any()
    c = out['corner_p2p']
    assert c[0] == 0 and c[1] == 0 and c[2] == 0 and np.isnan(c[3]) and np.isfinite(c[4])
    return dict(p40_conn_nonzero=(int(nz[st].sum()), int(st.sum())),
                p40_p2p_above=int((out['p40_s0_predict_p2p'] > 1e-3).sum()),
                u10_reverse_zeroed=int((rm0 & ~rm1).sum()), u10_nonzero=int(rm1.sum()),
                zeroed_by_threshold=(int(out['p31x41_kth_zeroed_by_threshold']),
                                     int(out['u10_kth_zeroed_by_threshold'])))


def main():
    op = ref_loader.load()
    decoder = op.decoder
    out = {}
    with Counter(decoder.CifCaf) as counter, np.errstate(all='ignore'), \
            warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, gen, h, w, seed, mode, extra in CASES:
            dec, anns, cs, fields, skel = run_case(decoder, gen, h, w, seed, mode, extra)
            counter.active = True
            rm1, rm0, p2p = edge_tables(dec, anns, cs)
            counter.active = False
            out.update({
                name + '_generator': np.array(gen), name + '_H': h, name + '_W': w,
                name + '_seed': seed, name + '_mode': np.array(mode),
                name + '_skeleton': np.asarray(skel, np.int32),
                name + '_n_people': extra.get('n_people', 8),
                name + '_connection_method': np.array(extra.get('connection_method', 'blend')),
                name + '_keypoint_threshold': np.float64(dec.keypoint_threshold),
                name + '_input_sha': np.array(sha(*fields)),
                name + '_ann_data': np.stack([a.data for a in anns]).astype(np.float32),
                name + '_ann_joint_scales': np.stack([a.joint_scales
                                                      for a in anns]).astype(np.float32),
                name + '_conn_rm1': rm1, name + '_conn_rm0': rm0, name + '_p2p': p2p,
            })
            if 'keypoint_threshold' in extra:  # the same queries with no threshold
                dec.keypoint_threshold = 0.0
                free = edge_tables(dec, anns, cs)[0]
                out[name + '_zeroed_by_threshold'] = int((free.any(axis=2) &
                                                          ~rm1.any(axis=2)).sum())
            if name == 'p40_s0_predict':
                edge_dec, edge_cs = dec, cs
            print('%-16s anns %2d  conn nonzero %4d / %4d  p2p > 1e-3 %5d / %5d' % (
                name, len(anns), rm1.any(axis=2).sum(), rm1.shape[0] * rm1.shape[1],
                (p2p > 1e-3).sum(), p2p.size))
        # a return that no stored query takes: add a case (another seed) to CASES until it is
        assert (counter.counts > 0).all(), counter.counts
        out['blend_returns'] = counter.counts.copy()
    edge_dec.keypoint_threshold, edge_dec.connection_method = 0.001, 'blend'
    out['edge_keypoint_threshold'] = np.float64(edge_dec.keypoint_threshold)
    gen_edge_sets(out, edge_dec, edge_cs)
    decoder.CifSeeds.threshold = None
    decoder.CifCaf.keypoint_threshold = 0.0
    decoder.CifCaf.connection_method = 'blend'
    print('conditions', check_conditions(out), 'blend returns', out['blend_returns'].tolist())
    path = os.path.join(HERE, 'edges.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    assert gen_golden.HERE == HERE
    main()
