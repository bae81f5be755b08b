"""Keypoint counts and skeletons other than COCO's, on the host (tests/kc_util.py cases).

The reference's own outputs (tests/golden/kc_*.npz, made by gen_golden.py's `kc` section)
pin the oracle and the host twin of the decode outside K = 17: stages and annotations are
compared exactly (golden_util's tolerances are zero), the twin against the oracle byte for
byte on batches, the host NMS against the oracle's over a range of K, and the entry points
refuse shapes outside the envelope K <= PP_MAX_KP (24), C <= PP_MAX_EDGES (64).  The
counts at the end keep the GPU tests of tests/test_gpu_kc.py from passing vacuously: the
oracle alone must meet them.  CPU only."""
import numpy as np
import pytest

import golden_util as gu
import kc_util as kc
import oracle
from openpifpaf_amd import stages_cpu, synthetic
from openpifpaf_amd._abi import ANN_DTYPE, PP_MAX_EDGES, PP_MAX_FRONTIER, PP_MAX_KP, make_config
from openpifpaf_amd._lib import PPError

KEYS = ('data', 'joint_scales', 'score', 'n_keypoints', 'n_decoding', 'decoding_pairs',
        'decoding_xyv', 'n_frontier', 'frontier_pairs')
FIXTURES = kc.fixture_list()
FIDS = [kc.fixture_id(fx) for fx in FIXTURES]


def _same(got, want):
    assert len(got) == len(want)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key


# ---- the cases and their generators ------------------------------------------------------

def test_cases_are_well_formed():
    expect = {'pair2': (2, 1), 'loop3': (3, 3), 'iso4': (4, 2), 'chain5': (5, 4),
              'split6': (6, 4), 'k8c7': (8, 7), 'k20c33': (20, 33), 'k24star': (24, 23),
              'k24c64': (PP_MAX_KP, PP_MAX_EDGES)}
    assert set(expect) == set(kc.NAMES)
    for name in kc.NAMES:
        k, skeleton = kc.case(name)
        kc.check_skeleton(k, skeleton)
        assert (k, len(skeleton)) == expect[name]
        assert (len(kc.components(k, skeleton)) == 1) == (name in kc.CONNECTED), name
    assert kc.components(*kc.case('iso4')) == [[0, 1, 2], [3]]
    assert kc.components(*kc.case('split6')) == [[0, 1, 2], [3, 4, 5]]
    for name in ('k20c33', 'k24c64'):  # mixed directions: about half the edges reversed
        _, skeleton = kc.case(name)
        rev = sum(j1 > j2 for j1, j2 in skeleton)
        assert 0.4 * len(skeleton) <= rev <= 0.6 * len(skeleton), (name, rev)
    assert 2 * len(kc.case('k20c33')[1]) == 66            # the second slot per lane
    assert 4 * len(kc.case('k24c64')[1]) == PP_MAX_FRONTIER
    assert sorted(kc.committed_fixtures()) == sorted(
        FIDS + [kc.fixture_id(kc.MULTI_FIXTURE)])


def test_check_skeleton_refuses():
    for bad in ([(1, 1)], [(1, 2), (2, 1)], [(1, 2), (1, 2)], [(0, 1)], [(1, 4)]):
        with pytest.raises(AssertionError):
            kc.check_skeleton(3, bad)


def test_generators():
    """uniform_kc(17, 19, ...) is synthetic.uniform; every generator is deterministic."""
    for h, w, seed in ((20, 23, 0), (12, 15, 5)):
        assert gu.sha(*kc.uniform_kc(17, 19, h, w, seed)) == \
            gu.sha(*synthetic.uniform(h, w, n_caf=19, seed=seed))
    k, skeleton = kc.case('k20c33')
    cif, caf = kc.planted_kc(k, skeleton, 33, 40, seed=1)
    assert cif.shape == (20, 5, 33, 40) and caf.shape == (33, 9, 33, 40)
    assert gu.sha(cif, caf) == gu.sha(*kc.planted_kc(k, skeleton, 33, 40, seed=1))
    assert gu.sha(cif, caf) != gu.sha(*kc.planted_kc(k, skeleton, 33, 40, seed=2))
    assert (cif[:, 0] >= 0.7).any(axis=(1, 2)).all()  # every joint planted
    assert (caf[:, 0] >= 0.7).any(axis=(1, 2)).all()  # and every limb
    heads = kc.planted_kc_multi(k, skeleton, 321, 321, [8, 16], seed=1)
    assert [h[0].shape for h in heads] == [(20, 5, 41, 41), (20, 5, 21, 21)]
    again = kc.planted_kc_multi(k, skeleton, 321, 321, [8, 16], seed=1)
    assert gu.sha(*[f for h in heads for f in h]) == gu.sha(*[f for h in again for f in h])
    um = kc.uniform_kc_multi(5, 4, 161, 161, [8, 16], seed=2)
    assert [h[1].shape for h in um] == [(4, 9, 21, 21), (4, 9, 11, 11)]
    assert gu.sha(*um[1]) == gu.sha(*kc.uniform_kc(5, 4, 11, 11, 2001))


# ---- oracle and host twin against the reference's fixtures -------------------------------

@pytest.mark.parametrize('fx', FIXTURES, ids=FIDS)
def test_oracle_stages(fx):
    g = kc.load_fixture(fx)
    cif, caf, skeleton = gu.case_inputs(g)
    assert cif.shape[0] == int(g['K']) == kc.case(fx[0])[0] and skeleton == kc.case(fx[0])[1]
    cfg = gu.case_config(g)
    hr = oracle.cifhr(cif, cfg)
    assert gu.sha(hr) == str(g['cifhr_sha'])
    assert np.array_equal(gu.seeds_as_rows(oracle.seeds(cif, hr, cfg)), g['seeds'])
    for tag, th in (('a', 0.1), ('b', 0.0001)):
        fwd, bwd = oracle.caf_scored(caf, hr, skeleton, th, cfg)
        assert [f.shape[1] for f in fwd] == list(g['caf_%s_fwd_counts' % tag])
        assert [b.shape[1] for b in bwd] == list(g['caf_%s_bwd_counts' % tag])
        assert [gu.sha(f) for f in fwd] == [str(s) for s in g['caf_%s_fwd_sha' % tag]]
        assert [gu.sha(b) for b in bwd] == [str(s) for s in g['caf_%s_bwd_sha' % tag]]


@pytest.mark.parametrize('fx', FIXTURES, ids=FIDS)
def test_oracle_decode(fx):
    g = kc.load_fixture(fx)
    cif, caf, skeleton = gu.case_inputs(g)
    recs = oracle.decode(cif, caf, skeleton, gu.case_config(g))
    assert (recs['n_keypoints'] == int(g['K'])).all()
    errs = gu.compare_annotations(g, recs)
    assert not errs, errs[:10]


@pytest.mark.parametrize('fx', FIXTURES, ids=FIDS)
def test_twin_stages_and_decode(fx):
    g = kc.load_fixture(fx)
    cif, caf, skeleton = gu.case_inputs(g)
    cfg = gu.case_config(g)
    hh, ww = oracle.hr_shape(cif.shape[2], cif.shape[3], cfg.stride)
    hr = stages_cpu.cifhr(cif[None], cfg)
    assert gu.sha(hr[0, :, :hh, :ww]) == str(g['cifhr_sha'])
    assert np.array_equal(gu.seeds_as_rows(stages_cpu.seeds(cif[None], hr, cfg)[0]), g['seeds'])
    fwd, bwd = stages_cpu.caf_scored(caf[None], hr, skeleton, cfg.caf_threshold, cfg)[0]
    assert [gu.sha(f) for f in fwd] == [str(s) for s in g['caf_a_fwd_sha']]
    assert [gu.sha(b) for b in bwd] == [str(s) for s in g['caf_a_bwd_sha']]
    recs, offsets = stages_cpu.decode_batch(cif[None], caf[None], skeleton, cfg, n_threads=1)
    assert recs.dtype == ANN_DTYPE and offsets.tolist() == [0, len(recs)]
    errs = gu.compare_annotations(g, recs)
    assert not errs, errs[:10]


def test_oracle_multi_vs_reference():
    """The ms2 FieldConfig with K = 24, C = 64: CifHr, seeds (heads x K segments), both
    CafScored sets and the annotations of the reference."""
    g = kc.load_fixture(kc.MULTI_FIXTURE)
    name, multi, _ = kc.MULTI_FIXTURE
    _, skeleton = kc.case(name)
    fields, kw = kc.multi_case(name, multi)
    assert gu.sha(*fields) == str(g['input_sha'])
    mem, cfg = oracle.Members(fields, **kw), gu.case_config(g)
    hr = oracle.cifhr_multi(mem, cfg)
    assert list(hr.shape) == list(g['cifhr_shape'])
    assert gu.sha(hr) == str(g['cifhr_sha'])
    assert np.array_equal(gu.seeds_as_rows(oracle.seeds_multi(mem, hr, cfg)), g['seeds'])
    for tag, th in (('a', 0.1), ('b', 0.0001)):
        fwd, bwd = oracle.caf_scored_multi(mem, hr, skeleton, th, cfg)
        assert [f.shape[1] for f in fwd] == list(g['caf_%s_fwd_counts' % tag])
        assert [gu.sha(f) for f in fwd] == [str(s) for s in g['caf_%s_fwd_sha' % tag]]
        assert [gu.sha(b) for b in bwd] == [str(s) for s in g['caf_%s_bwd_sha' % tag]]
    recs = oracle.decode_multi(mem, skeleton, cfg)
    assert len(recs) >= 3
    errs = gu.compare_annotations(g, recs)
    assert not errs, errs[:10]


# ---- host twin against the oracle ----------------------------------------------------------

@pytest.mark.parametrize('name', kc.NAMES)
def test_twin_vs_oracle_batch(name):
    """3-image uniform 20x23 batches in eval defaults, on 1 thread and on 2: the same bytes,
    and every image the oracle's records."""
    k, skeleton = kc.case(name)
    cfg = kc.config('eval')
    cif, caf = kc.uniform_kc_batch(k, len(skeleton), 3, 20, 23, first_seed=20)
    one, off1 = stages_cpu.decode_batch(cif, caf, skeleton, cfg, n_threads=1)
    two, off2 = stages_cpu.decode_batch(cif, caf, skeleton, cfg, n_threads=2)
    assert np.array_equal(off1, off2) and one.tobytes() == two.tobytes()
    assert off1[-1] > 0
    for i in range(3):
        ref = oracle.decode(cif[i], caf[i], skeleton, cfg)
        got = one[off1[i]:off1[i + 1]]
        _same(got, ref)
        assert (got['image'] == i).all()
        got = got.copy()
        got['image'] = 0  # the oracle decodes one image
        assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize('name', sorted(kc.REPEATED))
def test_twin_vs_oracle_repeated_pairs(name):
    """Skeletons with an unordered pair twice (kc.REPEATED): a later duplicate by_source key
    overwrites the CAF index and direction in place.  The only test that reaches that branch
    of csrc/by_source.hpp; uniform fields in eval defaults (predict defaults decode nothing
    on them)."""
    k, skeleton = kc.REPEATED[name]
    with pytest.raises(AssertionError):
        kc.check_skeleton(k, skeleton)
    cfg = kc.config('eval')
    counts = []
    longest = 0
    for h, w, seed in ((20, 23, 0), (12, 15, 5)):
        cif, caf = kc.uniform_kc(k, len(skeleton), h, w, seed)
        ref = oracle.decode(cif, caf, skeleton, cfg)
        got, _ = stages_cpu.decode_batch(cif[None], caf[None], skeleton, cfg, n_threads=1)
        _same(got, ref)
        counts.append(len(ref))
        longest = max(longest, int(ref['n_frontier'].max()))
    # what the oracle alone decodes there, so that the comparison is not vacuous
    assert counts == {'rep3': [5, 3], 'rep4': [9, 2]}[name]
    if name == 'rep4':
        assert longest == 5


def variant_configs(name):
    """The option sets of the `variants` tests: name -> pp_config keyword arguments."""
    k, skeleton = kc.case(name)
    c = len(skeleton)
    return {
        'max': dict(connection_method='max'),
        'greedy': dict(greedy=True),
        'confscales': dict(confidence_scales=[0.5 + 0.37 * (i % 5) for i in range(c)]),
        'seedmask': dict(seed_mask=[f not in (0, k - 1) for f in range(k)]),
    }


@pytest.mark.parametrize('name', kc.VARIANT_CASES)
@pytest.mark.parametrize('gen,mode', [('uniform', 'eval'), ('planted', 'eval'),
                                      ('planted', 'predict')])
def test_twin_vs_oracle_variants(name, gen, mode):
    h, w = (20, 23) if gen == 'uniform' else kc.PLANTED_SIZE
    cif, caf, skeleton = kc.inputs(name, gen, h, w)
    base = oracle.decode(cif, caf, skeleton, kc.config(mode))
    differs = 0
    for tag, kw in variant_configs(name).items():
        cfg = kc.config(mode, **kw)
        ref = oracle.decode(cif, caf, skeleton, cfg)
        got, _ = stages_cpu.decode_batch(cif[None], caf[None], skeleton, cfg)
        _same(got, ref)
        differs += len(ref) != len(base) or any(
            not np.array_equal(ref[key], base[key]) for key in KEYS)
    assert differs >= 2  # the options change the decode of these inputs


# ---- standalone keypoint NMS ---------------------------------------------------------------

NMS_K = (1, 2, 3, 7, 8, 9, 16, 24)


def nms_poses(k, n=200, seed=0):
    """n random poses of k joints: overlapping ones, a quarter of which repeat another
    pose's confidences at their own positions, and 10 pairs of far-away poses that share
    their confidences, which survive unedited with tied scores."""
    rng = np.random.default_rng(500 + k + seed)
    base = rng.uniform(10.0, 120.0, (n, 1, 2)).astype(np.float32)
    base[-20:, 0, 0] = 1000.0 + 200.0 * np.arange(20)
    xy = (base + rng.normal(0.0, 10.0, (n, k, 2))).astype(np.float32)
    v = rng.uniform(0.0, 1.0, (n, k)).astype(np.float32)
    v[rng.uniform(0.0, 1.0, (n, k)) < 0.2] = 0.0
    v[n // 4:n // 2] = v[:n // 4]
    xy[3 * n // 4:-20] = xy[n // 2:3 * n // 4 - 20]  # and some coincide exactly
    v[-10:] = v[-20:-10] = np.maximum(v[-20:-10], np.float32(0.3))
    data = np.concatenate([xy, v[:, :, None]], axis=2).astype(np.float32)
    scales = rng.uniform(0.5, 24.0, (n, k)).astype(np.float32)
    return data, scales


NMS_CFGS = [(0.0, 0.0, 0.0), (0.001, 0.1, 0.0), (0.0, 0.0, 0.5)]


@pytest.mark.parametrize('k', NMS_K)
def test_nms_keypoints_cpu_vs_oracle(k):
    for kt, it, sup in NMS_CFGS:
        data, scales = nms_poses(k)
        order, recs = oracle.nms_keypoints(data, scales, kt, it, sup)
        assert 0 < len(order) <= len(data)
        cfg = make_config(nms_keypoint_threshold=kt, nms_instance_threshold=it,
                          nms_suppression=sup)
        got = data.copy()
        got_order, scores = stages_cpu.nms_keypoints(got, scales, cfg)
        assert got_order == order.tolist()
        assert np.array_equal(got[order], recs['data'][:, :k])
        want = np.array([oracle.ann_score(d[:, 2]) for d in recs['data'][:, :k]])
        assert np.array_equal(scores, want)
        assert (np.diff(scores) == 0).sum() >= 10  # tied scores among the survivors


# ---- the envelope --------------------------------------------------------------------------

def _zeros(k, c, h=6, w=7):
    return np.zeros((1, k, 5, h, w), np.float32), np.zeros((1, c, 9, h, w), np.float32)


def test_envelope():
    cfg = make_config()
    star = [(1, j) for j in range(2, 26)]
    cif, caf = _zeros(25, 24)
    with pytest.raises(PPError, match='PP_ESHAPE.*outside the supported envelope'):
        stages_cpu.decode_batch(cif, caf, star, cfg)
    with pytest.raises(ValueError, match='rejected the shapes'):
        oracle.decode(cif[0], caf[0], star, cfg)
    pairs = [(a, b) for a in range(1, 25) for b in range(a + 1, 25)][:65]
    cif, caf = _zeros(24, 65)
    with pytest.raises(PPError, match='PP_ESHAPE.*outside the supported envelope'):
        stages_cpu.decode_batch(cif, caf, pairs, cfg)
    with pytest.raises(ValueError, match='rejected the shapes'):
        oracle.decode(cif[0], caf[0], pairs, cfg)
    k, skeleton = kc.case('chain5')
    cif, caf = _zeros(k, len(skeleton) + 1)
    with pytest.raises(ValueError, match='4 pairs for 5 CAF fields'):
        stages_cpu.decode_batch(cif, caf, skeleton, cfg)
    cif, caf = _zeros(k, len(skeleton))
    with pytest.raises(PPError, match='PP_EINVAL.*skeleton joint index out of 1..K'):
        stages_cpu.decode_batch(cif, caf, skeleton[:-1] + [(4, 6)], cfg)
    # both maxima are inside
    k, skeleton = kc.case('k24c64')
    cif, caf = _zeros(k, len(skeleton))
    recs, offsets = stages_cpu.decode_batch(cif, caf, skeleton, cfg)
    assert len(recs) == 0 and offsets.tolist() == [0, 0]
    assert len(oracle.decode(cif[0], caf[0], skeleton, cfg)) == 0


# ---- what the oracle alone reaches (the GPU tests assert the same of the device) ---------

def _decoded(name, gen, h, w, mode):
    cif, caf, skeleton = kc.inputs(name, gen, h, w)
    return oracle.decode(cif, caf, skeleton, kc.config(mode))


@pytest.mark.parametrize('name', kc.NAMES)
def test_oracle_counts(name):
    k, skeleton = kc.case(name)
    recs = _decoded(name, 'uniform', 20, 23, 'eval')
    assert len(recs) >= 5
    if name in kc.CONNECTED:  # some annotation grew over a spanning tree
        assert (recs['n_decoding'] == k - 1).any()
    else:
        assert not (recs['n_decoding'] == k - 1).any()
    for mode in ('eval', 'predict'):
        assert len(_decoded(name, 'planted', *kc.PLANTED_SIZE, mode)) >= 3, mode


def test_oracle_counts_maxima():
    recs = _decoded('k24c64', 'uniform', 31, 34, 'eval')
    assert len(recs) >= 50
    for h, w in kc.UNIFORM_SIZES:
        assert _decoded('k24c64', 'uniform', h, w, 'eval')['n_frontier'].max() >= 80, (h, w)
    assert _decoded('k20c33', 'uniform', 20, 23, 'eval')['n_frontier'].max() > 33


def test_oracle_counts_unconnected():
    """iso4: joint 4 has no edge, so force-complete cannot fill it, nor grow from it;
    split6: the flood fill does not cross from one component into the other."""
    for gen, h, w in (('uniform', 20, 23), ('planted',) + kc.PLANTED_SIZE):
        set_ = _decoded('iso4', gen, h, w, 'eval')['data'][:, :4, 2] > 0
        assert (~set_[:, 3] & set_[:, :3].all(axis=1)).any()
        assert (set_[:, 3] & ~set_[:, :3].any(axis=1)).any()
        assert not (set_[:, 3] & set_[:, :3].any(axis=1)).any()
        set_ = _decoded('split6', gen, h, w, 'eval')['data'][:, :6, 2] > 0
        a, b = set_[:, :3].any(axis=1), set_[:, 3:].any(axis=1)
        assert (a & ~b).any() and (b & ~a).any() and not (a & b).any()
