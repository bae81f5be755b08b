"""The device decode at keypoint counts and skeletons other than COCO's, on an MI355X.

The kernels carry the number of keypoints K (<= PP_MAX_KP = 24) and of skeleton edges C
(<= PP_MAX_EDGES = 64) as run-time values; tests/kc_util.py lists the cases (K from 2 to 24,
C from 1 to 64: cycles, an isolated joint, two components, a star, 2C > 64, both maxima) and
DESIGN.md ("envelope") what each reaches.  Everything is compared exactly: against the
reference's own outputs (tests/golden/kc_*.npz) and against the oracle, which
tests/test_kc_cpu.py pins to the same fixtures on the host.

From the narrowest layer to the widest, so that `-x` stops at the first one that breaks:
stages, single-image decodes, batches (both seed-loop kernels), option variants, shape
switching on one engine, compact records, multi-scale, standalone NMS and inverse.
"""
import ctypes

import numpy as np
import pytest

import golden_util as gu
import kc_util as kc
import oracle
from test_kc_cpu import NMS_CFGS, NMS_K, nms_poses, variant_configs

pytestmark = pytest.mark.gpu

KEYS = ('data', 'joint_scales', 'score', 'n_keypoints', 'n_decoding', 'decoding_pairs',
        'decoding_xyv', 'n_frontier', 'frontier_pairs')
FIXTURES = kc.fixture_list()
FIDS = [kc.fixture_id(fx) for fx in FIXTURES]


@pytest.fixture(scope='module')
def dec():
    from openpifpaf_amd import decoder
    return decoder


def _same(got, want, where=None):
    assert len(got) == len(want), (where, len(got), len(want))
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (where, key)


def _mode(mode, connection_method='blend', greedy=0):
    return {'mode': mode, 'connection_method': connection_method, 'greedy': greedy}


def _cifcaf(dec, name, g, **kw):
    """CifCaf of a case, the decoder classes configured as fixture (or _mode dict) g says."""
    k, skeleton = kc.case(name)
    gu.configure_decoder(dec, g)
    fc = kw.pop('field_config', None) or dec.FieldConfig()
    return dec.CifCaf(fc, keypoints=kc.keypoint_names(k), skeleton=skeleton, **kw)


# ---- a. stages ---------------------------------------------------------------------------

@pytest.mark.parametrize('fx', FIXTURES, ids=FIDS)
def test_stages_vs_reference(dec, fx):
    g = kc.load_fixture(fx)
    cif, caf, skeleton = gu.case_inputs(g)
    gu.configure_decoder(dec, g)
    fc = dec.FieldConfig()
    hr = dec.CifHr(fc).fill([cif, caf]).accumulated
    assert hr.shape[0] == int(g['K'])
    assert gu.sha(hr) == str(g['cifhr_sha'])
    seeds = dec.CifSeeds(hr, fc).fill([cif, caf]).get()
    rows = np.array([tuple(float(t) for t in s) for s in seeds], np.float32).reshape(-1, 5)
    assert np.array_equal(rows, g['seeds'])
    for tag, th in (('a', None), ('b', 0.0001)):
        cs = dec.CafScored(hr, fc, skeleton, score_th=th).fill([cif, caf])
        assert [f.shape[1] for f in cs.forward] == list(g['caf_%s_fwd_counts' % tag])
        assert [b.shape[1] for b in cs.backward] == list(g['caf_%s_bwd_counts' % tag])
        assert [gu.sha(f) for f in cs.forward] == [str(s) for s in g['caf_%s_fwd_sha' % tag]]
        assert [gu.sha(b) for b in cs.backward] == [str(s) for s in g['caf_%s_bwd_sha' % tag]]


# ---- b. single-image decodes ---------------------------------------------------------------

@pytest.mark.parametrize('fx', FIXTURES, ids=FIDS)
def test_decode_vs_reference_and_oracle(dec, fx):
    g = kc.load_fixture(fx)
    cif, caf, skeleton = gu.case_inputs(g)
    k = int(g['K'])
    cc = _cifcaf(dec, fx[0], g)
    recs, _, _ = cc.decode_records(cif[None], caf[None])
    recs = recs.copy()
    errs = gu.compare_annotations(g, recs)
    assert not errs, errs[:10]
    _same(recs, oracle.decode(cif, caf, skeleton, gu.case_config(g)))
    assert len(recs) >= (5 if str(g['generator']) == 'uniform' else 3)
    anns = cc([cif, caf])
    assert len(anns) == len(g['ann_score'])
    for a, r, s in zip(anns, recs, g['ann_score']):
        assert a.data.shape == (k, 3) and a.data.tobytes() == r['data'][:k].tobytes()
        assert a.score() == s


@pytest.mark.parametrize('hw', [kc.UNIFORM_SIZES[0], kc.UNIFORM_SIZES[2]], ids=['12x15', '31x34'])
@pytest.mark.parametrize('name', kc.NAMES)
def test_decode_uniform_sizes_vs_oracle(dec, name, hw):
    """Uniform eval at the two other sizes.  For k24c64, set A has 1,079 columns at 12x15
    (both LDS stagings hold them) and overflows them at 20x23 and above (global columns)."""
    cif, caf, skeleton = kc.inputs(name, 'uniform', *hw)
    cc = _cifcaf(dec, name, _mode('eval'))
    recs, _, _ = cc.decode_records(cif[None], caf[None])
    _same(recs, oracle.decode(cif, caf, skeleton, kc.config('eval')))
    if name == 'k24c64':
        assert recs['n_frontier'].max() >= 80
        if hw == (31, 34):
            assert len(recs) >= 50


@pytest.mark.parametrize('name', kc.NAMES)
def test_decode_planted_eval_vs_oracle(dec, name):
    k, _ = kc.case(name)
    cif, caf, skeleton = kc.inputs(name, 'planted', *kc.PLANTED_SIZE)
    cc = _cifcaf(dec, name, _mode('eval'))
    recs, _, _ = cc.decode_records(cif[None], caf[None])
    _same(recs, oracle.decode(cif, caf, skeleton, kc.config('eval')))
    assert len(recs) >= 3
    assert (recs['n_decoding'] == k - 1).any() == (name in kc.CONNECTED)


def test_decode_unconnected_joints(dec):
    """iso4: joint 4 has no edge, so force-complete cannot fill it and nothing grows from it;
    split6: the flood fill stays inside the seed's component."""
    for gen, h, w in (('uniform', 20, 23), ('planted',) + kc.PLANTED_SIZE):
        sets = {}
        for name in ('iso4', 'split6'):
            cif, caf, skeleton = kc.inputs(name, gen, h, w)
            recs, _, _ = _cifcaf(dec, name, _mode('eval')).decode_records(cif[None], caf[None])
            _same(recs, oracle.decode(cif, caf, skeleton, kc.config('eval')))
            sets[name] = recs['data'][:, :kc.case(name)[0], 2] > 0
        s = sets['iso4']
        assert (~s[:, 3] & s[:, :3].all(axis=1)).any()
        assert (s[:, 3] & ~s[:, :3].any(axis=1)).any()
        assert not (s[:, 3] & s[:, :3].any(axis=1)).any()
        a, b = sets['split6'][:, :3].any(axis=1), sets['split6'][:, 3:].any(axis=1)
        assert (a & ~b).any() and (b & ~a).any() and not (a & b).any()


# ---- c. batches: every image against the oracle ---------------------------------------------

def _ext_workgroups(n_img):
    """External helper workgroups per image of the seed loop, as the launcher computes them
    (csrc/decode.hip seed_ext_per_image, kExtWgMax = 3)."""
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return max(0, min(3, cus // n_img - 1))


@pytest.mark.parametrize('n,ext', [(3, 3), (136, 0)])
@pytest.mark.parametrize('name', ['k24c64', 'k20c33', 'iso4', 'pair2'])
def test_batch_vs_oracle(dec, name, n, ext):
    """n = 3 runs seed_loop_ext_kernel (3 helper workgroups per image), n = 136 the one-CU
    seed_loop_kernel (none).  All images are checked, and a second decode of the batch
    returns the same bytes."""
    assert _ext_workgroups(n) == ext
    k, skeleton = kc.case(name)
    cif, caf = kc.uniform_kc_batch(k, len(skeleton), n, 20, 23, first_seed=100)
    cc = _cifcaf(dec, name, _mode('eval'))
    recs, offsets, _ = cc.decode_records(cif, caf)
    recs, offsets = recs.copy(), np.array(offsets)
    again, off2, _ = cc.decode_records(cif, caf)
    assert np.array_equal(offsets, off2) and recs.tobytes() == again.tobytes()
    cfg = kc.config('eval')
    for i in range(n):
        got = recs[offsets[i]:offsets[i + 1]]
        _same(got, oracle.decode(cif[i], caf[i], skeleton, cfg), i)
        assert (got['image'] == i).all()
    assert offsets[-1] >= 2 * n


def test_repeated_pairs_batch_vs_oracle(dec):
    """kc.REPEATED (an unordered pair twice: a later by_source entry overwrites the earlier
    one in place, csrc/by_source.hpp through decode.hip's grow_args) as 3-image uniform 20x23
    eval batches, so seed_loop_ext_kernel runs: every image the oracle's bytes, twice."""
    assert _ext_workgroups(3) == 3
    cfg = kc.config('eval')
    gu.configure_decoder(dec, _mode('eval'))
    for name, (k, skeleton) in sorted(kc.REPEATED.items()):
        cif, caf = kc.uniform_kc_batch(k, len(skeleton), 3, 20, 23, first_seed=0)
        refs = [oracle.decode(cif[i], caf[i], skeleton, cfg) for i in range(3)]
        assert len(refs[0]) == {'rep3': 5, 'rep4': 9}[name]
        cc = dec.CifCaf(dec.FieldConfig(), keypoints=kc.keypoint_names(k), skeleton=skeleton)
        for run in range(2):
            recs, offsets, _ = cc.decode_records(cif, caf)
            for i, ref in enumerate(refs):
                got = recs[offsets[i]:offsets[i + 1]]
                assert len(got) == len(ref), (name, run, i, len(got), len(ref))
                for key in KEYS:
                    assert got[key].tobytes() == ref[key].tobytes(), (name, run, i, key)
                assert (got['image'] == i).all()


# ---- d. variants -----------------------------------------------------------------------------

@pytest.mark.parametrize('gen,mode', [('uniform', 'eval'), ('planted', 'eval'),
                                      ('planted', 'predict')])
@pytest.mark.parametrize('name', kc.VARIANT_CASES)
def test_variants_vs_oracle(dec, name, gen, mode):
    """connection_method 'max', greedy, confidence_scales of length C and a seed_mask that
    clears fields 0 and K - 1, in eval and predict defaults."""
    h, w = (20, 23) if gen == 'uniform' else kc.PLANTED_SIZE
    cif, caf, skeleton = kc.inputs(name, gen, h, w)
    k = kc.case(name)[0]
    for tag, kw in variant_configs(name).items():
        g = _mode(mode, kw.get('connection_method', 'blend'), int(kw.get('greedy', False)))
        fc = dec.FieldConfig(seed_mask=kw['seed_mask']) if 'seed_mask' in kw else None
        cc = _cifcaf(dec, name, g, field_config=fc,
                     confidence_scales=kw.get('confidence_scales'))
        recs, _, _ = cc.decode_records(cif[None], caf[None])
        ref = oracle.decode(cif, caf, skeleton, kc.config(mode, **kw))
        _same(recs, ref, tag)
        assert len(ref) >= 3, tag
        if tag == 'seedmask':
            # no annotation starts from a masked field: each one's first decoding source is
            # the seed joint (an annotation that never grew has a single joint set)
            first = np.where(ref['n_decoding'] > 0, ref['decoding_pairs'][:, 0, 0], -1)
            assert not np.isin(first, (0, k - 1)).any()


def _initial_records(name, gen, h, w, cfg):
    """Three annotations of another image's decode, shifted and cut to the first half of
    the joints (their decoding orders cut to match): the grow has work to do."""
    k, skeleton = kc.case(name)
    cif, caf, _ = kc.inputs(name, gen, h, w, seed=41)
    take = oracle.decode(cif, caf, skeleton, cfg)[:3].copy()
    assert len(take) >= 2
    cut = max(1, k // 2)
    take['data'][:, :, 0] += np.where(take['data'][:, :, 2] > 0, np.float32(2.5), 0)
    take['data'][:, cut:, :] = 0.0
    take['joint_scales'][:, cut:] = 0.0
    take['n_frontier'] = 0
    take['frontier_pairs'] = 0
    take['score'] = 0.0
    for r in take:
        nd = int(r['n_decoding'])
        # entries between joints that are kept and still set (NMS zeroes some), so that the
        # grown order stays within the record's K entries
        sel = [t for t in range(nd) if (r['decoding_pairs'][t] < cut).all() and
               (r['data'][r['decoding_pairs'][t].astype(int), 2] > 0).all()]
        pairs, xyv = r['decoding_pairs'][sel].copy(), r['decoding_xyv'][sel].copy()
        r['decoding_pairs'][:] = 0
        r['decoding_xyv'][:] = 0
        r['decoding_pairs'][:len(sel)] = pairs
        r['decoding_xyv'][:len(sel)] = xyv
        r['n_decoding'] = len(sel)
    return take


@pytest.mark.parametrize('name', kc.VARIANT_CASES)
def test_initial_annotations_vs_oracle(dec, name):
    from openpifpaf_amd.annotation import Annotation
    k, skeleton = kc.case(name)
    cfg = kc.config('eval')
    cif, caf, _ = kc.inputs(name, 'uniform', 20, 23)
    init_recs = _initial_records(name, 'uniform', 20, 23, cfg)
    init = [Annotation.from_record(r, kc.keypoint_names(k), skeleton) for r in init_recs]
    cc = _cifcaf(dec, name, _mode('eval'))
    anns = cc([cif, caf], initial_annotations=init)
    ref, idx = oracle.decode_initial(cif, caf, skeleton, init_recs, cfg)
    got = gu.annotations_as_records(anns, k)
    for key in KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), key
    ident = [next((i for i, a0 in enumerate(init) if a0 is a), -1) for a in anns]
    assert np.array_equal(np.where(idx < len(init), idx, -1), ident)
    assert max(ident) >= 0  # an initial annotation survived, as the caller's own object


# ---- e. shape switching on one engine --------------------------------------------------------

def test_shape_switching_on_one_engine(dec):
    """k24c64, pair2, COCO's p40_s0_eval, then k24c64 again through the same DecodeEngine:
    each result equals the reference's (what a fresh process decodes), so no workspace or
    zero region is sized by the K or C of the decode before."""
    from openpifpaf_amd import constants, engine
    assert engine.engine() is engine.engine()
    big = ('k24c64', 'u20x23', 'eval')
    for fx in (big, ('pair2', 'u20x23', 'eval'), None, big):
        if fx is None:
            g = gu.load_case('p40_s0_eval')
            cif, caf, skeleton = gu.case_inputs(g)
            gu.configure_decoder(dec, g)
            cc = dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                            skeleton=skeleton)
        else:
            g = kc.load_fixture(fx)
            cif, caf, skeleton = gu.case_inputs(g)
            cc = _cifcaf(dec, fx[0], g)
        recs, _, _ = cc.decode_records(cif[None], caf[None])
        errs = gu.compare_annotations(g, recs)
        assert not errs, (fx, errs[:10])
        _same(recs, oracle.decode(cif, caf, skeleton, gu.case_config(g)), fx)


# ---- f. compact records ----------------------------------------------------------------------

@pytest.mark.parametrize('name', kc.NAMES)
def test_packed_record_size(name):
    from openpifpaf_amd._abi import PACK_ALL, PP_PACK_DECODING, PP_PACK_FRONTIER, packed_dtype
    from openpifpaf_amd._lib import load
    k, skeleton = kc.case(name)
    c = len(skeleton)
    for flags in (0, PP_PACK_DECODING, PP_PACK_FRONTIER, PACK_ALL):
        dt = packed_dtype(k, c, flags)
        assert dt.itemsize == load().pp_packed_record_size(k, c, flags), flags
        assert dt.itemsize % 16 == 0
        assert dt['data'].shape == (k, 3)
        if flags & PP_PACK_FRONTIER:
            assert dt['frontier_pairs'].shape == (4 * c, 2)


@pytest.mark.parametrize('name', kc.NAMES)
def test_compact_records_equal_full(dec, name):
    """Compact records of every flag set against the full ones of the same decode, and
    distributed.expand_compact back to full records."""
    import torch
    from test_gpu_parity import _compact_vs_full
    from openpifpaf_amd import engine
    from openpifpaf_amd._abi import PACK_ALL, PP_PACK_DECODING, PP_PACK_FRONTIER, packed_dtype
    from openpifpaf_amd.distributed import expand_compact
    k, skeleton = kc.case(name)
    c = len(skeleton)
    cif, caf = kc.uniform_kc_batch(k, c, 3, 20, 23, first_seed=100)
    eng = engine.DecodeEngine()
    b = eng.launch(torch.from_numpy(cif).cuda(), torch.from_numpy(caf).cuda(), skeleton,
                   kc.config('eval'))
    full, off = eng.fetch_gather(b)
    full = full.copy()
    assert len(full) >= 6
    for flags in (PACK_ALL, PP_PACK_DECODING, PP_PACK_FRONTIER, 0):
        got, got_off = eng.fetch_async(b, (k, c, flags), capacity=len(full)).result()
        assert got.dtype == packed_dtype(k, c, flags)
        assert np.array_equal(off, got_off)
        assert np.array_equal(got['data'], full['data'][:, :k])
        assert np.array_equal(got['joint_scales'], full['joint_scales'][:, :k])
        assert np.array_equal(got['score'], full['score'])
        assert np.array_equal(got['image'], full['image'])
        if flags == PACK_ALL:
            _compact_vs_full(full, got, k=k, skeleton=skeleton)
            back = expand_compact(got, k, c)
            _same(back, full)
            for r, f in zip(back, full):
                nd, nf = int(f['n_decoding']), int(f['n_frontier'])
                assert r['decoding_xyv'][:nd].tobytes() == f['decoding_xyv'][:nd].tobytes()
                assert np.array_equal(r['frontier_pairs'][:nf], f['frontier_pairs'][:nf])
    # the API's own path fetches compact records
    cc = _cifcaf(dec, name, _mode('eval'))
    per_image = cc.decode_batch(cif, caf)
    assert [len(a) for a in per_image] == np.diff(off).tolist()
    flat = [a for anns in per_image for a in anns]
    for a, f in zip(flat, full):
        assert a.data.tobytes() == f['data'][:k].tobytes()
        assert len(a.frontier_order) == int(f['n_frontier'])
        assert a.score() == f['score']


# ---- g. multi-scale ----------------------------------------------------------------------------

def test_multi_scale_vs_reference_and_oracle(dec):
    """The ms2 FieldConfig with K = 24, C = 64 through pp_decode_multi (the seeds sort has
    heads x K segments): stages and annotations of the reference, records of the oracle."""
    name, multi, _ = kc.MULTI_FIXTURE
    g = kc.load_fixture(kc.MULTI_FIXTURE)
    k, skeleton = kc.case(name)
    fields, kw = kc.multi_case(name, multi)
    assert gu.sha(*fields) == str(g['input_sha'])
    fc = dec.FieldConfig(**kw)
    cc = _cifcaf(dec, name, g, field_config=fc)
    hr = dec.CifHr(fc).fill(fields).accumulated
    assert list(hr.shape) == list(g['cifhr_shape'])
    assert gu.sha(hr) == str(g['cifhr_sha'])
    seeds = dec.CifSeeds(hr, fc).fill(fields).get()
    rows = np.array([tuple(float(t) for t in s) for s in seeds], np.float32).reshape(-1, 5)
    assert np.array_equal(rows, g['seeds'])
    for tag, th in (('a', None), ('b', 0.0001)):
        cs = dec.CafScored(hr, fc, skeleton, score_th=th).fill(fields)
        assert [f.shape[1] for f in cs.forward] == list(g['caf_%s_fwd_counts' % tag])
        assert [gu.sha(f) for f in cs.forward] == [str(s) for s in g['caf_%s_fwd_sha' % tag]]
        assert [gu.sha(b) for b in cs.backward] == [str(s) for s in g['caf_%s_bwd_sha' % tag]]
    recs, _, _ = cc.decode_fields_records([f[None] for f in fields])
    recs = recs.copy()
    errs = gu.compare_annotations(g, recs)
    assert not errs, errs[:10]
    assert len(recs) >= 3
    _same(recs, oracle.decode_multi(oracle.Members(fields, **kw), skeleton, gu.case_config(g)))
    anns = cc(fields)
    assert [a.score() for a in anns] == g['ann_score'].tolist()


# ---- h. standalone NMS and inverse -------------------------------------------------------------

def _device_nms(data, scales, k, cfg):
    """pp_nms_keypoints over one group -> (survivors' input indices, their records, the
    input records as the kernel left them)."""
    import torch
    from openpifpaf_amd import _device
    from openpifpaf_amd._abi import ANN_DTYPE
    from openpifpaf_amd._lib import call, load
    n = len(data)
    recs = np.zeros(n, ANN_DTYPE)
    recs['data'][:, :k] = data
    recs['joint_scales'][:, :k] = scales
    recs['n_keypoints'] = k
    d_in = torch.from_numpy(recs.view(np.uint8).reshape(n, ANN_DTYPE.itemsize)).cuda()
    d_out = torch.zeros_like(d_in)
    d_counts = torch.tensor([n], dtype=torch.int32, device='cuda')
    d_out_counts = torch.zeros(1, dtype=torch.int32, device='cuda')
    d_index = torch.zeros(n, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(load().pp_nms_workspace_size(1, n)), dtype=torch.uint8, device='cuda')
    call('pp_nms_keypoints', _device.ptr(d_in), _device.ptr(d_counts), 1, k, n,
         ctypes.byref(cfg), _device.ptr(d_out), _device.ptr(d_out_counts), _device.ptr(d_index),
         _device.ptr(ws), ctypes.c_size_t(ws.numel()), _device.stream())
    m = int(d_out_counts.cpu().item())
    out = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=ANN_DTYPE)[:m]
    edited = np.frombuffer(d_in.cpu().numpy().tobytes(), dtype=ANN_DTYPE)
    return d_index[:m].cpu().numpy(), out, edited


@pytest.mark.parametrize('k', NMS_K)
def test_nms_keypoints_vs_oracle(dec, k):
    """pp_nms_keypoints (pw_sum's K < 8 branch, whole blocks of 8 and a tail) and
    nms.Keypoints().annotations on 200 poses with tied scores."""
    from openpifpaf_amd._abi import make_config
    from openpifpaf_amd.annotation import Annotation
    kps = kc.keypoint_names(k)
    skeleton = [(j, j + 1) for j in range(1, k)] or [(1, 1)]
    for kt, it, sup in NMS_CFGS:
        data, scales = nms_poses(k)
        order, ref = oracle.nms_keypoints(data, scales, kt, it, sup)
        want = np.array([oracle.ann_score(d[:, 2]) for d in ref['data'][:, :k]])
        assert (np.diff(want) == 0).sum() >= 10
        cfg = make_config(nms_keypoint_threshold=kt, nms_instance_threshold=it,
                          nms_suppression=sup)
        index, out, edited = _device_nms(data, scales, k, cfg)
        assert index.tolist() == order.tolist()
        assert np.array_equal(out['data'], ref['data'])
        assert np.array_equal(out['score'], want)
        assert np.array_equal(edited['data'][order], ref['data'])
        anns = []
        for d, sc in zip(data, scales):
            a = Annotation(kps, skeleton)
            a.data, a.joint_scales = d.copy(), sc.copy()
            anns.append(a)
        nms = dec.nms.Keypoints()
        nms.keypoint_threshold, nms.instance_threshold, nms.suppression = kt, it, sup
        res = nms.annotations(list(anns))
        ids = {id(a): i for i, a in enumerate(anns)}
        assert [ids[id(a)] for a in res] == order.tolist()
        assert np.array_equal(np.stack([a.data for a in res]), ref['data'][:, :k])
        assert np.array_equal(np.stack([a.data for a in anns]), edited['data'][:, :k])
        assert np.array_equal(np.array([a.score() for a in res]), want)


@pytest.mark.parametrize('name', ['chain5', 'k24c64'])
def test_annotations_inverse_vs_oracle(dec, name):
    """Preprocess.annotations_inverse (pp_annotations_inverse) on decoded poses of K = 5 and
    K = 24 under a shift / scale, an hflip with a swap table and a rotation."""
    from openpifpaf_amd import transforms
    k, skeleton = kc.case(name)
    kps = kc.keypoint_names(k)
    cif, caf, _ = kc.inputs(name, 'planted', *kc.PLANTED_SIZE)
    anns = _cifcaf(dec, name, _mode('eval'))([cif, caf])
    assert len(anns) >= 3 and max(len(a.decoding_order) for a in anns) == k - 1
    # keypoints 2j+1 <-> 2j+2 swap (the last of an odd K stays)
    hflip = {}
    for j in range(0, k - 1, 2):
        hflip[kps[j]], hflip[kps[j + 1]] = kps[j + 1], kps[j]
    swap = transforms._HorizontalSwap(kps, hflip)
    table = transforms.swap_table(swap, k)
    assert sorted(table.tolist()) == list(range(k)) and (table != np.arange(k)).sum() >= k - 1
    base = {'offset': np.array((3.5, -2.25)), 'scale': np.array((0.5, 0.75)),
            'rotation': {'angle': 0.0, 'width': None, 'height': None}, 'hflip': False,
            'width_height': np.array((641, 427)), 'image_id': 7}
    metas = {'shift': base, 'flip': dict(base, hflip=True, horizontal_swap=swap),
             'rot': dict(base, rotation={'angle': 12.5, 'width': 481, 'height': 361},
                         offset=np.array((-1.0, 4.5)), scale=np.array((1.25, 0.8)))}
    data = np.stack([a.data for a in anns])
    scales = np.stack([a.joint_scales for a in anns])
    nd = np.array([len(a.decoding_order) for a in anns])
    dxyv = np.zeros((len(anns), k, 6), np.float32)
    for i, a in enumerate(anns):
        for t, (_, __, c1, c2) in enumerate(a.decoding_order):
            dxyv[i, t, :3], dxyv[i, t, 3:] = c1, c2
    for tag, meta in metas.items():
        inv = transforms.Preprocess.annotations_inverse(anns, meta)
        want = oracle.annotations_inverse(data, scales, dxyv, nd, meta,
                                          table if meta['hflip'] else None)
        assert np.array_equal(np.stack([a.data for a in inv]), want[0]), tag
        assert np.array_equal(np.stack([a.joint_scales for a in inv]), want[1]), tag
        got = np.zeros_like(dxyv)
        for i, a in enumerate(inv):
            for t, (_, __, c1, c2) in enumerate(a.decoding_order):
                got[i, t, :3], got[i, t, 3:] = c1[:3], c2[:3]
        assert np.array_equal(got, want[2]), tag
        assert np.array_equal(np.stack([a.data for a in anns]), data)  # inputs untouched


# ---- the envelope on the device entry points -----------------------------------------------

def test_envelope_refused(dec):
    """pp_decode_batch refuses K = 25, C = 65 and a skeleton index above K before it
    launches anything; the engine refuses caf.shape[1] != len(skeleton); K = 24 with C = 64
    decodes."""
    import torch
    from openpifpaf_amd import _device, engine
    from openpifpaf_amd._abi import ANN_DTYPE, skeleton_array
    from openpifpaf_amd._lib import PPError, call
    cfg = kc.config('eval')
    cap = 16
    anns = torch.zeros(cap * ANN_DTYPE.itemsize, dtype=torch.uint8, device='cuda')
    counts = torch.zeros(1, dtype=torch.int32, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')

    def fields(k, c):
        return (torch.zeros((1, k, 5, 6, 7), device='cuda'),
                torch.zeros((1, c, 9, 6, 7), device='cuda'))

    def raw(k, c, skeleton):
        cif, caf = fields(k, c)
        skel = skeleton_array(skeleton)
        call('pp_decode_batch', _device.ptr(cif), _device.ptr(caf), 1, k, c, 6, 7,
             skel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cfg), _device.ptr(None),
             _device.ptr(anns), cap, _device.ptr(counts), _device.ptr(status), _device.ptr(ws),
             ctypes.c_size_t(ws.numel()), _device.stream())

    with pytest.raises(PPError, match='PP_ESHAPE.*K <= PP_MAX_KP, C <= PP_MAX_EDGES'):
        raw(25, 24, [(1, j) for j in range(2, 26)])
    pairs = [(a, b) for a in range(1, 25) for b in range(a + 1, 25)][:65]
    with pytest.raises(PPError, match='PP_ESHAPE.*K <= PP_MAX_KP, C <= PP_MAX_EDGES'):
        raw(24, 65, pairs)
    with pytest.raises(PPError, match='PP_EINVAL.*skeleton joint index out of 1..K'):
        raw(5, 4, [(1, 2), (2, 3), (3, 4), (4, 6)])
    eng = engine.DecodeEngine()
    with pytest.raises(ValueError, match='skeleton has 4 edges but caf has 5 fields'):
        eng.decode(*fields(5, 5), kc.case('chain5')[1], cfg)
    recs, offsets, _ = eng.decode(*fields(24, 64), kc.case('k24c64')[1], cfg)
    assert len(recs) == 0 and list(offsets) == [0, 0]
