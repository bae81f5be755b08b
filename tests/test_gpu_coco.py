"""COCO prediction records on the device (pp_coco_keypoints / pp_coco_dets, csrc/coco.hip):
byte for byte the host twins' records, the reference's json text on its fixture, the
decode's records untouched, and the decoders' coco_batch against the per-image route
(decode_batch, then eval_coco.coco_predictions).  All comparisons are exact."""
import ctypes
import json

import numpy as np
import pytest

import coco_util
from openpifpaf_amd import _abi, eval_coco
from openpifpaf_amd._abi import PP_COCO_EMPTY, PP_COCO_NAN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


@pytest.fixture(scope='module')
def fx():
    return coco_util.load_fixture()


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        return torch.from_numpy(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))).cuda()
    return torch.from_numpy(a).cuda()


def _device_records(torch, recs, counts, metas, ids, hswap, **kw):
    d = _dev(torch, recs)
    before = d.clone()
    got = eval_coco.coco_records(d, _dev(torch, counts), _dev(torch, metas).reshape(-1),
                                 _dev(torch, np.asarray(ids, np.int64)),
                                 hswap=None if hswap is None else _dev(torch, hswap), **kw)
    assert torch.equal(d, before)  # the decode's records are only read
    return got


def _same(got, want):
    assert got.offsets.tolist() == want.offsets.tolist()
    assert got.flags.tolist() == want.flags.tolist()
    assert got.records.tobytes() == want.records.tobytes()


# ---- 1. the reference's fixture ---------------------------------------------------------
@pytest.mark.parametrize('tag', ['coco', 'chain5'])
def test_fixture_parity(torch, fx, tag):
    recs, counts, metas, ids, hswap, k = coco_util.pose_batch(fx, tag)
    for key, th, cap in coco_util.param_sets(fx, tag):
        kw = dict(k=k, small_threshold=th, max_per_image=cap)
        got = _device_records(torch, recs, counts, metas, ids, hswap, **kw)
        _same(got, eval_coco.coco_records_cpu(recs, counts, metas, ids, hswap=hswap, **kw))
        assert coco_util.dumps(got.predictions()) == str(fx[key]), key


def test_fixture_parity_detections(torch, fx):
    recs, counts, metas, ids = coco_util.det_batch(fx)
    for cap in (20, 1):
        got = _device_records(torch, recs, counts, metas, ids, None, det=True, max_per_image=cap)
        _same(got, eval_coco.coco_records_cpu(recs, counts, metas, ids, det=True,
                                              max_per_image=cap))
        assert coco_util.dumps(got.predictions()) == str(fx['det_json_m%d' % cap])


# ---- 2. the shapes where the prefix and the packing can go wrong --------------------------
COUNTS = (257, 0, 1, 63, 64, 65, 255, 256, 300, 350)  # 350: above the capacity of 300


def _synthetic(k, n_img, seed):
    rng = np.random.default_rng(seed)
    counts = [COUNTS[i % len(COUNTS)] for i in range(n_img)]
    recs, counts = coco_util.random_poses(rng, n_img, 300, k, counts)
    metas = coco_util.random_metas(rng, n_img)
    ids = rng.integers(1, 1 << 40, n_img).astype(np.int64)
    hswap = coco_util.random_swap(rng, k)
    th = coco_util.split_threshold(recs, counts, metas, hswap, k)
    return recs, counts, metas, ids, hswap, th


@pytest.mark.parametrize('n_img', [1, 70])
@pytest.mark.parametrize('k', [2, 17, 24])
def test_synthetic_equals_twin(torch, k, n_img):
    recs, counts, metas, ids, hswap, th = _synthetic(k, n_img, 100 * k + n_img)
    if n_img > 1:
        recs['data'][5, 60, k - 1, 0] = np.nan  # image 5 (65 records): flagged
        assert metas['hflip'].any() and not metas['hflip'].all()
    for cap in (1, 20, 300):
        for small in (0.0, th):
            kw = dict(k=k, small_threshold=small, max_per_image=cap, category_id=2)
            got = _device_records(torch, recs, counts, metas, ids, hswap, **kw)
            want = eval_coco.coco_records_cpu(recs, counts, metas, ids, hswap=hswap, **kw)
            _same(got, want)
            if n_img > 1:
                assert (got.flags & PP_COCO_NAN).tolist() == [int(i == 5) for i in range(n_img)]
                assert got.flags[1] & PP_COCO_EMPTY
    kept = np.diff(eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, hswap=hswap,
                                              small_threshold=th, max_per_image=300).offsets)
    full = np.minimum(counts, 300)
    assert ((kept < full) | (full <= 1)).all() and (kept >= 1).all()
    assert (kept[full > 8] > 1).all()  # the threshold splits the images


@pytest.mark.parametrize('det', [False, True])
def test_out_capacity_one_short(torch, det):
    """out_capacity = total - 1: the counts are complete, the last record's slot keeps its
    fill, and nothing behind the block is written (device memory destination)."""
    from openpifpaf_amd import _device
    from openpifpaf_amd._lib import call, load
    k, n_img = 5, 7  # K odd: a 176-byte record; detections: 56 bytes (8 mod 16)
    recs, counts, metas, ids, _, _ = _synthetic(k, n_img, 77)
    if det:
        rng = np.random.default_rng(5)
        recs = np.zeros((n_img, 300), _abi.DET_DTYPE)
        recs['field'] = rng.integers(0, 3, recs.shape)
        recs['score'] = rng.random(recs.shape)
        recs['bbox'] = rng.uniform(1, 200, recs.shape + (4,))
    want = eval_coco.coco_records_cpu(recs, counts, metas, ids, k=k, det=det, max_per_image=20)
    width = want.records.dtype.itemsize
    total = int(want.offsets[-1])
    guard = 4096
    out = torch.full((total * width + guard,), 0xFF, dtype=torch.uint8, device='cuda')
    oc = torch.zeros(n_img, dtype=torch.int32, device='cuda')
    of = torch.zeros(n_img, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(load().pp_coco_workspace_size(n_img)), dtype=torch.uint8, device='cuda')
    params = _abi.CocoParams(0.0, 20, 1)
    d_recs, d_counts = _dev(torch, recs), _dev(torch, counts)
    d_metas, d_ids = _dev(torch, metas).reshape(-1), _dev(torch, ids)
    tail = (ctypes.byref(params), _device.ptr(out), total - 1, _device.ptr(oc), _device.ptr(of),
            _device.ptr(ws), _device.stream())
    if det:
        call('pp_coco_dets', _device.ptr(d_recs), _device.ptr(d_counts), n_img, 300,
             _device.ptr(d_metas), _device.ptr(d_ids), *tail)
    else:
        call('pp_coco_keypoints', _device.ptr(d_recs), _device.ptr(d_counts), n_img, 300, k,
             _device.ptr(d_metas), _device.ptr(d_ids), _device.ptr(None), *tail)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert oc.cpu().numpy().tolist() == np.diff(want.offsets).tolist()
    assert of.cpu().numpy().tolist() == want.flags.tolist()
    assert host[:(total - 1) * width].tobytes() == want.records[:total - 1].tobytes()
    assert (host[(total - 1) * width:] == 0xFF).all()


# ---- 3. end to end ------------------------------------------------------------------------
def _eval_defaults(dec):
    dec.CifHr.v_threshold = 0.1
    dec.CafScored.default_score_th = 0.1
    dec.CifSeeds.threshold = 0.2
    dec.CifCaf.force_complete = True
    dec.CifCaf.keypoint_threshold = 0.0
    dec.CifCaf.greedy = False
    dec.CifCaf.connection_method = 'blend'
    dec.nms.Keypoints.instance_threshold = 0.0
    dec.nms.Keypoints.keypoint_threshold = 0.0


def _metas(n, first_id):
    from test_oracle_golden import inverse_metas
    named = inverse_metas()
    return [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=first_id + i) for i in range(n)]


@pytest.fixture(scope='module')
def pose_cases(torch):
    """(batch records, per-image route) of the planted and the uniform batch, made once."""
    from openpifpaf_amd import constants, decoder as dec, synthetic
    _eval_defaults(dec)
    d = dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                   skeleton=constants.COCO_PERSON_SKELETON)
    out = {}
    for name, kind, n, h, w, params in (('planted', 'planted', 6, 33, 40, {}),
                                        ('uniform', 'uniform', 3, 20, 23,
                                         {'max_per_image': 3})):
        cif, caf = synthetic.batch(kind, n, h, w)
        metas = _metas(n, 40)
        first = d.coco_batch(cif, caf, metas, **params)
        first_bytes = first.records.tobytes()
        second = d.coco_batch(cif, caf, metas, **params)
        anns = d.decode_batch(cif, caf)
        per_image = []
        for a, m in zip(anns, metas):
            per_image += eval_coco.coco_predictions(a, m, **params)
        out[name] = dict(first=first, first_bytes=first_bytes, second=second, anns=anns,
                         per_image=per_image, dec=d, cif=cif, caf=caf, metas=metas, params=params)
    dec.CifSeeds.threshold = None
    return out


@pytest.mark.parametrize('name', ['planted', 'uniform'])
def test_coco_batch_equals_per_image_route(torch, pose_cases, name):
    c = pose_cases[name]
    got = c['first'].predictions()
    assert coco_util.dumps(got) == coco_util.dumps(c['per_image'])
    assert len(got) > len(c['metas'])  # more than one record per image somewhere
    assert c['second'].records.tobytes() == c['first_bytes']
    assert c['second'].offsets.tolist() == c['first'].offsets.tolist()
    if name == 'uniform':
        assert np.diff(c['first'].offsets).max() == 3 and max(len(a) for a in c['anns']) > 3


def test_decode_after_coco_batch_unaffected(torch, pose_cases):
    from openpifpaf_amd import decoder as dec
    c = pose_cases['planted']
    _eval_defaults(dec)
    again = c['dec'].decode_batch(c['cif'], c['caf'])
    dec.CifSeeds.threshold = None
    assert [len(a) for a in again] == [len(a) for a in c['anns']]
    for la, lb in zip(again, c['anns']):
        for a, b in zip(la, lb):
            assert a.data.tobytes() == b.data.tobytes()
            assert a.joint_scales.tobytes() == b.joint_scales.tobytes()


def test_coco_batch_needs_device_nms(torch):
    from openpifpaf_amd import constants, decoder as dec, synthetic

    class HostNms:
        def annotations(self, anns):
            return anns
    d = dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                   skeleton=constants.COCO_PERSON_SKELETON, nms=HostNms())
    cif, caf = synthetic.batch('planted', 1, 20, 23)
    with pytest.raises(TypeError):
        d.coco_batch(cif, caf, _metas(1, 1))


def test_cifdet_coco_batch(torch):
    from openpifpaf_amd import decoder as dec, synthetic
    dec.CifHr.v_threshold = 0.1
    dec.CifSeeds.threshold = 0.5
    d = dec.CifDet(dec.FieldConfig(), ['c0', 'c1', 'c2'])
    det = synthetic.det_batch('planted', 3, 40, 40, first_seed=0, n_categories=3)
    metas = _metas(3, 90)
    for m in metas:
        m.pop('horizontal_swap', None)
    got = d.coco_batch(det, metas, max_per_image=5)
    per_image = []
    for a, m in zip(d.decode_batch(det), metas):
        per_image += eval_coco.coco_predictions(a, m, max_per_image=5)
    dec.CifSeeds.threshold = None
    assert coco_util.dumps(got.predictions()) == coco_util.dumps(per_image)
    assert len(per_image) > 3


# ---- 4. the prediction files ----------------------------------------------------------------
def test_write_predictions(torch, pose_cases, tmp_path):
    import zipfile
    c = pose_cases['planted']
    p = eval_coco.Predictions().from_batch(c['first'])
    assert p.image_ids == [m['image_id'] for m in c['metas']]
    name = str(tmp_path / 'out')
    p.write_predictions(name)
    want = [{k: v for k, v in r.items() if k in ('image_id', 'category_id', 'keypoints', 'score')}
            for r in c['per_image']]
    with open(name + '.pred.json') as f:
        assert json.load(f) == json.loads(json.dumps(want))
    with zipfile.ZipFile(name + '.zip') as z:
        assert z.namelist() == ['predictions.json']
        assert json.loads(z.read('predictions.json')) == json.loads(json.dumps(want))
