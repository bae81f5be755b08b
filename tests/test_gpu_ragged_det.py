"""pp_cifdet_decode_ragged on the device (engine.RaggedDetFields, CifDet.decode_ragged /
coco_ragged, heads.RaggedDetCollector): CifDet images of different field sizes decoded as one
batch, each exactly as it decodes alone at its own size.  The reference of every device result
is the C oracle on the image alone (oracle.cifdet_decode / cifdet_hr); every comparison is of
bytes.  And the sort of more than 4,096 seeds per field through both entry points."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import ragged_det_util as rd

pytestmark = pytest.mark.gpu

TWELVE = [(s, seed) for seed in (0, 1) for s in rd.SHAPES]
CATS = ['c0', 'c1', 'c2']


@pytest.fixture
def dec():
    """The decoder package with the class attributes a CifDet decode reads at the reference's
    defaults and CifHr.v_threshold 0.1 (whatever earlier tests left behind);
    CifSeeds.threshold is each test's."""
    from openpifpaf_amd import decoder
    wanted = [(decoder.CifHr, 'v_threshold', rd.CIF_THRESHOLD), (decoder.CifHr, 'neighbors', 16),
              (decoder.CifSeeds, 'threshold', None), (decoder.CifSeeds, 'score_scale', 1.0),
              (decoder.nms.Detection, 'suppression', 0.1),
              (decoder.nms.Detection, 'suppression_soft', 0.3),
              (decoder.nms.Detection, 'instance_threshold', 0.1),
              (decoder.nms.Detection, 'iou_threshold', 0.7),
              (decoder.nms.Detection, 'iou_threshold_soft', 0.5)]
    before = [(obj, name, getattr(obj, name)) for obj, name, _ in wanted]
    for obj, name, value in wanted:
        setattr(obj, name, value)
    yield decoder
    for obj, name, value in before:
        setattr(obj, name, value)


def _cifdet(dec, kind, k=rd.K, seed_threshold=None):
    dec.CifSeeds.threshold = rd.SEED_THRESHOLD[kind] if seed_threshold is None else seed_threshold
    return dec.CifDet(dec.FieldConfig(), ['c%d' % i for i in range(k)])


def _device_fields(kind, shapes_seeds, k=rd.K):
    """One field list per image ([det (k, 7, h, w)]) on the device."""
    import torch
    return [[torch.from_numpy(rd.image(kind, h, w, seed, k).copy()).cuda()]
            for (h, w), seed in shapes_seeds]


def _check_records(recs, offsets, kind, shapes_seeds, k=rd.K, seed_threshold=None,
                   instance_threshold=None):
    assert len(offsets) == len(shapes_seeds) + 1
    counts = []
    for i, ((h, w), seed) in enumerate(shapes_seeds):
        want = rd.own_decode(kind, h, w, seed, k, seed_threshold, instance_threshold)
        rd.assert_same_records(recs[offsets[i]:offsets[i + 1]], want, i)
        counts.append(len(want))
    return counts


# ---- 1. the stages: the dense map of the first stage --------------------------------------
def test_stages_cifhr_map(dec):
    """12 uniform images in a 24x30 container: d_cifhr inside each image's own H' x W' is
    oracle.cifdet_hr's bytes, every other element of the NaN-filled buffer is +0.0f."""
    import torch
    from openpifpaf_amd import _device, engine
    from openpifpaf_amd._abi import DET_DTYPE
    from openpifpaf_amd._lib import call, load
    from openpifpaf_amd.decoder.generator.cifdet import det_nms_config
    ragged = engine.RaggedDetFields([f[0] for f in _device_fields('uniform', TWELVE)])
    n, k, h, w = ragged.n, ragged.k, ragged.h, ragged.w
    assert (n, k, h, w) == (12, rd.K) + rd.CONTAINER
    cfg, z, cap = rd.config('uniform'), det_nms_config(), h * w
    hh, ww = (h - 1) * cfg.stride + 1, (w - 1) * cfg.stride + 1
    pitch = int(load().pp_cifhr_pitch(ww))
    hr = torch.full((n, k, hh, pitch), float('nan'), device='cuda')
    ws = torch.empty(int(load().pp_cifdet_ragged_workspace_size(n, k, h, w, ctypes.byref(cfg),
                                                                cap)),
                     dtype=torch.uint8, device='cuda')
    out = torch.empty((n, cap, DET_DTYPE.itemsize), dtype=torch.uint8, device='cuda')
    counts = torch.empty(n, dtype=torch.int32, device='cuda')
    status = torch.empty(n, dtype=torch.int32, device='cuda')
    call('pp_cifdet_decode_ragged', _device.ptr(ragged.det), n, k, h, w,
         _device.ptr(ragged.extents), ragged.extents_host.ctypes.data_as(ctypes.c_void_p),
         ctypes.byref(cfg), ctypes.byref(z), _device.ptr(hr), _device.ptr(out), cap,
         _device.ptr(counts), _device.ptr(status), _device.ptr(ws),
         ctypes.c_size_t(ws.numel()), _device.stream())
    assert status.cpu().numpy().tolist() == [0] * n
    bits = hr.cpu().numpy().view(np.uint32)
    for i, ((hi, wi), seed) in enumerate(TWELVE):
        want = rd.own_hr('uniform', hi, wi, seed)
        ho, wo = want.shape[1:]
        assert (ho, wo) == ((hi - 1) * cfg.stride + 1, (wi - 1) * cfg.stride + 1)
        assert bits[i, :, :ho, :wo].tobytes() == want.view(np.uint32).tobytes(), i
        outside = np.ones((hh, pitch), bool)
        outside[:ho, :wo] = False
        assert not bits[i][:, outside].any(), i  # +0.0f, bit for bit
    # the records of the same call
    host, cnt = out.cpu().numpy(), counts.cpu().numpy()
    for i, ((hi, wi), seed) in enumerate(TWELVE):
        got = np.frombuffer(host[i, :cnt[i]].tobytes(), dtype=DET_DTYPE)
        rd.assert_same_records(got, rd.own_decode('uniform', hi, wi, seed), i)


# ---- 2. the records -----------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['uniform', 'planted'])
def test_records(dec, kind):
    """The 12 images through CifDet.decode_ragged against the oracle, twice on one CifDet."""
    cd = _cifdet(dec, kind)
    fields = _device_fields(kind, TWELVE)
    recs, offsets = cd.decode_ragged_records(fields)
    counts = _check_records(recs, offsets, kind, TWELVE)
    print(kind, 'detections per image', counts)
    assert min(counts) >= 1
    again, again_off = cd.decode_ragged_records(fields)
    assert again.tobytes() == recs.tobytes() and again_off.tolist() == offsets.tolist()
    anns = cd.decode_ragged(fields)
    assert [len(a) for a in anns] == counts
    for i, image_anns in enumerate(anns):
        got = recs[offsets[i]:offsets[i + 1]]
        assert [a.field_i for a in image_anns] == got['field'].tolist()
        assert np.array([a.score for a in image_anns], np.float32).tobytes() == \
            got['score'].tobytes()


# ---- 3. the smallest extents --------------------------------------------------------------
def test_smallest_extents(dec):
    """(1, 1), (1, 6), (2, 7), (3, 4) and (5, 5) in one 5x7 container: an image's own occupancy
    grid has zero rows or columns (every seed free) while the container's has not.  An image
    of one row has H' = 1, so scalar_values gives its default for every y but 0 and no seed
    reaches v > 0.1: those images decode to nothing at the usual thresholds, and the batch is
    decoded again with seed threshold 0 and nms.Detection.instance_threshold 0, where every
    cell of theirs is a seed, free, and a record."""
    from openpifpaf_amd import engine
    cases = [(s, seed) for seed in (0, 1, 2) for s in rd.SMALL]
    cd = _cifdet(dec, 'uniform')
    ragged = engine.RaggedDetFields([f[0] for f in _device_fields('uniform', cases)])
    assert (ragged.h, ragged.w) == (5, 7)
    recs, offsets = cd.decode_ragged_records(ragged)
    counts = _check_records(recs, offsets, 'uniform', cases)
    print('detections per image', counts)
    assert sum(counts) >= 10
    dec.nms.Detection.instance_threshold = 0.0
    cd = _cifdet(dec, 'uniform', seed_threshold=0.0)
    recs, offsets = cd.decode_ragged_records(ragged)
    counts = _check_records(recs, offsets, 'uniform', cases, seed_threshold=0.0,
                            instance_threshold=0.0)
    print('detections per image, thresholds 0', counts)
    assert all(counts[i] >= 1 for i, (s, _) in enumerate(cases) if s[0] == 1)


# ---- 4. equal shapes ----------------------------------------------------------------------
def test_equal_shapes_give_the_uniform_decode(dec):
    import torch
    cases = [(rd.CONTAINER, seed) for seed in range(4)]
    cd = _cifdet(dec, 'uniform')
    fields = _device_fields('uniform', cases)
    want, want_off = cd.decode_records(torch.stack([f[0] for f in fields]))
    got, got_off = cd.decode_ragged_records(fields)
    assert got_off.tolist() == want_off.tolist() and want_off[-1] >= 4
    assert got.tobytes() == want.tobytes()


# ---- 5. from the head's conv outputs ------------------------------------------------------
# quad 1 gives odd field sizes (2 n - 1): the odd sizes at or below ragged_util.SHAPES
ODD = [(13, 17), (17, 13), (13, 29), (13, 13), (21, 15), (23, 29)]
# output channel [c, x, y, b, w, h, b2] -> concatenated channel (conf, 2 vectors, 2 logb)
PERM = (0, 1, 2, 5, 3, 4, 6)


def conv_from_det(det):
    """The inverse of the 'cifdet' ingest at quad 1: fields (K, 7, h, w), h and w odd -> the
    conv output (K * 7 * 4, (h + 1) / 2, (w + 1) / 2).  float64, rounded to float32."""
    f = np.asarray(det, np.float64)
    k, _, h, w = f.shape
    cat = np.empty_like(f)
    cat[:, list(PERM)] = f
    conf = np.clip(cat[:, :1], 1e-6, 1 - 1e-6)
    conf = np.log(conf / (1 - conf))
    yy, xx = np.indices((h, w), dtype=np.float64)
    vec = cat[:, 1:5].copy()
    vec[:, 0] -= xx  # the index grid is added to the first vector only
    vec[:, 1] -= yy
    groups = [g.reshape(-1, h, w) for g in (conf, vec, cat[:, 5:])]
    full = np.zeros((k * 7, h + 1, w + 1))  # the row and column PixelShuffle's crop drops
    full[:, :h, :w] = np.concatenate(groups)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    conv = full.reshape(k * 7, hc, 2, wc, 2).transpose(0, 2, 4, 1, 3).reshape(k * 28, hc, wc)
    return conv.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _convs(dtype_name):
    """Per image of ODD: the conv output on the device and the per-image route's field
    (fields_from_conv of that conv alone), computed once."""
    import torch
    from openpifpaf_amd import heads
    convs, fields = [], []
    for (h, w) in ODD:
        conv = torch.from_numpy(conv_from_det(rd.image('uniform', h, w, 0))).cuda()
        conv = conv.to(getattr(torch, dtype_name))
        convs.append(conv)
        fields.append(heads.fields_from_conv(conv[None], rd.K, 'cifdet', 1)[0])
        assert tuple(fields[-1].shape) == (rd.K, 7, h, w)
    return convs, fields


def test_conv_inverse_is_the_ingest_inverse():
    """conv_from_det against the oracle's ingest: the fields come back (to rounding)."""
    det = rd.image('uniform', 13, 17, 0)
    back = oracle.fields_from_conv(conv_from_det(det)[None], rd.K, 'cifdet', 1)[0]
    assert back.shape == det.shape
    assert np.allclose(back, det, rtol=1e-5, atol=1e-5)


def _metas(n):
    from test_oracle_golden import inverse_metas
    named = inverse_metas()
    return [dict(named[('shift', 'rot')[i % 2]], image_id=40 + i) for i in range(n)]


@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_from_conv(dec, dtype_name):
    """RaggedDetFields.from_conv + decode_ragged / coco_ragged against the per-image route:
    fields_from_conv per image, CifDet.__call__ and the per-image COCO predictions."""
    import coco_util
    from openpifpaf_amd import engine, heads
    convs, fields = _convs(dtype_name)
    cd = _cifdet(dec, 'uniform')
    ragged = engine.RaggedDetFields.from_conv(convs, rd.K, quad=1)
    assert (ragged.n, ragged.k, ragged.h, ragged.w) == (6, rd.K, 23, 29)
    assert ragged.extents_host.tolist() == [list(s) for s in ODD]
    assert ragged.extents.cpu().numpy().tolist() == [list(s) for s in ODD]
    collected = heads.RaggedDetCollector(rd.K, quad=1)((convs,))
    assert isinstance(collected, engine.RaggedDetFields)
    assert collected.det.cpu().numpy().tobytes() == ragged.det.cpu().numpy().tobytes()
    got = cd.decode_ragged(ragged)
    want = [cd([f]) for f in fields]
    print(dtype_name, 'detections per image', [len(a) for a in want])
    assert len(got) == 6 and min(len(a) for a in want) >= 1
    for g, w in zip(got, want):
        assert [a.field_i for a in g] == [a.field_i for a in w]
        for name in ('score', 'bbox'):
            assert np.array([getattr(a, name) for a in g], np.float32).tobytes() == \
                np.array([getattr(a, name) for a in w], np.float32).tobytes()
    # the list of per-image fields takes the pack route to the same records
    listed = cd.decode_ragged([[f] for f in fields])
    assert [[(a.field_i, a.score) for a in g] for g in listed] == \
        [[(a.field_i, a.score) for a in g] for g in got]
    # pack() runs the ingest launch again
    ragged.det.fill_(float('nan'))
    ragged.extents.fill_(-1)
    ragged.pack()
    assert ragged.det.cpu().numpy().tobytes() == collected.det.cpu().numpy().tobytes()
    assert ragged.extents.cpu().numpy().tolist() == [list(s) for s in ODD]
    metas = _metas(6)
    coco = cd.coco_ragged(ragged, metas, max_per_image=5)
    per_image = []
    for f, m in zip(fields, metas):
        per_image += cd.coco_batch(f[None], [m], max_per_image=5).predictions()
    assert len(per_image) >= 6
    assert coco_util.dumps(coco.predictions()) == coco_util.dumps(per_image)


# ---- 6. the capacity retry ----------------------------------------------------------------
def test_capacity_retry(dec):
    cd = _cifdet(dec, 'uniform')
    fields = _device_fields('uniform', TWELVE[:6])
    want = [len(rd.own_decode('uniform', h, w, seed)) for (h, w), seed in TWELVE[:6]]
    assert max(want) > 4  # the first capacity overflows
    recs, offsets = cd.decode_ragged_records(fields, cap=4)
    assert _check_records(recs, offsets, 'uniform', TWELVE[:6]) == want


# ---- 7. more than 4,096 seeds per field ---------------------------------------------------
def test_more_than_4096_seeds_per_field(dec):
    """det_uniform(65, 65, 2, seed 3) at seed threshold 0 has 4,225 seeds in each field: the
    sort runs over 8,192 keys per field in global memory, more than the field's 4,225 cells.
    Through the uniform entry point, and as one image of a 65x67 ragged batch: the oracle's
    720 records (361 + 359).  With `cells` keys per field the sorts of neighbouring fields
    overlapped; that is a race between workgroups, and the one run of this input on the
    earlier layout gave the oracle's records too, so the uniform half pins the result rather
    than the defect (DESIGN.md §4 "Ragged CifDet")."""
    import torch
    cd = _cifdet(dec, 'uniform', k=2, seed_threshold=0.0)
    big, other = ((65, 65), 3), ((65, 67), 4)
    want = rd.own_decode('uniform', 65, 65, 3, 2, 0.0)
    assert len(want) == 720
    assert np.bincount(want['field'], minlength=2).tolist() == [361, 359]
    det = torch.from_numpy(rd.image('uniform', 65, 65, 3, 2).copy()).cuda()
    recs, offsets = cd.decode_records(det[None])
    assert offsets.tolist() == [0, 720]
    rd.assert_same_records(recs, want, 0)
    cases = [other, big]
    recs, offsets = cd.decode_ragged_records(_device_fields('uniform', cases, k=2))
    _check_records(recs, offsets, 'uniform', cases, k=2, seed_threshold=0.0)
    assert offsets[2] - offsets[1] == 720


# ---- 8. Python errors ---------------------------------------------------------------------
def test_python_errors(dec):
    import torch
    from openpifpaf_amd import engine
    cd = _cifdet(dec, 'uniform')
    fields = _device_fields('uniform', TWELVE[:3])
    with pytest.raises(ValueError, match='K'):  # mixed K
        engine.RaggedDetFields([fields[0][0], fields[1][0][:2].contiguous()])
    with pytest.raises(ValueError, match='contiguous float32'):  # a view with a column step
        engine.RaggedDetFields([fields[0][0], fields[1][0][:, :, :, ::2]])
    with pytest.raises(ValueError, match='contiguous float32'):
        engine.RaggedDetFields([fields[0][0].double()])
    with pytest.raises(ValueError, match='7'):  # CIF fields
        engine.RaggedDetFields([fields[0][0][:, :5].contiguous()])
    with pytest.raises(ValueError, match='at least one image'):
        engine.RaggedDetFields([])
    with pytest.raises(NotImplementedError, match='group'):
        cd.decode_ragged(fields, group=object())
    with pytest.raises(NotImplementedError, match='group'):
        cd.coco_ragged(fields, _metas(3), group=object())
    with pytest.raises(TypeError):
        cd.decode_ragged(fields, keep_cifhr=True)
    with pytest.raises(ValueError, match='2 metas for 3 images'):
        cd.coco_ragged(fields, _metas(2))
    two_heads = dec.CifDet(dec.FieldConfig(cif_indices=[0, 1], cif_strides=[8, 16],
                                           cif_min_scales=[0.0, 0.0]), CATS)
    with pytest.raises(NotImplementedError, match='one detection head'):
        two_heads.decode_ragged([f + f for f in fields])
    min_scale = dec.CifDet(dec.FieldConfig(cif_min_scales=[4.0]), CATS)
    with pytest.raises(NotImplementedError, match='min scale'):
        min_scale.decode_ragged(fields)
    torch.cuda.synchronize()
