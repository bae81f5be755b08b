"""pp_fields_from_conv_ragged on the device (heads.fields_from_conv_ragged, RaggedCollector,
engine.RaggedFields.from_conv): the conv outputs of images of different sizes go straight
into the container of a ragged batch.  The expected value of every comparison is the route
that existed before: heads.fields_from_conv on each image's dense clone, zero-padded with
torch into the container's shape.  Every comparison is of bytes."""
import functools

import numpy as np
import pytest

import ragged_util as ru
from test_gpu_ingest_strided import PER, SENTINEL, _bytes, _head, _values

pytestmark = pytest.mark.gpu

# a 1x1 image, one that fills the container's height but not its width (5x5 beside 2x7), the
# reverse (2x7), and sizes inside both
EXTENTS = [(1, 1), (3, 4), (4, 3), (2, 7), (5, 5), (1, 6)]
# quad 1: fields of 23x29 = 667 (neither a multiple of 256 nor of 64), 17x19 = 323 and 1
BOUNDARY = [(12, 15), (9, 10), (1, 1)]
NAN = float('nan')


def _dim(n, quad):
    for _ in range(quad):
        n = 2 * n - 1
    return n


def _padded(convs, n_fields, kind, quad, flip, shape=None):
    """The parent's route: one fields_from_conv per image on its dense clone, zero-padded."""
    import torch
    from openpifpaf_amd import heads
    fields = [heads.fields_from_conv(c.clone(memory_format=torch.contiguous_format)[None],
                                     n_fields, kind, quad, hflip=flip) for c in convs]
    h, w = shape or (max(f.shape[3] for f in fields), max(f.shape[4] for f in fields))
    out = torch.zeros((len(convs), n_fields, PER[kind], h, w), device='cuda')
    for i, f in enumerate(fields):
        out[i, :, :, :f.shape[3], :f.shape[4]] = f[0]
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, dtype_name, flipped, quad, extents=tuple(EXTENTS)):
    """(per-image dense convs, hflip, the padded per-image ingests), computed once and shared
    (read-only) by the tests that need the same inputs."""
    n_fields, flip = _head(kind)
    rng = np.random.default_rng(100 * quad + len(kind) + len(dtype_name) + flipped)
    ch = n_fields * PER[kind] * 4 ** quad
    convs = tuple(_values(rng, dtype_name, (ch, h, w)) for h, w in extents)
    flip = flip if flipped else None
    return convs, n_fields, flip, _padded(convs, n_fields, kind, quad, flip)


def _field_extents(extents, quad):
    return [[_dim(h, quad), _dim(w, quad)] for h, w in extents]


# ---- 1. the grid of small cases -----------------------------------------------------------
@pytest.mark.parametrize('quad', [0, 1, 2])
@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('kind', ['cif', 'caf', 'cifdet'])
def test_grid(kind, dtype_name, flipped, quad):
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case(kind, dtype_name, flipped, quad)
    assert tuple(want.shape[3:]) == (_dim(5, quad), _dim(7, quad))
    out = torch.full(want.shape, NAN, device='cuda')
    got, ext, ext_host = heads.fields_from_conv_ragged(list(convs), n_fields, kind, quad,
                                                       hflip=flip, out=out)
    assert got is out and _bytes(got) == _bytes(want)
    assert ext.dtype == torch.int32 and ext_host.dtype == np.int32
    assert ext.cpu().numpy().tolist() == ext_host.tolist() == _field_extents(EXTENTS, quad)
    # a container of the call's own, and (1, ch, h, w) inputs
    got, _, _ = heads.fields_from_conv_ragged([c[None] for c in convs], n_fields, kind, quad,
                                              hflip=flip)
    assert got.shape == want.shape and _bytes(got) == _bytes(want)


# ---- 2. workgroup and wave boundaries -----------------------------------------------------
@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_workgroup_and_wave_boundaries(dtype_name, flipped):
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case('caf', dtype_name, flipped, 1, tuple(BOUNDARY))
    assert want.shape == (3, 19, 9, 23, 29)
    out = torch.full(want.shape, NAN, device='cuda')
    heads.fields_from_conv_ragged(list(convs), n_fields, 'caf', 1, hflip=flip, out=out)
    assert _bytes(out) == _bytes(want)


# ---- 3. a larger container, and one 4 bytes off a 16-byte boundary ---------------------------
@pytest.mark.parametrize('flipped', [False, True])
def test_container_larger_than_every_image(flipped):
    from openpifpaf_amd import heads
    convs, n_fields, flip, _ = _case('cif', 'float32', flipped, 1)
    want = _padded(convs, n_fields, 'cif', 1, flip, shape=(9 + 2, 13 + 3))
    got, ext, _ = heads.fields_from_conv_ragged(list(convs), n_fields, 'cif', 1, hflip=flip,
                                                shape=(11, 16))
    assert got.shape == want.shape == (6, 17, 5, 11, 16)
    assert _bytes(got) == _bytes(want)
    assert ext.cpu().numpy().tolist() == _field_extents(EXTENTS, 1)


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_container_off_a_16_byte_boundary(dtype_name):
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case('caf', dtype_name, True, 1)
    assert want.shape[4] == 13  # W odd: the planes start at every 4-byte phase
    flat = torch.full((1 + want.numel() + 3,), SENTINEL, device='cuda')
    out = flat[1:1 + want.numel()].view(want.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    got, _, _ = heads.fields_from_conv_ragged(list(convs), n_fields, 'caf', 1, hflip=flip,
                                              out=out)
    assert got is out and _bytes(out) == _bytes(want)
    assert flat[0].item() == SENTINEL and (flat[1 + want.numel():] == SENTINEL).all()


# ---- 4. the batched form ------------------------------------------------------------------
def _batched(convs, channels0=0, channels=None):
    """(n, channels, hmax, wmax) full of NaN with image i in [c0, c0 + ch) x [0, h_i) x
    [0, w_i)."""
    import torch
    ch = convs[0].shape[0]
    hmax, wmax = max(c.shape[1] for c in convs), max(c.shape[2] for c in convs)
    big = torch.full((len(convs), channels or ch, hmax, wmax), NAN, dtype=convs[0].dtype,
                     device='cuda')
    for i, c in enumerate(convs):
        big[i, channels0:channels0 + ch, :c.shape[1], :c.shape[2]] = c
    return big


@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
@pytest.mark.parametrize('kind', ['cif', 'caf'])
def test_batched_tensor_with_extents(kind, dtype_name, flipped):
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case(kind, dtype_name, flipped, 1)
    ch = convs[0].shape[0]
    big = _batched(convs)
    assert big.shape == (6, ch, 5, 7) and big.isnan().any()
    for extents in (EXTENTS, np.array(EXTENTS), torch.tensor(EXTENTS)):
        out = torch.full(want.shape, NAN, device='cuda')
        got, ext, _ = heads.fields_from_conv_ragged(big, n_fields, kind, 1, hflip=flip,
                                                    conv_extents=extents, out=out)
        assert _bytes(got) == _bytes(want) and not got.isnan().any()
        assert ext.cpu().numpy().tolist() == _field_extents(EXTENTS, 1)
    # a channel slice of a fused tensor: other channel and image strides than the dense ones
    fused = _batched(convs, channels0=3, channels=1024)
    view = fused[:, 3:3 + ch]
    assert view.stride() == (1024 * 35, 35, 7, 1) and not view.is_contiguous()
    got, _, _ = heads.fields_from_conv_ragged(view, n_fields, kind, 1, hflip=flip,
                                              conv_extents=EXTENTS)
    assert _bytes(got) == _bytes(want) and not got.isnan().any()


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_row_sliced_views(dtype_name):
    """A list whose tensors are spatial crops of larger ones: row stride > w_i."""
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case('caf', dtype_name, True, 1)
    views = []
    for c in convs:
        ch, h, w = c.shape
        big = torch.full((ch, h + 2, w + 3), NAN, dtype=c.dtype, device='cuda')
        big[:, 1:1 + h, 2:2 + w] = c
        views.append(big[:, 1:1 + h, 2:2 + w])
        assert views[-1].stride() == ((h + 2) * (w + 3), w + 3, 1)
    got, _, _ = heads.fields_from_conv_ragged(views, n_fields, 'caf', 1, hflip=flip)
    assert _bytes(got) == _bytes(want) and not got.isnan().any()
    # columns not adjacent: that image is copied, the result is the same
    views[3] = convs[3].permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert views[3].stride(2) != 1
    got, _, _ = heads.fields_from_conv_ragged(views, n_fields, 'caf', 1, hflip=flip)
    assert _bytes(got) == _bytes(want)


# ---- 5. a field range ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _caf_and_dense(flipped):
    import torch
    rng = np.random.default_rng(29 + flipped)
    parts = []
    for kind in ('caf', 'dense'):
        n_fields, flip = _head(kind)
        convs = tuple(_values(rng, 'float32', (n_fields * 9 * 4, h, w)) for h, w in EXTENTS)
        flip = flip if flipped else None
        parts.append((convs, n_fields, flip, _padded(convs, n_fields, 'caf', 1, flip)))
    return parts, torch.cat([parts[0][3], parts[1][3]], dim=1)


@pytest.mark.parametrize('flipped', [False, True])
def test_field_range(flipped):
    import torch
    from openpifpaf_amd import heads
    ((caf, _, caf_flip, caf_want), (dense, _, dense_flip, _)), want = _caf_and_dense(flipped)
    assert want.shape == (6, 44, 9, 9, 13)
    out = torch.full(want.shape, SENTINEL, device='cuda')
    res, _, _ = heads.fields_from_conv_ragged(list(caf), 19, 'caf', 1, hflip=caf_flip, out=out)
    assert res is out
    assert (out[:, 19:] == SENTINEL).all()  # zero region included
    assert _bytes(out[:, :19].contiguous()) == _bytes(caf_want)
    heads.fields_from_conv_ragged(list(dense), 25, 'caf', 1, hflip=dense_flip, out=out,
                                  out_field0=19)
    assert _bytes(out) == _bytes(want)


# ---- 6. end to end ------------------------------------------------------------------------
SIX = [(s, 0) for s in ru.SHAPES]
# output channel -> concatenated channel (conf, vectors, logb, scales) of the two heads
PERM = {'cif': (0, 1, 2, 3, 4), 'caf': (0, 1, 2, 5, 7, 3, 4, 6, 8)}


def conv_from_fields(field, kind):
    """The inverse of the head's tail at quad 0: decoder fields (n_fields, 5 | 9, h, w) -> the
    conv output (channels, h, w) grouped as conf, vectors, logb, scales.  float64, rounded."""
    f = np.asarray(field, np.float64)
    n_fields, n_out, h, w = f.shape
    nv = 1 if kind == 'cif' else 2
    cat = np.empty_like(f)
    cat[:, list(PERM[kind])] = f
    conf = np.clip(cat[:, :1], 1e-6, 1 - 1e-6)
    conf = np.log(conf / (1 - conf))
    yy, xx = np.indices((h, w), dtype=np.float64)
    vec = cat[:, 1:1 + 2 * nv].copy()
    vec[:, 0::2] -= xx
    vec[:, 1::2] -= yy
    logb = cat[:, 1 + 2 * nv:1 + 3 * nv]
    scales = np.log(np.maximum(cat[:, 1 + 3 * nv:], 1e-6))
    groups = [g.reshape(-1, h, w) for g in (conf, vec, logb, scales)]
    return np.concatenate(groups).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _planted():
    """Per image of ru.SHAPES: (cif conv, caf conv) on the device and the parent route's
    fields (cif (17, 5, h, w), caf (19, 9, h, w)) on the device."""
    import torch
    from openpifpaf_amd import heads
    convs, fields = [], []
    for (h, w), seed in SIX:
        cif, caf = ru.image('planted', h, w, seed)
        pair = (torch.from_numpy(conv_from_fields(cif, 'cif')).cuda(),
                torch.from_numpy(conv_from_fields(caf, 'caf')).cuda())
        convs.append(pair)
        fields.append((heads.fields_from_conv(pair[0][None], 17, 'cif', 0)[0],
                       heads.fields_from_conv(pair[1][None], 19, 'caf', 0)[0]))
    return convs, fields


DEFAULTS = {
    'eval': dict(seed=0.2, force_complete=True, keypoint=0.0, nms_keypoint=0.0, instance=0.0),
    'predict': dict(seed=0.5, force_complete=False, keypoint=0.001, nms_keypoint=0.001,
                    instance=0.1),
}


@pytest.fixture(params=['eval', 'predict'])
def cifcaf(request):
    from openpifpaf_amd import constants, decoder as dec
    d = DEFAULTS[request.param]
    wanted = [(dec.CifHr, 'v_threshold', 0.1), (dec.CafScored, 'default_score_th', 0.1),
              (dec.CifSeeds, 'threshold', d['seed']),
              (dec.CifCaf, 'force_complete', d['force_complete']),
              (dec.CifCaf, 'keypoint_threshold', d['keypoint']), (dec.CifCaf, 'greedy', False),
              (dec.CifCaf, 'connection_method', 'blend'),
              (dec.nms.Keypoints, 'instance_threshold', d['instance']),
              (dec.nms.Keypoints, 'keypoint_threshold', d['nms_keypoint'])]
    before = [(obj, name, getattr(obj, name)) for obj, name, _ in wanted]
    for obj, name, value in wanted:
        setattr(obj, name, value)
    decoder = dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                         skeleton=constants.COCO_PERSON_SKELETON)
    decoder.mode = request.param
    yield decoder
    for obj, name, value in before:
        setattr(obj, name, value)


def _same_annotations(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.data.tobytes() == b.data.tobytes()
        assert a.joint_scales.tobytes() == b.joint_scales.tobytes()
        assert len(a.decoding_order) == len(b.decoding_order)
        for x, y in zip(a.decoding_order, b.decoding_order):
            assert x[:2] == y[:2] and x[2].tobytes() == y[2].tobytes()
            assert x[3].tobytes() == y[3].tobytes()
        assert a.frontier_order == b.frontier_order


def test_decode_ragged_from_conv(cifcaf):
    """Eval and predict defaults: CifCaf.decode_ragged of RaggedFields.from_conv equals
    decode_ragged of the per-image fields_from_conv list, and the host twin on those fields.
    (On the host, this recipe gives 5, 3, 5, 5, 4, 3 annotations per image in eval defaults
    and 5, 2, 5, 5, 3, 3 in predict defaults.)"""
    from openpifpaf_amd import engine, stages_cpu
    convs, fields = _planted()
    ragged = engine.RaggedFields.from_conv([c[0] for c in convs], [c[1] for c in convs], 17, 19,
                                           quad=0)
    assert (ragged.n, ragged.k, ragged.c, ragged.h, ragged.w) == (6, 17, 19) + ru.CONTAINER
    assert ragged.extents_host.tolist() == [list(s) for s in ru.SHAPES]
    assert ragged.extents.cpu().numpy().tolist() == [list(s) for s in ru.SHAPES]
    got = cifcaf.decode_ragged(ragged)
    want = cifcaf.decode_ragged([list(f) for f in fields])
    print(cifcaf.mode, 'annotations per image', [len(a) for a in got])
    assert len(got) == len(want) == 6 and sum(len(a) for a in got) >= 1
    for g, w in zip(got, want):
        _same_annotations(g, w)
    # full records against the host twin on the parent route's fields
    cfg = ru.config(cifcaf.mode)
    recs, offsets, _ = engine.DecodeEngine().decode(None, None, ru.SKELETONS['coco'], cfg,
                                                    ragged=ragged)
    twin, twin_off = stages_cpu.decode_ragged([f[0].cpu().numpy() for f in fields],
                                              [f[1].cpu().numpy() for f in fields],
                                              ru.SKELETONS['coco'], cfg)
    assert np.array(offsets).tolist() == np.array(twin_off).tolist()
    assert [len(a) for a in got] == np.diff(twin_off).tolist()
    for i in range(6):
        ru.assert_same_records(recs[offsets[i]:offsets[i + 1]],
                               twin[twin_off[i]:twin_off[i + 1]], i)
    for kw in ({'initial_annotations': [object()]}, {'group': object()}, {'keep_cifhr': True}):
        with pytest.raises(NotImplementedError):
            cifcaf.decode_ragged(ragged, **kw)


def test_coco_ragged_from_conv(cifcaf):
    from test_oracle_golden import inverse_metas
    from openpifpaf_amd import engine
    convs, fields = _planted()
    named = inverse_metas()
    metas = [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=70 + i) for i in range(6)]
    ragged = engine.RaggedFields.from_conv([c[0] for c in convs], [c[1] for c in convs], 17, 19,
                                           quad=0)
    got = cifcaf.coco_ragged(ragged, metas, max_per_image=5)
    want = cifcaf.coco_ragged([list(f) for f in fields], metas, max_per_image=5)
    assert got.offsets.tolist() == want.offsets.tolist() and got.offsets[-1] >= 1
    assert got.flags.tolist() == want.flags.tolist()
    assert got.records.tobytes() == want.records.tobytes()


# ---- 7. RaggedCollector and caf_parts -----------------------------------------------------
def test_ragged_collector_and_repack():
    from openpifpaf_amd import engine, heads
    convs, fields = _planted()
    cifs, cafs = [c[0] for c in convs], [c[1] for c in convs]
    want = engine.RaggedFields([tuple(f) for f in fields])
    direct = engine.RaggedFields.from_conv(cifs, cafs, 17, 19, quad=0)
    collected = heads.RaggedCollector(17, 19, quad=0)((cifs, cafs))
    assert isinstance(collected, engine.RaggedFields)
    for r in (direct, collected):
        assert _bytes(r.cif) == _bytes(want.cif) and _bytes(r.caf) == _bytes(want.caf)
        assert r.extents.cpu().numpy().tolist() == want.extents_host.tolist()
        assert r.extents_host.tolist() == want.extents_host.tolist()
    # pack() runs the two ingest launches again
    direct.cif.fill_(NAN)
    direct.caf.fill_(NAN)
    direct.extents.fill_(-1)
    direct.pack()
    assert _bytes(direct.cif) == _bytes(want.cif) and _bytes(direct.caf) == _bytes(want.caf)
    assert direct.extents.cpu().numpy().tolist() == want.extents_host.tolist()


@pytest.mark.parametrize('flipped', [False, True])
def test_caf_parts(flipped):
    from openpifpaf_amd import engine
    ((caf, _, caf_flip, _), (dense, _, dense_flip, _)), want = _caf_and_dense(flipped)
    n_cif, cif_flip = _head('cif')
    cif, _, _, cif_want = _case('cif', 'float32', flipped, 1)
    ragged = engine.RaggedFields.from_conv(
        list(cif), None, n_cif, None, quad=1, cif_hflip=cif_flip if flipped else None,
        caf_parts=[(list(caf), 19, caf_flip), (list(dense), 25, dense_flip)])
    assert (ragged.k, ragged.c, ragged.h, ragged.w) == (17, 44, 9, 13)
    assert _bytes(ragged.caf) == _bytes(want) and _bytes(ragged.cif) == _bytes(cif_want)


# ---- 8. Python errors ---------------------------------------------------------------------
def test_python_errors():
    import torch
    from openpifpaf_amd import engine, heads
    cif, _, _, _ = _case('cif', 'float32', False, 1)
    caf, _, _, _ = _case('caf', 'float32', False, 1)
    cif, caf = list(cif), list(caf)
    sentinel = torch.full((6, 17, 5, 9, 13), SENTINEL, device='cuda')
    with pytest.raises(ValueError):  # lists of different lengths
        engine.RaggedFields.from_conv(cif, caf[:5], 17, 19)
    with pytest.raises(ValueError):  # CIF and CAF extents that differ
        engine.RaggedFields.from_conv(cif, caf[:4] + [caf[5], caf[4]], 17, 19)
    big = _batched(cif)
    for rows in ([(1, 1), (3, 4), (4, 3), (2, 8), (5, 5), (1, 6)],
                 [(1, 1), (3, 4), (4, 3), (2, 7), (6, 5), (1, 6)],
                 [(1, 1), (3, 4), (4, 3), (2, 7), (0, 5), (1, 6)], EXTENTS[:5]):
        with pytest.raises(ValueError):  # a conv_extents row beyond the batched tensor
            heads.fields_from_conv_ragged(big, 17, 'cif', conv_extents=rows, out=sentinel)
    with pytest.raises(ValueError):  # conv_extents with a list input
        heads.fields_from_conv_ragged(cif, 17, 'cif', conv_extents=EXTENTS, out=sentinel)
    with pytest.raises(ValueError):  # a channel count that does not match n_fields
        heads.fields_from_conv_ragged(cif, 16, 'cif', out=sentinel[:, :16].contiguous())
    with pytest.raises(ValueError):
        heads.fields_from_conv_ragged(cif, 17, 'cif', quad=0)
    for shape in ((8, 13), (9, 12)):
        with pytest.raises(ValueError):  # shape smaller than an image
            heads.fields_from_conv_ragged(cif, 17, 'cif', shape=shape)
    with pytest.raises(ValueError):  # an `out` of another shape
        heads.fields_from_conv_ragged(cif, 17, 'cif', out=sentinel[:, :, :, :8].contiguous())
    with pytest.raises(ValueError):
        heads.fields_from_conv_ragged([], 17, 'cif')
    torch.cuda.synchronize()
    assert (sentinel == SENTINEL).all()  # nothing was launched
