"""pp_fields_from_conv_ragged_heads on the device (heads.RaggedHeadsIngest,
engine.RaggedHeadSet.from_conv, heads.RaggedMultiScaleCollector): the conv outputs of every
head of every image of a ragged multi-scale batch go into the containers in one launch.  The
expected value of every comparison comes from routes that existed before:
heads.fields_from_conv_ragged per entry into a NaN-filled container, and
engine.RaggedHeadSet over per-image heads.fields_from_conv.  Every comparison is of bytes."""
import functools

import numpy as np
import pytest

import ragged_multi_util as rmu
from test_gpu_ingest_ragged import DEFAULTS, EXTENTS, NAN, _dim, conv_from_fields
from test_gpu_ingest_strided import PER, SENTINEL, _bytes, _head, _values

pytestmark = pytest.mark.gpu

SIX = [(p, 0) for p in rmu.PIXELS]


def _rotated(m):
    """EXTENTS in another order per entry: no two heads share a container size pattern."""
    return tuple(EXTENTS[i] for i in np.random.default_rng(40 + m).permutation(len(EXTENTS)))


def _field_config(n_scales):
    from openpifpaf_amd import decoder
    return decoder.FieldConfig(
        cif_indices=[2 * i for i in range(n_scales)],
        caf_indices=[2 * i + 1 for i in range(n_scales)],
        cif_strides=[8 * (1 + i % 2) for i in range(n_scales)],
        caf_strides=[8 * (1 + i % 2) for i in range(n_scales)],
        cif_min_scales=[0.0] * n_scales, caf_min_distances=[0.0] * n_scales,
        caf_max_distances=[None] * n_scales)


def _want(convs, n_fields, kind, quad, flip, shape=None, out=None, out_field0=0, **kw):
    """The parent's route for one entry: pp_fields_from_conv_ragged into a NaN-filled container."""
    import torch
    from openpifpaf_amd import heads
    if out is None:
        h = max(_dim(c.shape[-2], quad) for c in convs)
        w = max(_dim(c.shape[-1], quad) for c in convs)
        out = torch.full((len(convs), n_fields, PER[kind]) + (shape or (h, w)), NAN, device='cuda')
    heads.fields_from_conv_ragged(convs, n_fields, kind, quad, hflip=flip, out=out,
                                  out_field0=out_field0, **kw)
    return out


@functools.lru_cache(maxsize=None)
def _entries(n_entries, dtype_name, quad):
    """Per entry (kind, n_fields, hflip or None, per-image convs, the entry's container by the
    parent's route): scales x (CIF, CAF), the second half of eight mirrored.  Shared, read-only."""
    rng = np.random.default_rng(1000 * n_entries + 10 * quad + len(dtype_name))
    out = []
    for m in range(n_entries):
        kind = 'caf' if m % 2 else 'cif'
        n_fields, flip = _head(kind)
        flip = flip if n_entries == 8 and m >= 4 else None
        convs = tuple(_values(rng, dtype_name, (n_fields * PER[kind] * 4 ** quad, h, w))
                      for h, w in _rotated(m))
        out.append((kind, n_fields, flip, convs, _want(list(convs), n_fields, kind, quad, flip)))
    return tuple(out)


def _parts(entries):
    return [(list(convs), n_fields, kind, flip, m)
            for m, (kind, n_fields, flip, convs, _) in enumerate(entries)]


def _nan_like(entries):
    import torch
    return {m: torch.full(e[4].shape, NAN, device='cuda') for m, e in enumerate(entries)}


# ---- 1. the grid ---------------------------------------------------------------------------
@pytest.mark.parametrize('quad', [0, 1, 2])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('n_entries', [4, 8])
def test_grid(n_entries, dtype_name, quad):
    import torch
    from openpifpaf_amd import engine, heads
    entries = _entries(n_entries, dtype_name, quad)
    assert len({tuple(c.shape[1:] for c in e[3]) for e in entries}) == n_entries
    outs = _nan_like(entries)
    ing = heads.RaggedHeadsIngest(_parts(entries), quad, outs=outs)
    assert all(o.isnan().all() for o in outs.values())  # nothing runs before launch()
    ing.launch()
    for m, e in enumerate(entries):
        assert ing.outs[m] is outs[m] and _bytes(outs[m]) == _bytes(e[4]), m
        assert not outs[m].isnan().any()
    want_ext = [[[_dim(h, quad), _dim(w, quad)] for h, w in _rotated(m)]
                for m in range(n_entries)]
    assert ing.extents.dtype == torch.int32 and ing.extents_host.dtype == np.int32
    assert ing.extents.shape == (n_entries, 6, 2)
    assert ing.extents.cpu().numpy().tolist() == ing.extents_host.tolist() == want_ext
    # the head set, with containers of its own, and (1, ch, h, w) inputs
    order = list(range(0, n_entries, 2)) + list(range(1, n_entries, 2))  # CIF heads first
    items = [([c[None] for c in e[3]], e[2]) if e[2] is not None else [c[None] for c in e[3]]
             for e in entries]
    for one_launch in (False, True):
        rhs = engine.RaggedHeadSet.from_conv(items, _field_config(n_entries // 2), quad=quad,
                                             one_launch=one_launch)
        assert (rhs.n, rhs.k, rhs.c) == (6, 17, 19)
        for t, m in zip(rhs.cifs + rhs.cafs, order):
            assert t.shape == entries[m][4].shape and _bytes(t) == _bytes(entries[m][4]), m
        assert rhs.extents.dtype == torch.int32 and rhs.extents.shape == (n_entries, 6, 2)
        assert rhs.extents.cpu().numpy().tolist() == rhs.extents_host.tolist() == \
            [want_ext[m] for m in order]
        assert (rhs.h, rhs.w) == tuple(rhs.cifs[0].shape[3:]) and rhs.stride0 == 8
        assert rhs.pairs == 0 and len(rhs.arr) == n_entries
        assert [(s.H, s.W) for s in rhs.arr] == [tuple(entries[m][4].shape[3:]) for m in order]
        assert [s.cif or s.caf for s in rhs.arr] == [t.data_ptr() for t in rhs.cifs + rhs.cafs]
        assert rhs.shape_key[:2] == ('ragged', 0) and len(rhs.shape_key) == 2 + n_entries


# ---- 2. workgroup and prefix boundaries ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary(flipped):
    """Containers of 23x29 = 667, 1 and 17x19 = 323 pixels: 3, 1 and 2 workgroups per plane,
    the single workgroup between the two others in the prefix table."""
    rng = np.random.default_rng(77 + flipped)
    out = []
    for kind, extents in (('caf', [(12, 15), (9, 10), (1, 1)]), ('cif', [(1, 1)] * 3),
                          ('caf', [(9, 10), (1, 1), (5, 5)])):
        n_fields, flip = _head(kind)
        flip = flip if flipped else None
        convs = tuple(_values(rng, 'float32', (n_fields * PER[kind] * 4, h, w))
                      for h, w in extents)
        out.append((kind, n_fields, flip, convs, _want(list(convs), n_fields, kind, 1, flip)))
    return tuple(out)


@pytest.mark.parametrize('flipped', [False, True])
def test_workgroup_and_prefix_boundaries(flipped):
    from openpifpaf_amd import heads
    entries = _boundary(flipped)
    assert [tuple(e[4].shape[3:]) for e in entries] == [(23, 29), (1, 1), (17, 19)]
    outs = _nan_like(entries)
    ing = heads.RaggedHeadsIngest(_parts(entries), 1, outs=outs).launch()
    for m, e in enumerate(entries):
        assert _bytes(outs[m]) == _bytes(e[4]), m
    assert ing.extents.cpu().numpy().tolist() == ing.extents_host.tolist()
    assert ing.extents_host[:, 0].tolist() == [[23, 29], [1, 1], [17, 19]]


# ---- 3. a larger container, and one 4 bytes off a 16-byte boundary ---------------------------
@pytest.mark.parametrize('flipped', [False, True])
def test_container_larger_than_every_image(flipped):
    import torch
    from openpifpaf_amd import heads
    entries = _boundary(flipped)
    shapes = [(25, 32), (2, 3), (17, 20)]
    want = [_want(list(e[3]), e[1], e[0], 1, e[2], shape=s) for e, s in zip(entries, shapes)]
    outs = {m: torch.full(w.shape, NAN, device='cuda') for m, w in enumerate(want)}
    ing = heads.RaggedHeadsIngest(_parts(entries), 1, outs=outs).launch()
    for m, w in enumerate(want):
        assert tuple(outs[m].shape[3:]) == shapes[m] and _bytes(outs[m]) == _bytes(w), m
    assert ing.extents_host[:, 0].tolist() == [[23, 29], [1, 1], [17, 19]]
    assert ing.extents.cpu().numpy().tolist() == ing.extents_host.tolist()


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_container_off_a_16_byte_boundary(dtype_name):
    import torch
    from openpifpaf_amd import heads
    entries = _entries(8, dtype_name, 1)
    outs, flats = {}, []
    for m, e in enumerate(entries):
        numel = e[4].numel()
        flat = torch.full((1 + numel + 3,), SENTINEL, device='cuda')
        outs[m] = flat[1:1 + numel].view(e[4].shape)
        assert outs[m].data_ptr() % 16 == 4 and outs[m].is_contiguous()
        flats.append(flat)
    heads.RaggedHeadsIngest(_parts(entries), 1, outs=outs).launch()
    for m, e in enumerate(entries):
        assert _bytes(outs[m]) == _bytes(e[4]), m
        assert flats[m][0].item() == SENTINEL and (flats[m][1 + e[4].numel():] == SENTINEL).all()


# ---- 4. parts -----------------------------------------------------------------------------
@pytest.mark.parametrize('flipped', [False, True])
def test_parts_side_by_side(flipped):
    """CAF and dense CAF into fields 2 .. 45 of a container of 48: the neighbours stay."""
    import torch
    from openpifpaf_amd import heads
    rng = np.random.default_rng(31 + flipped)
    cif_fields, cif_flip = _head('cif')
    cif = [_values(rng, 'float32', (cif_fields * 5 * 4, h, w)) for h, w in _rotated(1)]
    parts = [(cif, None, 'cif', cif_flip if flipped else None, 'cif')]
    want = torch.full((6, 48, 9, 9, 13), SENTINEL, device='cuda')
    field0 = 2
    for kind in ('caf', 'dense'):
        n_fields, flip = _head(kind)
        flip = flip if flipped else None
        convs = [_values(rng, 'float32', (n_fields * 9 * 4, h, w)) for h, w in EXTENTS]
        _want(convs, n_fields, 'caf', 1, flip, out=want, out_field0=field0)
        parts.append((convs, n_fields, 'caf', flip, 'caf'))
        field0 += n_fields
    assert field0 == 46
    out = torch.full(want.shape, SENTINEL, device='cuda')
    ing = heads.RaggedHeadsIngest(parts, 1, outs={'caf': out}, field0={'caf': 2}).launch()
    assert ing.outs[1] is out and _bytes(out) == _bytes(want)
    assert (out[:, :2] == SENTINEL).all() and (out[:, 46:] == SENTINEL).all()
    assert not (out[:, 2:46] == SENTINEL).any()
    assert _bytes(ing.outs[0]) == _bytes(_want(cif, cif_fields, 'cif', 1,
                                               cif_flip if flipped else None))
    assert ing.extents.shape == (2, 6, 2)  # one row per container, not per part
    assert ing.extents.cpu().numpy().tolist() == ing.extents_host.tolist()


# ---- 5. views -----------------------------------------------------------------------------
def _same_extent_entries(dtype_name, flipped):
    """Four entries (two scales x CIF, CAF) whose images all have EXTENTS."""
    rng = np.random.default_rng(len(dtype_name) + flipped)
    out = []
    for m in range(4):
        kind = 'caf' if m % 2 else 'cif'
        n_fields, flip = _head(kind)
        flip = flip if flipped and m >= 2 else None
        convs = [_values(rng, dtype_name, (n_fields * PER[kind] * 4, h, w)) for h, w in EXTENTS]
        out.append((kind, n_fields, flip, convs, _want(convs, n_fields, kind, 1, flip)))
    return out


def _check_head_set(rhs, entries):
    for t, m in zip(rhs.cifs + rhs.cafs, (0, 2, 1, 3)):
        assert _bytes(t) == _bytes(entries[m][4]), m
        assert not t.isnan().any()


def _items(entries, convs_of):
    return [(convs_of(m), e[2]) for m, e in enumerate(entries)]


def _both_routes(items, fc, **kw):
    """from_conv by its default route (a call per head) and by the one launch."""
    from openpifpaf_amd import engine
    return [engine.RaggedHeadSet.from_conv(items, fc, one_launch=one, **kw)
            for one in (False, True)]


@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_channel_slices_of_one_fused_tensor(dtype_name, flipped):
    import torch
    from openpifpaf_amd import engine
    entries = _same_extent_entries(dtype_name, flipped)
    chans = [e[3][0].shape[0] for e in entries]
    starts = [3 + sum(chans[:m]) + 5 * m for m in range(4)]
    fused = torch.full((6, starts[-1] + chans[-1] + 7, 5, 7), NAN, dtype=entries[0][3][0].dtype,
                       device='cuda')
    for e, c0 in zip(entries, starts):
        for i, c in enumerate(e[3]):
            fused[i, c0:c0 + c.shape[0], :c.shape[1], :c.shape[2]] = c
    views = [fused[:, c0:c0 + ch] for c0, ch in zip(starts, chans)]
    assert all(not v.is_contiguous() and v.stride(3) == 1 for v in views)
    for extents in (EXTENTS, np.array(EXTENTS), torch.tensor(EXTENTS)):
        for rhs in _both_routes(_items(entries, lambda m: views[m]), _field_config(2),
                                conv_extents=extents):
            _check_head_set(rhs, entries)
            assert rhs.extents_host.tolist() == \
                [[[_dim(h, 1), _dim(w, 1)] for h, w in EXTENTS]] * 4
            assert rhs.extents.cpu().numpy().tolist() == rhs.extents_host.tolist()


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_row_sliced_and_channels_last_views(dtype_name):
    import torch
    from openpifpaf_amd import engine
    entries = _same_extent_entries(dtype_name, True)

    def cropped(m):
        views = []
        for c in entries[m][3]:
            ch, h, w = c.shape
            big = torch.full((ch, h + 2, w + 3), NAN, dtype=c.dtype, device='cuda')
            big[:, 1:1 + h, 2:2 + w] = c
            views.append(big[:, 1:1 + h, 2:2 + w])
            assert views[-1].stride() == ((h + 2) * (w + 3), w + 3, 1)
        return views

    def channels_last(m):
        views = [c.permute(1, 2, 0).contiguous().permute(2, 0, 1) for c in entries[m][3]]
        assert views[4].stride(2) != 1 and views[4].stride(0) == 1
        return views

    fc = _field_config(2)
    for rhs in _both_routes(_items(entries, cropped), fc):
        _check_head_set(rhs, entries)
    # channels-last inputs (copied for the one launch, read in place by the calls per head)
    # give the same bytes: every head, and one image of one head among NCHW ones
    for rhs in _both_routes(_items(entries, channels_last), fc):
        _check_head_set(rhs, entries)
    mixed = _items(entries, lambda m: list(entries[m][3]))
    mixed[1][0][3] = channels_last(1)[3]
    for rhs in _both_routes(mixed, fc):
        _check_head_set(rhs, entries)
    # ... and as one batched channels-last tensor with conv_extents
    e = entries[1]
    big = torch.full((6, e[3][0].shape[0], 5, 7), NAN, dtype=e[3][0].dtype, device='cuda')
    for i, c in enumerate(e[3]):
        big[i, :, :c.shape[1], :c.shape[2]] = c
    nhwc = big.contiguous(memory_format=torch.channels_last)
    assert nhwc.stride(1) == 1
    from openpifpaf_amd import heads
    ing = heads.RaggedHeadsIngest([(nhwc, e[1], e[0], e[2], 0)], 1, conv_extents=EXTENTS).launch()
    assert _bytes(ing.outs[0]) == _bytes(e[4])


# ---- 6. pack() again ----------------------------------------------------------------------
@pytest.mark.parametrize('one_launch', [False, True])
def test_pack_again_after_the_convs_were_rewritten(one_launch):
    from openpifpaf_amd import engine
    entries = _same_extent_entries('float32', True)
    convs = [[c.clone() for c in e[3]] for e in entries]
    rhs = engine.RaggedHeadSet.from_conv(_items(entries, lambda m: convs[m]), _field_config(2),
                                         one_launch=one_launch)
    _check_head_set(rhs, entries)
    rng = np.random.default_rng(5)
    for row in convs:
        for c in row:
            c.copy_(_values(rng, 'float32', tuple(c.shape)))
    want = [_want(convs[m], e[1], e[0], 1, e[2]) for m, e in enumerate(entries)]
    assert _bytes(want[0]) != _bytes(entries[0][4])
    for t in rhs.cifs + rhs.cafs:
        t.fill_(NAN)
    rhs.extents.fill_(-1)
    rhs.pack()
    for t, m in zip(rhs.cifs + rhs.cafs, (0, 2, 1, 3)):
        assert _bytes(t) == _bytes(want[m]), m
    assert rhs.extents.cpu().numpy().tolist() == rhs.extents_host.tolist()


# ---- 7. end to end ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted(name):
    """Per head of the case's head list the per-image conv outputs (quad 0) of the planted
    fields, on the device."""
    import torch
    images = rmu.images(name, SIX)
    n_heads = len(images[0])
    return tuple(tuple(torch.from_numpy(conv_from_fields(img[j], 'caf' if j % 2 else 'cif')).cuda()
                       for img in images) for j in range(n_heads))


def _flips(name, half):
    """Per head None, or with `half` the un-flip tables for every second scale."""
    n_heads = len(rmu.image(name, *SIX[0][0], 0))
    return [(_head('caf' if j % 2 else 'cif')[1] if half and (j // 2) % 2 else None)
            for j in range(n_heads)]


def _parent_fields(name, flips):
    """The parent's route: one fields_from_conv per image per head."""
    from openpifpaf_amd import heads
    convs = _planted(name)
    return [[heads.fields_from_conv(convs[j][i][None], 19 if j % 2 else 17,
                                    'caf' if j % 2 else 'cif', 0, hflip=flips[j])[0]
             for j in range(len(convs))] for i in range(len(SIX))]


@pytest.fixture(params=[(name, mode, False) for name in rmu.PLANTED for mode in rmu.MODES] +
                [('ms10', 'eval', True)], ids=lambda p: '-'.join(str(v) for v in p))
def cifcaf(request):
    from openpifpaf_amd import constants, decoder as dec
    name, mode, half = request.param
    d = DEFAULTS[mode]
    wanted = [(dec.CifHr, 'v_threshold', 0.1), (dec.CafScored, 'default_score_th', 0.1),
              (dec.CifSeeds, 'threshold', d['seed']),
              (dec.CifCaf, 'force_complete', d['force_complete']),
              (dec.CifCaf, 'keypoint_threshold', d['keypoint']), (dec.CifCaf, 'greedy', False),
              (dec.CifCaf, 'connection_method', 'blend'),
              (dec.nms.Keypoints, 'instance_threshold', d['instance']),
              (dec.nms.Keypoints, 'keypoint_threshold', d['nms_keypoint'])]
    before = [(obj, attr, getattr(obj, attr)) for obj, attr, _ in wanted]
    for obj, attr, value in wanted:
        setattr(obj, attr, value)
    decoder = dec.CifCaf(dec.FieldConfig(**rmu.field_config_kwargs(name)),
                         keypoints=constants.COCO_KEYPOINTS,
                         skeleton=constants.COCO_PERSON_SKELETON)
    decoder.case, decoder.half = name, half
    yield decoder
    for obj, attr, value in before:
        setattr(obj, attr, value)


def _from_conv(decoder, one_launch):
    from openpifpaf_amd import engine
    convs, flips = _planted(decoder.case), _flips(decoder.case, decoder.half)
    items = [list(c) if f is None else (list(c), f) for c, f in zip(convs, flips)]
    return engine.RaggedHeadSet.from_conv(items, decoder.field_config, quad=0,
                                          one_launch=one_launch)


@pytest.mark.parametrize('one_launch', [False, True])
def test_decode_ragged_from_conv(cifcaf, one_launch):
    from openpifpaf_amd import engine
    from openpifpaf_amd._abi import skeleton_array
    fields_list = _parent_fields(cifcaf.case, _flips(cifcaf.case, cifcaf.half))
    want_set = engine.RaggedHeadSet(fields_list, cifcaf.field_config)
    got_set = _from_conv(cifcaf, one_launch)
    assert len(got_set.arr) == len(want_set.arr) == len(fields_list[0])
    for g, w in zip(got_set.cifs + got_set.cafs, want_set.cifs + want_set.cafs):
        assert g.shape == w.shape and _bytes(g) == _bytes(w)
    assert got_set.extents.cpu().numpy().tolist() == want_set.extents_host.tolist()
    assert got_set.extents_host.tolist() == want_set.extents_host.tolist()
    for key in ('n', 'k', 'c', 'h', 'w', 'stride0', 'pairs', 'shape_key'):
        assert getattr(got_set, key) == getattr(want_set, key), key
    # the records, whole
    eng = engine.DecodeEngine()
    got, got_off, _ = eng.decode(None, None, skeleton_array(cifcaf.skeleton), cifcaf.config(),
                                 ragged=got_set)
    got, got_off = got.copy(), np.array(got_off)
    want, want_off, _ = eng.decode(None, None, skeleton_array(cifcaf.skeleton), cifcaf.config(),
                                   ragged=want_set)
    print(cifcaf.case, cifcaf.half, 'annotations per image', np.diff(got_off).tolist())
    assert got_off.tolist() == np.array(want_off).tolist() and len(got_off) == 7
    assert got.tobytes() == want.tobytes()
    assert got_off[-1] >= 1
    # ... and the annotations of the public entry point
    anns = cifcaf.decode_ragged(got_set)
    ref = cifcaf.decode_ragged(fields_list)
    assert [len(a) for a in anns] == [len(a) for a in ref] == np.diff(got_off).tolist()
    for a, r in zip(anns, ref):
        for x, y in zip(a, r):
            assert x.data.tobytes() == y.data.tobytes()
            assert x.joint_scales.tobytes() == y.joint_scales.tobytes()


@pytest.mark.parametrize('one_launch', [False, True])
def test_coco_ragged_from_conv(cifcaf, one_launch):
    from test_oracle_golden import inverse_metas
    named = inverse_metas()
    metas = [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=70 + i) for i in range(6)]
    fields_list = _parent_fields(cifcaf.case, _flips(cifcaf.case, cifcaf.half))
    got = cifcaf.coco_ragged(_from_conv(cifcaf, one_launch), metas, max_per_image=5)
    want = cifcaf.coco_ragged(fields_list, metas, max_per_image=5)
    assert got.offsets.tolist() == want.offsets.tolist() and got.offsets[-1] >= 1
    assert got.flags.tolist() == want.flags.tolist()
    assert got.records.tobytes() == want.records.tobytes()


@pytest.mark.parametrize('dense', [False, True])
def test_ragged_multi_scale_collector(dense):
    """ms2's two scales as the unflipped and the mirrored pass of one scale each."""
    import torch
    from openpifpaf_amd import decoder, engine, heads
    from test_gpu_ingest_strided import DENSE, KPS, SKEL
    fc = decoder.FieldConfig(**rmu.field_config_kwargs('ms2'))
    planted = _planted('ms2')
    rng = np.random.default_rng(3)
    convs, fields = [], [[] for _ in SIX]
    for s in range(2):
        cif, caf = list(planted[2 * s]), list(planted[2 * s + 1])
        convs += [cif, caf]
        flips = (heads.cif_hflip(KPS), heads.caf_hflip(KPS, SKEL), heads.caf_hflip(KPS, DENSE))
        flips = flips if s else (None, None, None)
        if dense:
            convs.append([_values(rng, 'float32', (len(DENSE) * 9,) + tuple(c.shape[1:]))
                          for c in caf])
        for i in range(len(SIX)):
            fields[i].append(heads.fields_from_conv(cif[i][None], 17, 'cif', 0, hflip=flips[0])[0])
            both = heads.fields_from_conv(caf[i][None], 19, 'caf', 0, hflip=flips[1])[0]
            if dense:
                more = heads.fields_from_conv(convs[-1][i][None], len(DENSE), 'caf', 0,
                                              hflip=flips[2])[0]
                both = torch.cat([both, more]).contiguous()
            fields[i].append(both)
    want = engine.RaggedHeadSet(fields, fc)
    collector = heads.RaggedMultiScaleCollector(KPS, SKEL, fc, dense_skeleton=DENSE if dense
                                                else None, quad=0, n_scales=1)
    got = collector(convs)
    assert isinstance(got, engine.RaggedHeadSet)
    assert (got.k, got.c) == (17, 19 + (len(DENSE) if dense else 0)) == (want.k, want.c)
    for g, w in zip(got.cifs + got.cafs, want.cifs + want.cafs):
        assert g.shape == w.shape and _bytes(g) == _bytes(w)
    assert got.extents.cpu().numpy().tolist() == want.extents_host.tolist()
    assert got.shape_key == want.shape_key
    with pytest.raises(ValueError):
        collector(convs[:-1])
    if not dense:
        eng, cfg = engine.DecodeEngine(), rmu.config('eval')
        a, a_off, _ = eng.decode(None, None, rmu.SKEL, cfg, ragged=got)
        a, a_off = a.copy(), np.array(a_off)
        b, b_off, _ = eng.decode(None, None, rmu.SKEL, cfg, ragged=want)
        assert a_off.tolist() == np.array(b_off).tolist() and a_off[-1] >= 1
        assert a.tobytes() == b.tobytes()


# ---- 8. Python errors ---------------------------------------------------------------------
@pytest.mark.parametrize('one_launch', [False, True])
def test_python_errors(one_launch):
    import functools as ft
    import torch
    from openpifpaf_amd import decoder, engine
    from_conv = ft.partial(engine.RaggedHeadSet.from_conv, one_launch=one_launch)
    entries = _same_extent_entries('float32', False)
    fc = _field_config(2)
    items = [list(e[3]) for e in entries]
    assert from_conv(items, fc).n == 6
    with pytest.raises(ValueError, match='numbers of images'):
        from_conv(items[:3] + [items[3][:5]], fc)
    k16 = [c[:16 * 5 * 4] for c in items[2]]
    with pytest.raises(ValueError, match='K or C'):  # a head of another K
        from_conv(items[:2] + [k16, items[3]], fc)
    with pytest.raises(ValueError, match='K or C|channels'):  # an image of another K
        from_conv(items[:2] + [items[2][:5] + [k16[5]], items[3]], fc)
    with pytest.raises(ValueError, match='K or C|channels'):  # an image of another C
        from_conv(items[:3] + [items[3][:5] + [items[3][5][:18 * 9 * 4]]], fc)
    short = decoder.FieldConfig(cif_indices=[0, 2], caf_indices=[1, 3], cif_strides=[8, 16],
                                caf_strides=[8, 16], cif_min_scales=[0.0],
                                caf_min_distances=[0.0, 0.0], caf_max_distances=[None, None])
    with pytest.raises(NotImplementedError, match='cif_min_scales'):
        from_conv(items, short)
    with pytest.raises(ValueError, match='conv_extents'):
        from_conv(items, fc, conv_extents=EXTENTS)
    with pytest.raises(ValueError, match='head'):  # fewer heads than the config reads
        from_conv(items[:3], fc)
    with pytest.raises(ValueError):  # a host tensor
        from_conv(items[:3] + [[c.cpu() for c in items[3]]], fc)
    if one_launch:
        with pytest.raises(ValueError):  # one launch reads one type
            from_conv(items[:3] + [[c.half() for c in items[3]]], fc)
    with pytest.raises(ValueError):  # parts of one container that differ in size
        from_conv(items[:3] + [[(items[3], 19, None), (items[1][::-1], 19, None)]], fc)
    cif, caf = (torch.zeros((6, n * 4, 5, 7), device='cuda') for n in (17 * 5, 19 * 9))
    assert from_conv([cif, caf, cif, caf], fc, conv_extents=EXTENTS).n == 6
    for rows in ([(1, 1)] * 5 + [(6, 7)], [(1, 1)] * 5 + [(5, 8)], [(1, 1)] * 5 + [(0, 1)],
                 EXTENTS[:5]):
        with pytest.raises(ValueError, match='conv_extents'):  # a row beyond the batched tensor
            from_conv([cif, caf, cif, caf], fc, conv_extents=rows)
