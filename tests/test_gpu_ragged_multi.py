"""Ragged multi-scale batches on an MI355X: pp_fields_pack_ragged_heads and
pp_decode_multi_ragged (engine.RaggedHeadSet, DecodeEngine.decode(ragged=...),
CifCaf.decode_ragged / coco_ragged with a multi-scale FieldConfig).

Every image of a batch of mixed pixel sizes, each head at its own field size, must come out as
the oracle decodes it alone (tests/test_ragged_multi_cpu.py shows that zero-padding gives
other records for these very images).  The batch of six (one image per size) runs the split
CifHr fold and seed_loop_ext_kernel, the batch of 136 one workgroup per field and
seed_loop_kernel."""
import ctypes

import numpy as np
import pytest

import ragged_multi_util as rmu
import ragged_util as ru

pytestmark = pytest.mark.gpu

SIX = [(p, 0) for p in rmu.PIXELS]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def _fields(torch, name, pixels_seeds):
    return [[torch.tensor(f).cuda() for f in img] for img in rmu.images(name, pixels_seeds)]


def _field_config(name):
    from openpifpaf_amd import decoder
    return decoder.FieldConfig(**rmu.field_config_kwargs(name))


def _head_set(torch, name, pixels_seeds):
    from openpifpaf_amd import engine
    return engine.RaggedHeadSet(_fields(torch, name, pixels_seeds), _field_config(name))


def _decode(torch, name, pixels_seeds, cfg, cap=None, eng=None):
    from openpifpaf_amd import engine
    eng = eng or engine.DecodeEngine()
    recs, offsets, b = eng.decode(None, None, rmu.SKEL, cfg, cap=cap,
                                  ragged=_head_set(torch, name, pixels_seeds))
    return recs.copy(), np.array(offsets), b


def _check(got, offsets, name, pixels_seeds, cfg_key, cfg):
    assert len(offsets) == len(pixels_seeds) + 1
    for i, ((h, w), seed) in enumerate(pixels_seeds):
        ru.assert_same_records(got[offsets[i]:offsets[i + 1]],
                               rmu.own_decode(name, h, w, seed, cfg_key, cfg), i, ru.ORACLE_KEYS)
        assert (got['image'][offsets[i]:offsets[i + 1]] == i).all()


# ---- the packer ---------------------------------------------------------------------------
def test_pack_20_heads_equals_numpy_padding(torch):
    hs = _head_set(torch, 'ms10', SIX)
    want = rmu.padded(rmu.images('ms10', SIX))
    assert len(hs.cifs) == len(hs.cafs) == 10 and len(hs.arr) == 20
    for m in range(10):
        assert hs.cifs[m].cpu().numpy().tobytes() == want[2 * m].tobytes(), m
        assert hs.cafs[m].cpu().numpy().tobytes() == want[2 * m + 1].tobytes(), m
    # entry-major (n_heads, n_img, 2), CIF heads first: the sub-table of CIF head 0 is the
    # (n_img, 2) table of its sizes
    sizes = [[f.shape[2:] for f in img] for img in rmu.images('ms10', SIX)]
    table = np.array([[sizes[i][j] for i in range(6)]
                      for j in list(range(0, 20, 2)) + list(range(1, 20, 2))], np.int32)
    assert hs.extents.shape == (20, 6, 2)
    assert hs.extents.cpu().numpy().tolist() == table.tolist()
    assert hs.extents_host.tolist() == table.tolist()
    strides = rmu.field_config_kwargs('ms10')['cif_strides']
    assert [(s.H, s.W) for s in hs.arr] == [(24, 30) if st == 8 else (12, 15) for st in strides] * 2
    assert [s.stride for s in hs.arr] == strides * 2
    assert (hs.h, hs.w, hs.k, hs.c, hs.n, hs.pairs) == (24, 30, 17, 19, 6, 1)


@pytest.mark.parametrize('widths', [(8,), (9,), (8, 9, 12), (7, 30, 6)])
def test_pack_overwrites_dirty_containers(torch, widths):
    """One head and several, container widths that are and are not multiples of 4 (16-byte
    stores and head / tail elements), separate (pageable) host tables: packing into memory
    full of NaN leaves none behind and equals NumPy padding."""
    from openpifpaf_amd import _device
    from openpifpaf_amd._lib import call, load
    n, nh = 3, len(widths)
    rng = np.random.default_rng(nh)
    planes = [(2, 3), (3, 5), (1, 9)][:nh]
    H = [7, 5, 6][:nh]
    host = [[rng.standard_normal(planes[m] + (int(rng.integers(1, H[m] + 1)),
                                              int(rng.integers(1, widths[m] + 1))))
             .astype(np.float32) for _ in range(n)] for m in range(nh)]
    host[0][1] = rng.standard_normal(planes[0] + (H[0], widths[0])).astype(np.float32)
    dev = [[torch.from_numpy(a).cuda() for a in row] for row in host]
    outs = [torch.full((n,) + planes[m] + (H[m], widths[m]), float('nan'), device='cuda')
            for m in range(nh)]
    ptrs = np.array([t.data_ptr() for row in dev for t in row], np.uint64)
    ext = np.array([a.shape[2:] for row in host for a in row], np.int32)
    pl = np.array([p[0] * p[1] for p in planes], np.int32)
    sizes = np.array([(H[m], widths[m]) for m in range(nh)], np.int32)
    cont = np.array([t.data_ptr() for t in outs], np.uint64)
    tables = torch.empty(load().pp_ragged_heads_tables_size(n, nh), dtype=torch.uint8,
                         device='cuda')
    call('pp_fields_pack_ragged_heads', ptrs.ctypes.data, ext.ctypes.data, n, nh, pl.ctypes.data,
         sizes.ctypes.data, cont.ctypes.data, _device.ptr(tables),
         ctypes.c_size_t(tables.numel()), _device.stream())
    for m in range(nh):
        want = np.zeros((n,) + planes[m] + (H[m], widths[m]), np.float32)
        for i, a in enumerate(host[m]):
            want[i, :, :, :a.shape[2], :a.shape[3]] = a
        assert outs[m].cpu().numpy().tobytes() == want.tobytes(), m
    off = load().pp_ragged_heads_extents_offset(n, nh)
    assert tables[off:].view(torch.int32).cpu().numpy().tolist() == ext.reshape(-1).tolist()


def test_head_set_argument_checks(torch):
    from openpifpaf_amd import decoder, engine
    fc = _field_config('ms2')
    fields = _fields(torch, 'ms2', SIX[:2])
    with pytest.raises(ValueError, match='at least one image'):
        engine.RaggedHeadSet([], fc)
    with pytest.raises(ValueError, match='float32'):  # a host array
        engine.RaggedHeadSet([[rmu.image('ms2', 97, 129, 0)[0]] + fields[0][1:]], fc)
    with pytest.raises(ValueError, match='float32'):  # dtype
        engine.RaggedHeadSet([[fields[0][0].half()] + fields[0][1:]], fc)
    with pytest.raises(ValueError, match='contiguous'):
        engine.RaggedHeadSet([[fields[0][0].transpose(2, 3)] + fields[0][1:]], fc)
    with pytest.raises(ValueError, match='contiguous'):  # a batch dimension
        engine.RaggedHeadSet([[f[None] for f in fields[0]]], fc)
    with pytest.raises(ValueError, match='CIF heads'):  # CIF and CAF swapped
        engine.RaggedHeadSet([[fields[0][1], fields[0][0]] + fields[0][2:]], fc)
    with pytest.raises(ValueError, match='K or C'):
        engine.RaggedHeadSet([fields[0], [fields[1][0][:16].contiguous()] + fields[1][1:]], fc)
    with pytest.raises(ValueError, match='K or C'):  # between the heads of one image
        engine.RaggedHeadSet([fields[0][:3] + [fields[0][3][:18].contiguous()]], fc)
    with pytest.raises(ValueError, match='reads head 3'):  # fewer heads than the config names
        engine.RaggedHeadSet([fields[0][:3]], fc)
    short = decoder.FieldConfig(**dict(rmu.field_config_kwargs('ms2'), cif_strides=[8]))
    with pytest.raises(NotImplementedError, match='2 CIF and 2 CAF heads, but cif_strides has 1'):
        engine.RaggedHeadSet(fields, short)
    with pytest.raises(NotImplementedError, match='HeadSet'):
        engine.DecodeEngine().launch_checked(None, None, rmu.SKEL, rmu.config('eval'),
                                             heads=object(), ragged=engine.RaggedHeadSet(fields, fc))
    torch.cuda.synchronize()


# ---- the decode ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', rmu.MODES)
@pytest.mark.parametrize('name', rmu.CONFIGS)
def test_six_images_vs_oracle(torch, name, mode):
    cfg = rmu.config(mode)
    got, offsets, _ = _decode(torch, name, SIX, cfg)
    _check(got, offsets, name, SIX, mode, cfg)
    if name in rmu.PLANTED:
        assert (np.diff(offsets) >= 1).all()


@pytest.mark.parametrize('name', ['ms2', 'ms10'])
def test_136_images_vs_oracle(torch, name):
    cfg = rmu.config('eval')
    batch = [(rmu.PIXELS[i % len(rmu.PIXELS)], i) for i in range(136)]
    got, offsets, _ = _decode(torch, name, batch, cfg)
    _check(got, offsets, name, batch, 'eval', cfg)
    assert offsets[-1] >= 136


@pytest.mark.parametrize('name', ['ms2', 'ms10'])
def test_equal_sizes_equal_decode_multi(torch, name):
    from openpifpaf_amd import engine
    cfg = rmu.config('eval')
    batch = [((161, 121), s) for s in range(6)]
    got, offsets, _ = _decode(torch, name, batch, cfg)
    imgs = rmu.images(name, batch)
    stacked = [torch.from_numpy(np.stack([img[m] for img in imgs])).cuda()
               for m in range(len(imgs[0]))]
    want, want_off, _ = engine.DecodeEngine().decode(
        None, None, rmu.SKEL, cfg, heads=engine.HeadSet(stacked, _field_config(name)))
    assert offsets.tolist() == np.array(want_off).tolist() and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('kind', ['planted', 'uniform'])
def test_one_cif_one_caf_head_equals_decode_ragged(torch, kind):
    from openpifpaf_amd import decoder, engine
    cfg = ru.config('eval')
    six = [(s, 0) for s in ru.SHAPES]
    fields = [[torch.tensor(cif).cuda(), torch.tensor(caf).cuda()]
              for cif, caf in ru.images(kind, six)]
    want, want_off, _ = engine.DecodeEngine().decode(
        None, None, rmu.SKEL, cfg, ragged=engine.RaggedFields([tuple(f) for f in fields]))
    want, want_off = want.copy(), np.array(want_off)
    got, offsets, _ = engine.DecodeEngine().decode(
        None, None, rmu.SKEL, cfg, ragged=engine.RaggedHeadSet(fields, decoder.FieldConfig()))
    assert np.array(offsets).tolist() == want_off.tolist() and got.tobytes() == want.tobytes()
    assert offsets[-1] >= 6


@pytest.mark.parametrize('name', ['ms10', 'coarse'])
def test_stage_by_stage_equals_one_call(torch, name):
    from openpifpaf_amd import engine
    cfg = rmu.config('eval')
    want, want_off, _ = _decode(torch, name, SIX, cfg)
    eng = engine.DecodeEngine()
    hs = _head_set(torch, name, SIX)
    for stage in (1, 2, 4, 8):
        b = eng.launch_ragged_multi(hs, rmu.SKEL, cfg, cap=128, stages=stage)
    got, offsets = eng.fetch(b)
    assert np.array(offsets).tolist() == want_off.tolist() and got.tobytes() == want.tobytes()


@pytest.mark.parametrize('name', ['ms2', 'ms10'])
@pytest.mark.parametrize('key,kw', [('max', {'connection_method': 'max'}),
                                    ('greedy', {'greedy': True})])
def test_connection_method_and_greedy(torch, name, key, kw):
    cfg = rmu.config('eval', **kw)
    got, offsets, _ = _decode(torch, name, SIX, cfg)
    _check(got, offsets, name, SIX, 'eval_' + key, cfg)


def test_capacity_retry_and_repeat(torch):
    """From one annotation per image the capacity doubles until every image fits; the same
    batch again gives the same bytes."""
    from openpifpaf_amd import engine
    cfg = rmu.config('eval')
    eng = engine.DecodeEngine()
    got, offsets, b = _decode(torch, 'ms2', SIX, cfg, cap=1, eng=eng)
    assert b.cap > 1 and np.diff(offsets).max() > 1
    _check(got, offsets, 'ms2', SIX, 'eval', cfg)
    again, again_off, _ = _decode(torch, 'ms2', SIX, cfg, cap=1, eng=eng)
    assert again_off.tolist() == offsets.tolist() and again.tobytes() == got.tobytes()


# ---- the decoder's entry points -----------------------------------------------------------
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


@pytest.fixture(params=['ms2', 'ms10'])
def cifcaf(request):
    from openpifpaf_amd import constants, decoder as dec
    _eval_defaults(dec)
    cc = dec.CifCaf(_field_config(request.param), keypoints=constants.COCO_KEYPOINTS,
                    skeleton=constants.COCO_PERSON_SKELETON)
    cc.case = request.param
    yield cc
    dec.CifSeeds.threshold = None


def test_decode_ragged_annotations(torch, cifcaf):
    from openpifpaf_amd import engine
    fields_list = _fields(torch, cifcaf.case, SIX)
    anns = cifcaf.decode_ragged(fields_list)
    assert len(anns) == len(SIX)
    for i, fields in enumerate(fields_list):
        want = cifcaf(fields)
        assert len(anns[i]) == len(want) >= 1
        for a, r in zip(anns[i], want):
            assert a.data.tobytes() == r.data.tobytes()
            assert (np.asarray(a.joint_scales, np.float32).tobytes() ==
                    np.asarray(r.joint_scales, np.float32).tobytes())
            assert a.score() == r.score()
    # a ready RaggedHeadSet is decoded as it is
    ready = engine.RaggedHeadSet(fields_list, cifcaf.field_config)
    again = cifcaf.decode_ragged(ready)
    assert [[a.data.tobytes() for a in img] for img in again] == \
        [[a.data.tobytes() for a in img] for img in anns]
    for kw in ({'initial_annotations': [object()]}, {'group': object()}, {'keep_cifhr': True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            cifcaf.decode_ragged(fields_list, **kw)
    with pytest.raises(TypeError, match='RaggedHeadSet'):
        cifcaf.decode_ragged(engine.RaggedFields([(fields_list[0][0], fields_list[0][1])]))


def test_coco_ragged(torch, cifcaf):
    """The COCO records of the ragged batch are those of coco_heads over every image alone
    under the same meta: shifted, flipped and rotated ones."""
    from test_oracle_golden import inverse_metas
    named = inverse_metas()
    fields_list = _fields(torch, cifcaf.case, SIX)
    metas = [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=70 + i)
             for i in range(len(SIX))]
    assert any(m['hflip'] for m in metas)
    got = cifcaf.coco_ragged(fields_list, metas, max_per_image=5)
    assert len(got.offsets) == len(SIX) + 1
    for i, fields in enumerate(fields_list):
        one = cifcaf.coco_heads([f[None] for f in fields], [metas[i]], max_per_image=5)
        assert got.records[got.offsets[i]:got.offsets[i + 1]].tobytes() == one.records.tobytes()
        assert got.flags[i] == one.flags[0]
        assert len(one.records) >= 1
