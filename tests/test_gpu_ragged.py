"""Ragged batches on an MI355X: pp_fields_pack_ragged and pp_decode_ragged
(engine.RaggedFields, DecodeEngine.decode(ragged=...), CifCaf.decode_ragged / coco_ragged).

Every image of a batch of mixed field sizes must come out, byte for byte, as the host twin
decodes it alone at its own size (tests/test_ragged_cpu.py ties the twin to the oracle and
shows that zero-padding gives other annotations for these very images).  The batch of six
(one image per shape) runs the split CifHr kernels, seed_loop_ext_kernel and
complete_kernel; the batch of 136 the fused CifHr kernel and the one-CU seed_loop_kernel."""
import numpy as np
import pytest

import ragged_util as ru
from openpifpaf_amd._abi import PP_COCO_EMPTY

pytestmark = pytest.mark.gpu

SIX = [(s, 0) for s in ru.SHAPES]


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def _fields(torch, kind, shapes_seeds, skeleton='coco'):
    return [(torch.tensor(cif).cuda(), torch.tensor(caf).cuda())
            for cif, caf in ru.images(kind, shapes_seeds, skeleton)]


def _decode(torch, kind, shapes_seeds, cfg, skeleton='coco', cap=None, eng=None):
    from openpifpaf_amd import engine
    eng = eng or engine.DecodeEngine()
    ragged = engine.RaggedFields(_fields(torch, kind, shapes_seeds, skeleton))
    recs, offsets, b = eng.decode(None, None, ru.SKELETONS[skeleton], cfg, cap=cap,
                                  ragged=ragged)
    return recs.copy(), np.array(offsets), b


def _check(got, offsets, kind, shapes_seeds, cfg_key, cfg, skeleton='coco'):
    assert len(offsets) == len(shapes_seeds) + 1
    for i, ((h, w), seed) in enumerate(shapes_seeds):
        ru.assert_same_records(got[offsets[i]:offsets[i + 1]],
                               ru.own_decode(kind, h, w, seed, cfg_key, cfg, skeleton), i)


# ---- the packer ---------------------------------------------------------------------------
@pytest.mark.parametrize('shapes', [
    ru.SHAPES,                      # container W = 30: 4-byte stores; w_i = 17, 13, 14
    [(13, 17), (24, 32), (5, 30)],  # container W = 32: 16-byte stores over w_i = 17 and 30
    [(14, 14)],                     # n = 1, 4-byte stores
    [(16, 16)],                     # n = 1, 16-byte stores
])
def test_pack_equals_numpy_padding(torch, shapes):
    from openpifpaf_amd import engine
    rng = np.random.default_rng(len(shapes))
    cifs = [rng.standard_normal((17, 5, h, w)).astype(np.float32) for h, w in shapes]
    cafs = [rng.standard_normal((19, 9, h, w)).astype(np.float32) for h, w in shapes]
    ragged = engine.RaggedFields([(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
                                  for a, b in zip(cifs, cafs)])
    assert (ragged.h, ragged.w) == tuple(np.max(shapes, axis=0))
    assert ragged.cif.cpu().numpy().tobytes() == ru.padded(cifs).tobytes()
    assert ragged.caf.cpu().numpy().tobytes() == ru.padded(cafs).tobytes()
    assert ragged.extents.cpu().numpy().tolist() == [list(s) for s in shapes]
    assert ragged.extents_host.tolist() == [list(s) for s in shapes]


def test_pack_overwrites_a_dirty_container(torch):
    """No memset is needed: packing into memory full of NaN leaves none behind."""
    import ctypes
    from openpifpaf_amd import _device
    from openpifpaf_amd._lib import call, load
    shapes = [(3, 5), (7, 4), (6, 8)]
    rng = np.random.default_rng(3)
    host = [rng.standard_normal((2, 3, h, w)).astype(np.float32) for h, w in shapes]
    dev = [torch.from_numpy(a).cuda() for a in host]
    for width in (8, 9):  # 16-byte and 4-byte stores
        out = torch.full((3, 2, 3, 7, width), float('nan'), device='cuda')
        ptrs = np.array([t.data_ptr() for t in dev], np.uint64)
        ext = np.array(shapes, np.int32)
        tables = torch.empty(load().pp_ragged_tables_size(3), dtype=torch.uint8, device='cuda')
        call('pp_fields_pack_ragged', ptrs.ctypes.data, ext.ctypes.data, 3, 2, 3, 7, width,
             _device.ptr(out), _device.ptr(tables), ctypes.c_size_t(tables.numel()),
             _device.stream())
        want = np.zeros((3, 2, 3, 7, width), np.float32)
        for i, a in enumerate(host):
            want[i, :, :, :a.shape[2], :a.shape[3]] = a
        assert out.cpu().numpy().tobytes() == want.tobytes()


# ---- the decode ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind,mode', ru.CASES)
def test_six_images_vs_twin_and_oracle(torch, kind, mode):
    import oracle
    cfg = ru.config(mode)
    got, offsets, _ = _decode(torch, kind, SIX, cfg)
    _check(got, offsets, kind, SIX, mode, cfg)
    for i, ((h, w), seed) in enumerate(SIX):
        cif, caf = ru.image(kind, h, w, seed)
        ru.assert_same_records(got[offsets[i]:offsets[i + 1]],
                               oracle.decode(cif, caf, ru.SKELETONS['coco'], cfg), i,
                               ru.ORACLE_KEYS)
    assert offsets[-1] >= len(SIX)


@pytest.mark.parametrize('kind,mode', [('planted', 'eval'), ('uniform', 'eval')])
def test_136_images_vs_twin(torch, kind, mode):
    cfg = ru.config(mode)
    batch = [(ru.SHAPES[i % len(ru.SHAPES)], i) for i in range(136)]
    got, offsets, _ = _decode(torch, kind, batch, cfg)
    _check(got, offsets, kind, batch, mode, cfg)
    assert offsets[-1] >= 136


@pytest.mark.parametrize('n', [6, 136])
def test_separate_seeds_kernel(torch, n):
    """seed_threshold below the CifHr threshold: the seeds come from seeds_emit_kernel instead
    of the CifHr kernel."""
    cfg = ru.config('eval', seed_threshold=0.05)
    batch = [(ru.SHAPES[i % len(ru.SHAPES)], i) for i in range(n)]
    got, offsets, _ = _decode(torch, 'planted', batch, cfg)
    _check(got, offsets, 'planted', batch, 'eval_seed005', cfg)


@pytest.mark.parametrize('key,kw', [('max', {'connection_method': 'max'}),
                                    ('greedy', {'greedy': True})])
def test_connection_method_and_greedy(torch, key, kw):
    cfg = ru.config('eval', **kw)
    got, offsets, _ = _decode(torch, 'planted', SIX, cfg)
    _check(got, offsets, 'planted', SIX, 'eval_' + key, cfg)


def test_dense_skeleton(torch):
    """44 edges, 88 directed ones: the two-slot frontier."""
    cfg = ru.config('eval')
    got, offsets, _ = _decode(torch, 'planted', SIX, cfg, skeleton='dense')
    _check(got, offsets, 'planted', SIX, 'eval', cfg, skeleton='dense')
    assert offsets[-1] >= len(SIX)


def test_equal_shapes_equal_decode_batch(torch):
    from openpifpaf_amd import engine
    cfg = ru.config('eval')
    batch = [((21, 16), s) for s in range(6)]
    got, offsets, _ = _decode(torch, 'planted', batch, cfg)
    cifs, cafs = zip(*ru.images('planted', batch))
    want, want_off, _ = engine.DecodeEngine().decode(
        torch.from_numpy(np.stack(cifs)).cuda(), torch.from_numpy(np.stack(cafs)).cuda(),
        ru.SKELETONS['coco'], cfg)
    assert offsets.tolist() == np.array(want_off).tolist() and got.tobytes() == want.tobytes()


def test_capacity_retry_and_repeat(torch):
    """From 4 annotations per image the capacity doubles until the dense images fit; the
    same batch again gives the same bytes."""
    from openpifpaf_amd import engine
    cfg = ru.config('eval')
    eng = engine.DecodeEngine()
    got, offsets, b = _decode(torch, 'uniform', SIX, cfg, cap=4, eng=eng)
    assert b.cap > 4 and np.diff(offsets).max() > 4
    _check(got, offsets, 'uniform', SIX, 'eval', cfg)
    again, again_off, _ = _decode(torch, 'uniform', SIX, cfg, cap=4, eng=eng)
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


@pytest.fixture()
def cifcaf():
    from openpifpaf_amd import constants, decoder as dec
    _eval_defaults(dec)
    yield dec.CifCaf(dec.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                     skeleton=constants.COCO_PERSON_SKELETON)
    dec.CifSeeds.threshold = None


def test_decode_ragged_annotations(torch, cifcaf):
    cfg = ru.config('eval')
    fields_list = [list(f) for f in _fields(torch, 'planted', SIX)]
    anns = cifcaf.decode_ragged(fields_list)
    assert len(anns) == len(SIX)
    for i, ((h, w), seed) in enumerate(SIX):
        want = ru.own_decode('planted', h, w, seed, 'eval', cfg)
        assert len(anns[i]) == len(want)
        for a, r in zip(anns[i], want):
            assert a.data.tobytes() == r['data'][:17].tobytes()
            assert np.asarray(a.joint_scales, np.float32).tobytes() == r['joint_scales'][:17].tobytes()
    for kw in ({'initial_annotations': [object()]}, {'group': object()}, {'keep_cifhr': True}):
        with pytest.raises(NotImplementedError):
            cifcaf.decode_ragged(fields_list, **kw)


def test_coco_ragged(torch, cifcaf):
    """The COCO records of the ragged batch are the host twin's over the per-image decodes'
    records under the same metas: one flipped, one rotated, and a blank image (no annotation,
    so from_predictions' empty record)."""
    from test_oracle_golden import inverse_metas
    from openpifpaf_amd import eval_coco, transforms
    cfg = ru.config('eval')
    named = inverse_metas()
    batch = SIX + [((9, 11), 0)]
    fields_list = [list(f) for f in _fields(torch, 'planted', SIX)]
    fields_list.append([torch.zeros((17, 5, 9, 11), device='cuda'),
                        torch.zeros((19, 9, 9, 11), device='cuda')])
    metas = [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=70 + i)
             for i in range(len(batch))]
    assert any(m['hflip'] for m in metas)
    got = cifcaf.coco_ragged(fields_list, metas, max_per_image=5)
    own = [ru.own_decode('planted', h, w, seed, 'eval', cfg) for (h, w), seed in SIX]
    own.append(own[0][:0])
    cap = max(1, max(len(r) for r in own))
    recs = np.zeros((len(own), cap), own[0].dtype)
    for i, r in enumerate(own):
        recs[i, :len(r)] = r
    block = np.concatenate([transforms.meta_record(m) for m in metas])
    ids = np.array([m['image_id'] for m in metas], np.int64)
    swap = next(transforms.swap_table(m['horizontal_swap'], 17) for m in metas
                if m['hflip'] and m.get('horizontal_swap'))
    want = eval_coco.coco_records_cpu(recs, np.array([len(r) for r in own], np.int32), block,
                                      ids, k=17, hswap=swap, max_per_image=5)
    assert got.offsets.tolist() == want.offsets.tolist()
    assert got.flags.tolist() == want.flags.tolist()
    assert got.records.tobytes() == want.records.tobytes()
    assert got.flags[-1] & PP_COCO_EMPTY and not got.flags[0] & PP_COCO_EMPTY
