"""Ragged batches on the host: the twin pp_decode_ragged_cpu (stages_cpu.decode_ragged) is the
executable definition of the feature -- every image of a batch of mixed field sizes decodes
as it would alone at its own size.  Against the per-image decode and the C oracle, bit for
bit; a guard that the same images decode to OTHER annotations when zero-padded to the
container and decoded by the uniform entry point (so these inputs tell the two apart); and
the argument checks.  No GPU."""
import numpy as np
import pytest

import oracle
import ragged_util as ru
from openpifpaf_amd import constants, decoder, stages_cpu
from openpifpaf_amd._lib import PPError

SKEL = constants.COCO_PERSON_SKELETON


@pytest.fixture(scope='module')
def one_thread():
    """decode_ragged on one thread of the six shapes, per (case, seed): made once."""
    out = {}
    for kind, mode in ru.CASES:
        for seed in ru.SEEDS:
            cifs, cafs = zip(*ru.images(kind, [(s, seed) for s in ru.SHAPES]))
            out[kind, mode, seed] = stages_cpu.decode_ragged(list(cifs), list(cafs), SKEL,
                                                             ru.config(mode), n_threads=1)
    return out


@pytest.mark.parametrize('kind,mode', ru.CASES)
def test_twin_equals_own_size_decode_and_oracle(one_thread, kind, mode):
    cfg = ru.config(mode)
    total = 0
    for seed in ru.SEEDS:
        recs, offsets = one_thread[kind, mode, seed]
        assert len(offsets) == len(ru.SHAPES) + 1
        for i, (h, w) in enumerate(ru.SHAPES):
            got = recs[offsets[i]:offsets[i + 1]]
            ru.assert_same_records(got, ru.own_decode(kind, h, w, seed, mode, cfg), i)
            cif, caf = ru.image(kind, h, w, seed)
            ru.assert_same_records(got, oracle.decode(cif, caf, SKEL, cfg), i, ru.ORACLE_KEYS)
            total += len(got)
    assert total > 0


@pytest.mark.parametrize('kind,mode', ru.CASES)
def test_twin_three_threads(one_thread, kind, mode):
    for seed in ru.SEEDS:
        cifs, cafs = zip(*ru.images(kind, [(s, seed) for s in ru.SHAPES]))
        recs, offsets = stages_cpu.decode_ragged(list(cifs), list(cafs), SKEL, ru.config(mode),
                                                 n_threads=3)
        want, want_off = one_thread[kind, mode, seed]
        assert offsets.tolist() == want_off.tolist() and recs.tobytes() == want.tobytes()


@pytest.mark.parametrize('kind,mode', ru.CASES)
def test_zero_padding_gives_other_annotations(kind, mode):
    """The guard: decoded by the uniform decode_batch after zero-padding to 24x30, at least 4
    of the 6 seeds give other records than the own-size decode, at each of the five shapes
    smaller than the container."""
    cfg = ru.config(mode)
    for h, w in ru.SHAPES[:-1]:
        differ = 0
        for seed in ru.SEEDS:
            cif, caf = ru.image(kind, h, w, seed)
            big = ru.image(kind, *ru.CONTAINER, seed)  # only its size is used
            pad_cif, pad_caf = ru.padded([cif, big[0]])[:1], ru.padded([caf, big[1]])[:1]
            assert pad_cif.shape[3:] == ru.CONTAINER
            got, _ = stages_cpu.decode_batch(pad_cif, pad_caf, SKEL, cfg, n_threads=1)
            want = ru.own_decode(kind, h, w, seed, mode, cfg)
            same = len(got) == len(want) and all(
                got[k].tobytes() == want[k].tobytes() for k in ru.ORACLE_KEYS)
            differ += not same
        print('{} {} {}x{}: {} of {} seeds differ under padding'.format(
            kind, mode, h, w, differ, len(ru.SEEDS)))
        assert differ >= 4, (h, w, differ)


def test_equal_shapes_equal_decode_batch():
    cfg = ru.config('eval')
    cifs, cafs = zip(*ru.images('planted', [((14, 14), s) for s in range(3)]))
    recs, offsets = stages_cpu.decode_ragged(list(cifs), list(cafs), SKEL, cfg)
    want, want_off = stages_cpu.decode_batch(np.stack(cifs), np.stack(cafs), SKEL, cfg)
    assert offsets.tolist() == want_off.tolist() and recs.tobytes() == want.tobytes()


def _raw(ext, h=8, w=8, cfg=None, n=1):
    import ctypes
    from openpifpaf_amd._abi import ANN_DTYPE
    from openpifpaf_amd._lib import call
    cif = np.zeros((n, 17, 5, h, w), np.float32)
    caf = np.zeros((n, 19, 9, h, w), np.float32)
    ext = np.asarray(ext, np.int32).reshape(n, 2)
    sk = np.asarray(SKEL, np.int32)
    anns, counts, status = np.zeros((n, 8), ANN_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.int32)
    cfg = cfg or ru.config('eval')
    call('pp_decode_ragged_cpu', cif.ctypes.data, caf.ctypes.data, n, 17, 19, h, w,
         ext.ctypes.data, sk.ctypes.data, ctypes.byref(cfg), anns.ctypes.data, 8,
         counts.ctypes.data, status.ctypes.data, 1)
    return counts


def test_argument_checks():
    assert _raw([8, 8]).tolist() == [0] and _raw([1, 1]).tolist() == [0]
    for bad in ([9, 8], [8, 9], [0, 8], [8, 0], [-1, 4]):
        with pytest.raises(PPError, match='PP_ESHAPE'):
            _raw(bad)
    for name in ('cif_threshold', 'seed_threshold', 'caf_threshold', 'complete_caf_threshold'):
        with pytest.raises(PPError, match='PP_EINVAL'):
            _raw([8, 8], cfg=ru.config('eval', **{name: -0.5}))
    cif, caf = ru.image('planted', 13, 17, 0)
    cfg = ru.config('eval')
    with pytest.raises(ValueError, match='fields or channels'):  # K differs
        stages_cpu.decode_ragged([cif, cif[:16]], [caf, caf], SKEL, cfg)
    with pytest.raises(ValueError, match='fields or channels'):  # C differs
        stages_cpu.decode_ragged([cif, cif], [caf, caf[:18]], SKEL, cfg)
    with pytest.raises(ValueError, match='spatial'):
        stages_cpu.decode_ragged([cif], [ru.image('planted', 14, 14, 0)[1]], SKEL, cfg)
    with pytest.raises(ValueError):
        stages_cpu.decode_ragged([cif], [caf, caf], SKEL, cfg)


def test_multi_scale_field_config_is_refused():
    fc = decoder.FieldConfig(cif_indices=[0, 2], caf_indices=[1, 3], cif_strides=[8, 16],
                             caf_strides=[8, 16])
    cc = decoder.CifCaf(fc, keypoints=constants.COCO_KEYPOINTS, skeleton=SKEL)
    cif, caf = ru.image('planted', 13, 17, 0)
    with pytest.raises(NotImplementedError, match='single-scale'):
        cc.decode_ragged([[cif, caf, cif, caf]])
    one = decoder.CifCaf(decoder.FieldConfig(), keypoints=constants.COCO_KEYPOINTS, skeleton=SKEL)
    for kw in ({'group': object()}, {'initial_annotations': [object()]}, {'keep_cifhr': True}):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            one.decode_ragged([[cif, caf]], **kw)
