"""CIF / CAF target encoders without a GPU: the host twins (pp_encode_cif_cpu,
pp_encode_caf_cpu) against the reference's tensors (tests/golden/enc_*.npz, written by
tests/golden/gen_encoder.py), their helpers against NumPy, the refusals of the device entry
points (all before any HIP call), and the Python mirrors."""
import copy
import ctypes
import dataclasses

import numpy as np
import pytest

import encoder_util as eu
from openpifpaf_amd import _abi, _lib, encoder

RUNS = eu.fixture_runs()


def _encoder(name, which, stride):
    fx = eu.load_fixture(name)
    cif, caf = eu.encoders(eu.fixture_case(fx), stride)
    return fx, (cif if which == 'cif' else caf)


@pytest.mark.parametrize('name,which,stride', RUNS, ids=['%s-%s-s%d' % r for r in RUNS])
def test_twin_matches_reference(name, which, stride):
    """Every tensor of every fixture, bit for bit (NaN as 0x7FC00000 included)."""
    fx, enc = _encoder(name, which, stride)
    size, anns, meta = eu.fixture_scene(fx)
    got = enc.batch_cpu([size], [anns], [meta])
    want = eu.expected(fx, which, stride)
    assert len(got) == len(want)
    for g, e in zip(got, want):
        assert g.shape == (1,) + e.shape
        assert eu.same_bits(g[0], e)


@pytest.mark.parametrize('stride', eu.STRIDES)
def test_pose_45_matches_reference(stride):
    for name in ('two', 'chain5'):
        fx = eu.load_fixture(name)
        r = encoder.AnnRescaler(stride, int(fx['k']), np.array(fx['pose']))
        assert np.array_equal(r.pose_45, fx['s%d_pose_45' % stride])
        assert r.pose_45 is not r.pose and np.array_equal(r.pose, fx['pose'])


def test_norm_helper_is_numpys():
    """np.linalg.norm of a float32 pair (through x.dot(x)) is the unfused float32
    sqrt(x0 * x0 + x1 * x1) of the twin's helper, on 200,000 random pairs."""
    rng = np.random.default_rng(0)
    xy = (rng.standard_normal((200000, 2)) * 10.0 ** rng.uniform(-3, 3, (200000, 1)))
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.empty(len(xy), np.float32)
    _lib.call('pp_encode_norm_cpu', xy.ctypes.data_as(ctypes.c_void_p),
              out.ctypes.data_as(ctypes.c_void_p), len(xy))
    want = np.array([np.linalg.norm(p) for p in xy], np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # and the (n, 2) axis=1 form of cif.py:99
    assert np.array_equal(out, np.linalg.norm(xy, axis=1))


def test_linspace_helper_is_numpys():
    rng = np.random.default_rng(1)
    for num in range(2, 201):
        fmargin = float(rng.uniform(0.0, 0.4))
        out = np.empty(num, np.float64)
        _lib.call('pp_encode_linspace_cpu', fmargin, 1.0 - fmargin, num,
                  out.ctypes.data_as(ctypes.c_void_p))
        assert np.array_equal(out, np.linspace(fmargin, 1.0 - fmargin, num=num)), num


# ---- refusals: the device entry points return before any HIP call --------------------------

def _raw(enc, scene, name, edit=None, out=16, tables=16, tables_bytes=1 << 30, null=()):
    """Status and message of pp_encode_<name> on dummy device pointers."""
    size, anns, meta = scene
    cfg, keep = enc._config()
    images, ann_table, keypoints = enc._tables([size], [anns], [meta])
    elems, _ = enc._layout(images)
    if edit:
        edit(cfg, images, ann_table, keypoints)

    def vp(a, key):
        return None if key in null else a.ctypes.data_as(ctypes.c_void_p)
    lib = _lib.load()
    rc = getattr(lib, 'pp_encode_' + name)(
        None if 'enc' in null else ctypes.byref(cfg), vp(images, 'images'), len(images),
        vp(ann_table, 'anns'), vp(keypoints, 'keypoints'), len(ann_table),
        ctypes.c_void_p(out), elems, ctypes.c_void_p(tables), ctypes.c_size_t(tables_bytes), None)
    del keep
    return rc, lib.pp_last_error().decode()


@pytest.fixture(scope='module')
def two():
    fx = eu.load_fixture('two')
    cif, caf = eu.encoders(eu.fixture_case(fx), 8)
    return {'cif': cif, 'caf': caf}, eu.fixture_scene(fx)


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_refusals_before_launch(two, which):
    encs, scene = two
    enc = encs[which]
    for key in ('enc', 'images', 'anns', 'keypoints'):
        rc, msg = _raw(enc, scene, which, null=(key,))
        assert rc == -1 and 'NULL argument' in msg, key
    assert _raw(enc, scene, which, out=0)[0] == -1
    rc, msg = _raw(enc, scene, which, tables=0)
    assert rc == -1 and 'NULL argument' in msg
    rc, msg = _raw(enc, scene, which, tables_bytes=64)
    assert rc == -5 and 'too small' in msg

    def k25(cfg, *_):
        cfg.K = 25
    rc, msg = _raw(enc, scene, which, edit=k25)
    assert rc == -2 and 'PP_MAX_KP' in msg

    def nan_joint(cfg, images, anns, keypoints):
        keypoints[0, 3, 0] = np.nan
    rc, msg = _raw(enc, scene, which, edit=nan_joint)
    assert rc == -1 and 'non-finite' in msg

    def inf_joint(cfg, images, anns, keypoints):
        keypoints[1, 16, 1] = np.inf
    assert _raw(enc, scene, which, edit=inf_joint)[0] == -1

    def hidden_nan(cfg, images, anns, keypoints):  # v = 0: not a visible joint
        keypoints[0, 3] = (np.nan, np.nan, 0.0)
    assert _raw(enc, scene, which, edit=hidden_nan, tables_bytes=64)[0] == -5

    def same_joint(cfg, images, anns, keypoints):  # max_r = 0: the joint scale is 0
        keypoints[1, 5] = keypoints[0, 5]
    rc, msg = _raw(enc, scene, which, edit=same_joint)
    assert rc == -1 and 'asserts scale > 0' in msg

    def wrong_field(cfg, images, anns, keypoints):
        images['h'][0] += 1
    assert _raw(enc, scene, which, edit=wrong_field)[0] == -2

    def beyond(cfg, images, anns, keypoints):
        images['out_offset'][0][len(enc._shapes) - 1] += 1  # the last tensor ends the buffer
    assert _raw(enc, scene, which, edit=beyond)[0] == -2


def test_caf_refusals_before_launch(two):
    encs, scene = two

    def c65(cfg, *_):
        cfg.C = 65
    rc, msg = _raw(encs['caf'], scene, 'caf', edit=c65)
    assert rc == -2 and 'PP_MAX_EDGES' in msg

    def aspect(cfg, *_):
        cfg.aspect_ratio = 0.5
    rc, msg = _raw(encs['caf'], scene, 'caf', edit=aspect)
    assert rc == -1 and 'aspect_ratio' in msg

    def side9(cfg, *_):
        cfg.side = 9
    assert _raw(encs['caf'], scene, 'caf', edit=side9)[0] == -2
    grown = type('Caf', (encoder.Caf,), {'aspect_ratio': 0.5})
    with pytest.raises(NotImplementedError, match='aspect_ratio'):
        grown(encs['caf'].rescaler, skeleton=[(1, 2)], sigmas=None).batch_cpu(
            [scene[0]], [scene[1]], [scene[2]])


def test_cifdet_is_refused_by_name():
    for cls in (encoder.CifDet, encoder.AnnRescalerDet):
        with pytest.raises(NotImplementedError, match='CifDet encoder'):
            cls(8, 80)


# ---- the Python mirrors -------------------------------------------------------------------

def test_mirrors_have_the_reference_attributes():
    """encoder/cif.py:15-26, caf.py:16-33, annrescaler.py:9-26."""
    def fields(cls):
        return [(f.name, f.default) for f in dataclasses.fields(cls)]
    missing = dataclasses.MISSING
    assert fields(encoder.Cif) == [('rescaler', missing), ('sigmas', missing),
                                   ('v_threshold', 0), ('visualizer', None)]
    assert (encoder.Cif.side_length, encoder.Cif.padding) == (4, 10)
    assert fields(encoder.Caf) == [
        ('rescaler', missing), ('skeleton', missing), ('sigmas', missing),
        ('sparse_skeleton', None), ('dense_to_sparse_radius', 2.0),
        ('only_in_field_of_view', False), ('v_threshold', 0), ('visualizer', None)]
    assert (encoder.Caf.min_size, encoder.Caf.fixed_size, encoder.Caf.aspect_ratio,
            encoder.Caf.padding) == (3, False, 0.0, 10)
    r = encoder.AnnRescaler(8, 17, np.array(eu.load_fixture('two')['pose']))
    assert sorted(vars(r)) == ['n_keypoints', 'pose', 'pose_45', 'pose_45_total_area',
                               'pose_total_area', 'stride']
    assert (r.stride, r.n_keypoints) == (8, 17)


def test_struct_layout_matches_header(tmp_path):
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include')
    src = tmp_path / 'enc_layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pp_enc_image),
         offsetof(pp_enc_image, valid_area), offsetof(pp_enc_image, ann0), sizeof(pp_enc_ann),
         offsetof(pp_enc_ann, flags), sizeof(pp_encoder), offsetof(pp_encoder, v_threshold),
         offsetof(pp_encoder, fixed_size));
  return 0;
}
''')
    exe = tmp_path / 'enc_layout'
    subprocess.check_call(['gcc', '-I', header, str(src), '-o', str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    im, an = _abi.ENC_IMAGE_DTYPE, _abi.ENC_ANN_DTYPE
    assert vals == [im.itemsize, im.fields['valid_area'][1], im.fields['ann0'][1], an.itemsize,
                    an.fields['flags'][1], ctypes.sizeof(_abi.Encoder),
                    _abi.Encoder.v_threshold.offset, _abi.Encoder.fixed_size.offset]


# ---- batches ------------------------------------------------------------------------------

def _scenes(names):
    return [eu.fixture_scene(eu.load_fixture(n)) for n in names]


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_batch_equals_its_images_alone(which):
    """Equal sizes stack to (B, ...); mixed sizes give per-image tuples; both hold what each
    image gives alone (the fixtures' tensors), on one and on four threads."""
    fx = eu.load_fixture('two')
    cif, caf = eu.encoders(eu.fixture_case(fx), 8)
    enc = cif if which == 'cif' else caf
    names = ('two', 'overlap', 'border', 'few', 'empty', 'crowd_only')
    scenes = _scenes(names)
    for threads in (1, 4):
        got = enc.batch_cpu([s[0] for s in scenes], [s[1] for s in scenes],
                            [s[2] for s in scenes], n_threads=threads)
        assert isinstance(got, tuple)
        for i, name in enumerate(names):
            for g, e in zip(got, eu.expected(eu.load_fixture(name), which, 8)):
                assert g.shape[0] == len(names) and eu.same_bits(g[i], e)
    mixed = ('two', 'tiny', 'empty')
    scenes = _scenes(mixed)
    got = enc.batch_cpu([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes])
    assert isinstance(got, list) and len(got) == 3
    for per_image, name in zip(got, mixed):
        for g, e in zip(per_image, eu.expected(eu.load_fixture(name), which, 8)):
            assert eu.same_bits(g, e)
    assert enc.batch_cpu([], [], []) == []


def test_annotations_are_not_modified():
    fx = eu.load_fixture('overlap')
    cif, caf = eu.encoders(eu.fixture_case(fx), 4)
    size, anns, meta = eu.fixture_scene(fx)
    before = copy.deepcopy((anns, meta))
    cif.batch_cpu([size], [anns], [meta])
    caf.batch_cpu([np.zeros((3,) + size, np.float32)], [anns], [meta])
    for a, b in zip(anns, before[0]):
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(meta['valid_area'], before[1]['valid_area']) if meta else not before[1]


def test_python_refuses_what_it_cannot_marshal():
    fx = eu.load_fixture('two')
    cif, _ = eu.encoders(eu.fixture_case(fx), 8)
    size, anns, meta = eu.fixture_scene(fx)
    anns[0]['keypoints'] = anns[0]['keypoints'].astype(np.float64)
    with pytest.raises(NotImplementedError, match='float32'):
        cif.batch_cpu([size], [anns], [meta])
    with pytest.raises(ValueError):
        cif.batch_cpu([size], [anns, anns], [meta])
