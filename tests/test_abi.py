"""The C-ABI library loads and exports every symbol include/pifpaf_amd.h declares, and the
record layouts the Python side assumes match the C structs.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from openpifpaf_amd import _abi, _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(REPO, 'include', 'pifpaf_amd.h')


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(pp_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    from openpifpaf_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_every_declared_symbol_exported(lib):
    names = declared_functions()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    # and the ctypes table covers every declaration
    assert set(names) == set(_lib.EXPORTED), set(names) ^ set(_lib.EXPORTED)


def test_version_and_defaults(lib):
    assert lib.pp_version() == _abi.PP_ABI_VERSION
    cfg = _abi.PPConfig()
    lib.pp_default_config(ctypes.byref(cfg))
    ref = _abi.make_config()
    for name, typ in _abi.PPConfig._fields_:
        if issubclass(typ, ctypes._Pointer):  # confidence_scales: NULL in both
            assert not getattr(cfg, name) and not getattr(ref, name), name
            continue
        assert getattr(cfg, name) == pytest.approx(getattr(ref, name)), name


def test_pitch_and_workspace_sizes(lib):
    assert lib.pp_cifhr_pitch(633) == 640
    assert lib.pp_cifhr_pitch(1273) == 1280
    assert lib.pp_cifhr_pitch(641) == 672
    cfg = _abi.make_config()
    size = lib.pp_decode_workspace_size(256, 17, 19, 80, 80, ctypes.byref(cfg), 800)
    zoff = lib.pp_decode_workspace_zero_offset(256, 17, 19, 80, 80, ctypes.byref(cfg), 800)
    assert 0 < zoff < size
    assert lib.pp_decode_workspace_size(0, 17, 19, 80, 80, ctypes.byref(cfg), 800) >= 0
    assert lib.pp_decode_workspace_size(1, 0, 19, 80, 80, ctypes.byref(cfg), 800) == 0


def test_argument_errors_without_gpu(lib):
    cfg = _abi.make_config()
    rc = lib.pp_cifhr(None, 1, 17, 8, 8, ctypes.byref(cfg), None, None, 0, None)
    assert rc == -1
    assert b'NULL' in lib.pp_last_error()
    dummy = ctypes.c_void_p(16)
    rc = lib.pp_cifhr(dummy, 1, 0, 8, 8, ctypes.byref(cfg), dummy, dummy, 1 << 20, None)
    assert rc == -2


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pp_ann), offsetof(pp_ann, score),
         offsetof(pp_ann, decoding_pairs), offsetof(pp_ann, decoding_xyv),
         offsetof(pp_ann, frontier_pairs), sizeof(pp_seed), sizeof(pp_config),
         offsetof(pp_ann, n_frontier), offsetof(pp_config, exp_mode));
  return 0;
}
''')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    d = _abi.ANN_DTYPE
    assert vals == [d.itemsize, d.fields['score'][1], d.fields['decoding_pairs'][1],
                    d.fields['decoding_xyv'][1], d.fields['frontier_pairs'][1],
                    _abi.SEED_DTYPE.itemsize, ctypes.sizeof(_abi.PPConfig),
                    d.fields['n_frontier'][1], _abi.PPConfig.exp_mode.offset]


def test_no_oracle_in_product():
    """The product package never imports or links the oracle (test infrastructure)."""
    pkg = os.path.join(REPO, 'openpifpaf_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.hpp', '.cpp')):
                text = open(os.path.join(root, f)).read()
                assert 'oracle' not in text.replace('Oracle', '').lower() or f == 'build.py', f


def test_det_struct_layout_matches_header(tmp_path):
    src = tmp_path / 'det_layout.c'
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "pifpaf_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pp_det), offsetof(pp_det, score),
         offsetof(pp_det, bbox), offsetof(pp_det, image), sizeof(pp_det_nms),
         offsetof(pp_det_nms, apply));
  return 0;
}
''')
    exe = tmp_path / 'det_layout'
    subprocess.check_call(['gcc', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    d = _abi.DET_DTYPE
    assert vals == [d.itemsize, d.fields['score'][1], d.fields['bbox'][1], d.fields['image'][1],
                    ctypes.sizeof(_abi.DetNms), _abi.DetNms.apply.offset]


def test_scale_struct_and_multi_workspace():
    """pp_scale layout and the host-only multi-scale sizing entry points (no GPU needed)."""
    import ctypes
    from openpifpaf_amd._abi import ROLE_CAF, ROLE_CIF, Scale, make_config, scale_list
    from openpifpaf_amd._lib import load
    assert ctypes.sizeof(Scale) == 48
    lib = load()
    cfg = make_config()
    arr = scale_list([(0, 41, 41), (0, 21, 21)], [(0, 41, 41), (0, 21, 21)], [8, 16], [8, 16],
                     [0.0, 12.0], [0.0, 36.0], [160.0, None])
    assert [s.role for s in arr] == [ROLE_CIF, ROLE_CIF, ROLE_CAF, ROLE_CAF]
    size = lib.pp_decode_multi_workspace_size(arr, 4, 0, 2, 17, 19, ctypes.byref(cfg), 128)
    zero = lib.pp_decode_multi_workspace_zero_offset(arr, 4, 0, 2, 17, 19, ctypes.byref(cfg), 128)
    assert 0 < zero < size
    # one CIF + one CAF head of the single-scale shape sizes like pp_decode_workspace_size
    one = scale_list([(0, 41, 41)], [(0, 41, 41)], [8], [8])
    assert (lib.pp_decode_multi_workspace_size(one, 2, 0, 2, 17, 19, ctypes.byref(cfg), 128)
            == lib.pp_decode_workspace_size(2, 17, 19, 41, 41, ctypes.byref(cfg), 128))
    # ... and puts its working records at the same place (pp_decode_initial into a
    # single-scale engine workspace; CifCaf reads NMS-dropped initial annotations there)
    work = lib.pp_decode_work_offset(2, 17, 19, 41, 41, ctypes.byref(cfg), 128)
    assert 0 < work < lib.pp_decode_workspace_size(2, 17, 19, 41, 41, ctypes.byref(cfg), 128)
    assert work == lib.pp_decode_multi_work_offset(one, 2, 0, 2, 17, 19, ctypes.byref(cfg), 128)
    # pairs need an even CIF head count; no CAF head is rejected
    odd = scale_list([(0, 41, 41)] * 3, [(0, 41, 41)], [8] * 3, [8])
    assert lib.pp_decode_multi_workspace_size(odd, 4, 1, 1, 17, 19, ctypes.byref(cfg), 128) == 0
    cif_only = scale_list([(0, 41, 41)], [], [8], [])
    assert lib.pp_decode_multi_workspace_size(cif_only, 1, 0, 1, 17, 19, ctypes.byref(cfg), 128) == 0
    assert lib.pp_cifhr_multi_workspace_size(cif_only, 1, 0, 1, 17) > 0


def _workspace_grid(lib):
    """(workspace size, zero offset, work offset) of the single-scale and of the multi-scale
    sizing entry points over a grid of shapes, K = 17, C = 19."""
    import ctypes
    from openpifpaf_amd._abi import make_config, scale_list
    arr = scale_list([(0, 41, 41), (0, 21, 21)], [(0, 41, 41), (0, 21, 21)], [8, 16], [8, 16],
                     [0.0, 12.0], [0.0, 36.0], [160.0, None])
    single, multi = [], []
    for fc in (True, False):
        cfg = ctypes.byref(make_config(force_complete=fc))
        for n_img in (0, 1, 2, 256):
            for cap in (128, 800):
                for hw in (41, 80):
                    single.append((lib.pp_decode_workspace_size(n_img, 17, 19, hw, hw, cfg, cap),
                                   lib.pp_decode_workspace_zero_offset(n_img, 17, 19, hw, hw, cfg, cap),
                                   lib.pp_decode_work_offset(n_img, 17, 19, hw, hw, cfg, cap)))
                multi.append((lib.pp_decode_multi_workspace_size(arr, 4, 0, n_img, 17, 19, cfg, cap),
                              lib.pp_decode_multi_workspace_zero_offset(arr, 4, 0, n_img, 17, 19, cfg, cap),
                              lib.pp_decode_multi_work_offset(arr, 4, 0, n_img, 17, 19, cfg, cap)))
    return single, multi


def test_workspace_layout_pinned(lib):
    """The six workspace size / offset entry points return what they returned before they were
    folded onto one helper (recorded from that build): force_complete on then off, n_img 0, 1,
    2, 256, ann_capacity 128, 800, fields 41x41 and 80x80 (single) or the 4-head pp_scale
    array of test_scale_struct_and_multi_workspace (multi)."""
    single, multi = _workspace_grid(lib)
    assert single == WORKSPACE_SINGLE
    assert multi == WORKSPACE_MULTI


WORKSPACE_SINGLE = [
    (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
    (218801920, 217619968, 218499328), (633435648, 630626048, 633133056),
    (220136192, 217619968, 218636544), (634769920, 630626048, 633270272),
    (233600768, 231237632, 232996096), (677782272, 672163840, 677177600),
    (236269056, 231237632, 233270272), (680450560, 672163840, 677451776),
    (4660591616, 4358154240, 4583205888), (13867951104, 13148835840, 13790565376),
    (5002132480, 4358154240, 4618300416), (14209491968, 13148835840, 13825659904),
    (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0),
    (218478592, 217296640, 218176000), (632219136, 629409536, 631916544),
    (219812864, 217296640, 218313216), (633553408, 629409536, 632053760),
    (232954624, 230591488, 232349952), (675349504, 669731072, 674744832),
    (235622912, 230591488, 232624128), (678017792, 669731072, 675019008),
    (4577942528, 4275505152, 4500556800), (13556577280, 12837462016, 13479191552),
    (4919483392, 4275505152, 4535651328), (13898118144, 12837462016, 13514286080)]
WORKSPACE_MULTI = [
    (0, 0, 0), (0, 0, 0),
    (95188736, 94006784, 94886144), (96523008, 94006784, 95023360),
    (121112832, 118749696, 120508160), (123781120, 118749696, 120782336),
    (8392452096, 8090014720, 8315066368), (8733992960, 8090014720, 8350160896),
    (0, 0, 0), (0, 0, 0),
    (94798592, 93616640, 94496000), (96132864, 93616640, 94633216),
    (120332800, 117969664, 119728128), (123001088, 117969664, 120002304),
    (8292642816, 7990205440, 8215257088), (8634183680, 7990205440, 8250351616)]


def _decode_refusal_calls():
    """[(label, entry point, arguments)]: bad calls to the five decode entry points.  Device
    pointers are a dummy non-NULL value and workspace_bytes is 16 throughout, so that a call
    whose own check were lost would still stop at `workspace too small`, before any HIP call."""
    from openpifpaf_amd import constants
    from openpifpaf_amd._abi import make_config, scale_list, skeleton_array
    p = ctypes.c_void_p(16)
    coco = skeleton_array(constants.COCO_PERSON_SKELETON)
    keep = []  # what the argument lists point to

    def ptr(arr):
        keep.append(arr)
        return arr.ctypes.data_as(ctypes.c_void_p)

    def cfg(**kw):
        raw = {key: kw.pop(key) for key in ('connection_method', 'occupancy_reduction')
               if key in kw}
        c = make_config(**kw)
        for key, v in raw.items():
            setattr(c, key, v)
        keep.append(c)
        return ctypes.byref(c)

    def stages(cif=p, caf=p, n=1, k=17, c=19, h=8, w=8, skel=coco, config=None, cap=8, ws=p,
               size=16):
        return [cif, caf, n, k, c, h, w, None if skel is None else ptr(skel), config or cfg(),
                None, p, cap, p, p, ws, ctypes.c_size_t(size), ctypes.c_uint32(15), None]

    def batch(**kw):
        a = stages(**kw)
        return a[:16] + a[17:]

    def ragged(extents=((8, 8),), d_extents=p, hr=None, **kw):
        a = stages(**kw)
        return (a[:7] + [d_extents, ptr(np.asarray(extents, np.int32))] + a[7:9] + [hr] +
                a[10:])

    one = scale_list([(16, 8, 8)], [(16, 8, 8)], [8], [8])
    odd = scale_list([(16, 8, 8)] * 3, [(16, 8, 8)], [8] * 3, [8])
    no_cif = scale_list([(0, 8, 8)], [(16, 8, 8)], [8], [8])
    keep.extend([one, odd, no_cif])

    def multi(arr=one, pairs=0, n=1, k=17, c=19, skel=coco, config=None, cap=8, size=16):
        return [arr, len(arr), pairs, n, k, c, ptr(skel), config or cfg(), None, p, cap, p, p, p,
                ctypes.c_size_t(size), ctypes.c_uint32(15), None]

    def initial(init=p, init_counts=p, init_cap=4, **kw):
        a = multi(**kw)
        return a[:13] + [init, init_counts, init_cap, None] + a[13:]

    wide = np.tile(np.array([[1, 2]], np.int32), (65, 1))
    bad_joint = coco.copy()
    bad_joint[18, 1] = 18
    calls = [
        ('stages K=25', 'pp_decode_stages', stages(k=25)),
        ('stages C=65', 'pp_decode_stages', stages(c=65, skel=wide)),
        ('stages ann_capacity=0', 'pp_decode_stages', stages(cap=0)),
        ('stages occupancy_reduction=0', 'pp_decode_stages',
         stages(config=cfg(occupancy_reduction=0))),
        ('stages skeleton index K+1', 'pp_decode_stages', stages(skel=bad_joint)),
        ('stages NULL cif', 'pp_decode_stages', stages(cif=None)),
        ('stages NULL workspace', 'pp_decode_stages', stages(ws=None)),
        ('stages H=0', 'pp_decode_stages', stages(h=0)),
        ('stages connection_method=2', 'pp_decode_stages',
         stages(config=cfg(connection_method=2))),
        ('stages workspace_bytes=16', 'pp_decode_stages', stages()),
        ('stages n_img=0', 'pp_decode_stages', stages(n=0)),
        ('stages n_img=-1', 'pp_decode_stages', stages(n=-1)),
        ('stages K=25 and NULL skeleton', 'pp_decode_stages', stages(k=25, skel=None)),
        ('stages K=25 and connection_method=2', 'pp_decode_stages',
         stages(k=25, config=cfg(connection_method=2))),
        ('batch C=65', 'pp_decode_batch', batch(c=65, skel=wide)),
        ('batch NULL caf', 'pp_decode_batch', batch(caf=None)),
        ('batch workspace_bytes=16', 'pp_decode_batch', batch()),
        ('batch n_img=0', 'pp_decode_batch', batch(n=0)),
        ('multi odd heads in pairs', 'pp_decode_multi', multi(arr=odd, pairs=1)),
        ('multi NULL CIF field', 'pp_decode_multi', multi(arr=no_cif)),
        ('multi K=25', 'pp_decode_multi', multi(k=25)),
        ('multi skeleton index K+1', 'pp_decode_multi', multi(skel=bad_joint)),
        ('multi workspace_bytes=16', 'pp_decode_multi', multi()),
        ('multi n_img=0', 'pp_decode_multi', multi(n=0)),
        ('initial odd heads in pairs', 'pp_decode_initial', initial(arr=odd, pairs=1)),
        ('initial without counts', 'pp_decode_initial', initial(init_counts=None)),
        ('initial counts alone', 'pp_decode_initial', initial(init=None)),
        ('initial_capacity=0', 'pp_decode_initial', initial(init_cap=0)),
        ('initial C=65', 'pp_decode_initial', initial(c=65, skel=wide)),
        ('initial workspace_bytes=16', 'pp_decode_initial', initial()),
        ('initial n_img=0', 'pp_decode_initial', initial(n=0)),
        ('ragged NULL extents', 'pp_decode_ragged', ragged(d_extents=None)),
        ('ragged d_cifhr', 'pp_decode_ragged', ragged(hr=p)),
        ('ragged H=0', 'pp_decode_ragged', ragged(h=0)),
        ('ragged negative threshold', 'pp_decode_ragged',
         ragged(config=cfg(caf_threshold=-0.5))),
        ('ragged extent outside', 'pp_decode_ragged', ragged(extents=((8, 9),))),
        ('ragged extent 0', 'pp_decode_ragged', ragged(extents=((8, 8), (0, 3)), n=2)),
        ('ragged K=25', 'pp_decode_ragged', ragged(k=25)),
        ('ragged workspace_bytes=16', 'pp_decode_ragged', ragged()),
        ('ragged n_img=0', 'pp_decode_ragged', ragged(n=0, extents=((8, 8),))),
    ]
    return calls, keep


def _decode_refusals(lib):
    """(label, status, pp_last_error() or None for PP_OK) of every _decode_refusal_calls entry"""
    calls, keep = _decode_refusal_calls()
    out = []
    for label, name, args in calls:
        rc = getattr(lib, name)(*args)
        out.append((label, rc, lib.pp_last_error().decode() if rc else None))
    del keep
    return out


def test_decode_refusals_pinned(lib):
    """Every refusal of the five decode entry points, with its status and message as recorded
    from the library before decode_heads' checks became check_decode: the same checks in the
    same order (two cases trip two checks at once), the messages byte for byte (they name
    pp_decode_batch whichever entry point was called).  Every refusal happens before any HIP
    call, so no GPU is needed; an empty batch is PP_OK."""
    got = _decode_refusals(lib)
    assert [g[0] for g in got] == [r[0] for r in DECODE_REFUSALS]
    for g, want in zip(got, DECODE_REFUSALS):
        assert g == want


_ENVELOPE = ('pp_decode_batch: shape outside the supported envelope '
             '(K <= PP_MAX_KP, C <= PP_MAX_EDGES)')
DECODE_REFUSALS = [
    ('stages K=25', -2, _ENVELOPE),
    ('stages C=65', -2, _ENVELOPE),
    ('stages ann_capacity=0', -2, _ENVELOPE),
    ('stages occupancy_reduction=0', -2, _ENVELOPE),
    ('stages skeleton index K+1', -1, 'pp_decode_batch: skeleton joint index out of 1..K'),
    ('stages NULL cif', -1, 'pp_decode_batch: NULL argument'),
    ('stages NULL workspace', -1, 'pp_decode_batch: NULL argument'),
    ('stages H=0', -2, 'pp_decode_batch: bad shape'),
    ('stages connection_method=2', -1, 'connection method not known'),
    ('stages workspace_bytes=16', -5, 'pp_decode_batch: workspace too small'),
    ('stages n_img=0', 0, None),
    ('stages n_img=-1', -2, _ENVELOPE),
    ('stages K=25 and NULL skeleton', -1, 'pp_decode_batch: NULL argument'),
    ('stages K=25 and connection_method=2', -2, _ENVELOPE),
    ('batch C=65', -2, _ENVELOPE),
    ('batch NULL caf', -1, 'pp_decode_batch: NULL argument'),
    ('batch workspace_bytes=16', -5, 'pp_decode_batch: workspace too small'),
    ('batch n_img=0', 0, None),
    ('multi odd heads in pairs', -2,
     'pp_decode_multi: CIF head count is not a multiple of the CifHr group size'),
    ('multi NULL CIF field', -1, 'pp_decode_batch: NULL CIF field'),
    ('multi K=25', -2, _ENVELOPE),
    ('multi skeleton index K+1', -1, 'pp_decode_batch: skeleton joint index out of 1..K'),
    ('multi workspace_bytes=16', -5, 'pp_decode_batch: workspace too small'),
    ('multi n_img=0', 0, None),
    ('initial odd heads in pairs', -2,
     'pp_decode_initial: CIF head count is not a multiple of the CifHr group size'),
    ('initial without counts', -1, 'pp_decode_initial: d_initial and d_initial_counts go together'),
    ('initial counts alone', -1, 'pp_decode_initial: d_initial and d_initial_counts go together'),
    ('initial_capacity=0', -2, 'pp_decode_initial: bad initial_capacity'),
    ('initial C=65', -2, _ENVELOPE),
    ('initial workspace_bytes=16', -5, 'pp_decode_batch: workspace too small'),
    ('initial n_img=0', 0, None),
    ('ragged NULL extents', -1, 'pp_decode_ragged: NULL argument'),
    ('ragged d_cifhr', -1,
     'pp_decode_ragged: the dense CifHr map of a ragged batch has no layout '
     '(d_cifhr must be NULL)'),
    ('ragged H=0', -2, 'pp_decode_ragged: bad shape'),
    ('ragged negative threshold', -1, 'pp_decode_ragged: a ragged batch needs thresholds >= 0'),
    ('ragged extent outside', -2, 'pp_decode_ragged: extent outside the container'),
    ('ragged extent 0', -2, 'pp_decode_ragged: extent outside the container'),
    ('ragged K=25', -2, _ENVELOPE),
    ('ragged workspace_bytes=16', -5, 'pp_decode_batch: workspace too small'),
    ('ragged n_img=0', 0, None),
]


def test_packed_record_size_matches_python_layout():
    """pp_packed_record_size (a host function) agrees with _abi.packed_dtype for every flag
    set, COCO and dense skeletons; compact records are at least 2x smaller than pp_ann."""
    from openpifpaf_amd._abi import ANN_DTYPE, packed_dtype
    lib = _lib.load()
    for k, c in ((17, 19), (17, 44), (24, 64), (1, 1), (5, 3)):
        for flags in (0, 1, 2, 3):
            assert lib.pp_packed_record_size(k, c, flags) == packed_dtype(k, c, flags).itemsize
            assert packed_dtype(k, c, flags).itemsize % 16 == 0
    assert lib.pp_packed_record_size(0, 19, 3) == 0 and lib.pp_packed_record_size(17, 65, 3) == 0
    assert 2 * packed_dtype(17, 19, 3).itemsize < ANN_DTYPE.itemsize


def _handover_refusal_calls():
    """[(label, entry point, arguments)]: bad calls to the in-place inverse, the record packing
    and the COCO record entry points.  Device pointers are a dummy non-NULL value; every case
    stops at an argument check (or at the empty batch), before any HIP call."""
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(17)
    params, none = _abi.CocoParams(0.0, 20, 1), _abi.CocoParams(0.0, 0, 1)

    def inverse(anns=p, n=1, cap=8, k=17, flags=p):
        return [anns, p, n, cap, k, p, None, flags, None]

    def dets(metas=p, n=1, cap=8):
        return [p, p, n, cap, metas, None]

    def records(out=p, n=1, cap=8, out_cap=8):
        return [p, p, n, cap, out, out_cap, p, None]

    def compact(counts=p, n=1, cap=8, k=17, c=19, flags=_abi.PACK_ALL, out_cap=8):
        return [p, counts, n, cap, k, c, ctypes.c_uint32(flags), p, out_cap, p, None, None]

    def coco(det, ids=p, n=1, cap=8, k=17, par=params, out=p, ws=p):
        head = [p, p, n, cap] + ([] if det else [k]) + [p, ids] + ([] if det else [None])
        return head + [ctypes.byref(par), out, 8, p, p, ws, None]

    calls = [
        ('inverse NULL anns', 'pp_annotations_inverse', inverse(anns=None)),
        ('inverse NULL nan_flags', 'pp_annotations_inverse', inverse(flags=None)),
        ('inverse n_img=-1', 'pp_annotations_inverse', inverse(n=-1)),
        ('inverse capacity=0', 'pp_annotations_inverse', inverse(cap=0)),
        ('inverse K=0', 'pp_annotations_inverse', inverse(k=0)),
        ('inverse K=25', 'pp_annotations_inverse', inverse(k=25)),
        ('inverse n_img=0', 'pp_annotations_inverse', inverse(n=0)),
        ('dets NULL metas', 'pp_dets_inverse', dets(metas=None)),
        ('dets n_img=-1', 'pp_dets_inverse', dets(n=-1)),
        ('dets capacity=0', 'pp_dets_inverse', dets(cap=0)),
        ('dets n_img=0', 'pp_dets_inverse', dets(n=0)),
        ('records NULL out', 'pp_pack_records', records(out=None)),
        ('records n_img=-1', 'pp_pack_records', records(n=-1)),
        ('records capacity=0', 'pp_pack_records', records(cap=0)),
        ('records out_capacity=-1', 'pp_pack_records', records(out_cap=-1)),
        ('records n_img=0', 'pp_pack_records', records(n=0)),
        ('compact NULL counts', 'pp_pack_compact', compact(counts=None)),
        ('compact n_img=-1', 'pp_pack_compact', compact(n=-1)),
        ('compact capacity=0', 'pp_pack_compact', compact(cap=0)),
        ('compact K=0', 'pp_pack_compact', compact(k=0)),
        ('compact K=25', 'pp_pack_compact', compact(k=25)),
        ('compact C=65', 'pp_pack_compact', compact(c=65)),
        ('compact unknown flag', 'pp_pack_compact', compact(flags=4)),
        ('compact unknown flag and K=25', 'pp_pack_compact', compact(flags=4, k=25)),
        ('compact n_img=0', 'pp_pack_compact', compact(n=0)),
    ]
    for name, det in (('pp_coco_keypoints', False), ('pp_coco_dets', True)):
        tag = 'coco dets' if det else 'coco keypoints'
        calls += [
            (tag + ' NULL image_ids', name, coco(det, ids=None)),
            (tag + ' n_img=-1', name, coco(det, n=-1)),
            (tag + ' capacity=0', name, coco(det, cap=0)),
            (tag + ' max_per_image=0', name, coco(det, par=none)),
            (tag + ' NULL workspace', name, coco(det, ws=None)),
            (tag + ' odd out', name, coco(det, out=odd)),
            (tag + ' odd out and n_img=0', name, coco(det, out=odd, n=0)),
            (tag + ' n_img=0', name, coco(det, n=0)),
        ]
    calls += [('coco keypoints K=0', 'pp_coco_keypoints', coco(False, k=0)),
              ('coco keypoints K=25', 'pp_coco_keypoints', coco(False, k=25))]
    return calls, [params, none]


def _handover_refusals(lib):
    calls, keep = _handover_refusal_calls()
    out = []
    for label, name, args in calls:
        rc = getattr(lib, name)(*args)
        out.append((label, rc, lib.pp_last_error().decode() if rc else None))
    del keep
    return out


def test_handover_refusals_pinned(lib):
    """Every argument refusal of pp_annotations_inverse, pp_dets_inverse, pp_pack_records,
    pp_pack_compact, pp_coco_keypoints and pp_coco_dets, with its status and message as
    recorded from the library before inverse.hip was cut into inverse.hpp, pack.hip and
    pack_common.hpp: NULL arguments, n_img < 0, capacity 0, K 0 and 25, C 65, an unknown pack
    flag, max_per_image 0, a NULL workspace, an odd `out` address.  Every refusal happens
    before any HIP call, so no GPU is needed; an empty batch is PP_OK."""
    got = _handover_refusals(lib)
    assert [g[0] for g in got] == [r[0] for r in HANDOVER_REFUSALS]
    for g, want in zip(got, HANDOVER_REFUSALS):
        assert g == want


HANDOVER_REFUSALS = [
    ('inverse NULL anns', -1, 'pp_annotations_inverse: NULL argument'),
    ('inverse NULL nan_flags', -1, 'pp_annotations_inverse: NULL argument'),
    ('inverse n_img=-1', -2, 'pp_annotations_inverse: bad shape'),
    ('inverse capacity=0', -2, 'pp_annotations_inverse: bad shape'),
    ('inverse K=0', -2, 'pp_annotations_inverse: bad shape'),
    ('inverse K=25', -2, 'pp_annotations_inverse: bad shape'),
    ('inverse n_img=0', 0, None),
    ('dets NULL metas', -1, 'pp_dets_inverse: NULL argument'),
    ('dets n_img=-1', -2, 'pp_dets_inverse: bad shape'),
    ('dets capacity=0', -2, 'pp_dets_inverse: bad shape'),
    ('dets n_img=0', 0, None),
    ('records NULL out', -1, 'pp_pack_records: NULL argument'),
    ('records n_img=-1', -2, 'pp_pack_records: bad shape'),
    ('records capacity=0', -2, 'pp_pack_records: bad shape'),
    ('records out_capacity=-1', -2, 'pp_pack_records: bad shape'),
    ('records n_img=0', 0, None),
    ('compact NULL counts', -1, 'pp_pack_compact: NULL argument'),
    ('compact n_img=-1', -2, 'pp_pack_compact: bad shape'),
    ('compact capacity=0', -2, 'pp_pack_compact: bad shape'),
    ('compact K=0', -2, 'pp_pack_compact: bad shape'),
    ('compact K=25', -2, 'pp_pack_compact: bad shape'),
    ('compact C=65', -2, 'pp_pack_compact: bad shape'),
    ('compact unknown flag', -1, 'pp_pack_compact: unknown flag'),
    ('compact unknown flag and K=25', -2, 'pp_pack_compact: bad shape'),
    ('compact n_img=0', 0, None),
]
for _who in ('pp_coco_keypoints', 'pp_coco_dets'):
    _tag = 'coco dets' if _who == 'pp_coco_dets' else 'coco keypoints'
    HANDOVER_REFUSALS += [
        (_tag + ' NULL image_ids', -1, _who + ': NULL argument'),
        (_tag + ' n_img=-1', -2, _who + ': bad shape'),
        (_tag + ' capacity=0', -2, _who + ': bad shape'),
        (_tag + ' max_per_image=0', -2, _who + ': max_per_image < 1'),
        (_tag + ' NULL workspace', -1, _who + ': NULL argument'),
        (_tag + ' odd out', -1, _who + ': destination not 8-byte aligned'),
        (_tag + ' odd out and n_img=0', -1, _who + ': destination not 8-byte aligned'),
        (_tag + ' n_img=0', 0, None),
    ]
HANDOVER_REFUSALS += [
    ('coco keypoints K=0', -2, 'pp_coco_keypoints: K outside [1, PP_MAX_KP]'),
    ('coco keypoints K=25', -2, 'pp_coco_keypoints: K outside [1, PP_MAX_KP]'),
]
