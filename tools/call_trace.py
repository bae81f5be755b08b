"""Diagnostic: the library calls a fixed script of decodes makes, one line per call.

    python tools/call_trace.py [--out FILE]

openpifpaf_amd._lib.call is replaced by a recorder before anything else of the package is
imported, so every `from ._lib import call` binds it.  A line holds the symbol, every integer
argument and, for a tensor passed by pointer through _device.ptr, `t` and its numel; other
pointers are `p` (`null` when they are), never their value.  The inputs are synthetic with fixed seeds, so the
overflow retries are the same in every run: two trees that make the same calls write the
same file.  Needs the device."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpifpaf_amd import _lib  # noqa: E402

LINES = []
_call = _lib.call


class _Ptr(ctypes.c_void_p):
    numel = None


def _word(a):
    if isinstance(a, ctypes.c_void_p) and not a.value:
        return 'null'
    if isinstance(a, _Ptr):
        return 't{}'.format(a.numel)
    if isinstance(a, bool) or a is None:
        return repr(a)
    if isinstance(a, (int, np.integer)):
        return str(a)
    if isinstance(a, (ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int64)):
        return str(a.value)
    return 'p'


def _recorder(name, *args):
    LINES.append(' '.join([name] + [_word(a) for a in args]))
    return _call(name, *args)


_lib.call = _recorder

from openpifpaf_amd import _device, constants, decoder, synthetic  # noqa: E402
from openpifpaf_amd._abi import EVAL_CONFIG, PACK_ALL, make_config  # noqa: E402
from openpifpaf_amd import engine as E  # noqa: E402
from openpifpaf_amd.eval_coco import metas_device  # noqa: E402


def _ptr(t):
    p = _Ptr(0 if t is None else t.data_ptr())
    p.numel = None if t is None else t.numel()
    return p  # a null pointer stays a null pointer


_device.ptr = _ptr
SKEL = constants.COCO_PERSON_SKELETON
CFG = make_config(**EVAL_CONFIG)


def mark(text):
    LINES.append('# ' + text)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pose_batch(kind, n, h, w, seed):
    kw = {'n_caf': len(SKEL)} if kind == 'uniform' else {'skeleton': SKEL, 'n_people': 4}
    return tuple(dev(a) for a in synthetic.batch(kind, n, h, w, first_seed=seed, **kw))


def multi(sizes, seed):
    """Per-image head lists of the 'ms2' case at the images' pixel sizes, and its FieldConfig."""
    per = [synthetic.multi_case('ms2', seed=seed + i, h_px=s, w_px=s + 16, n_people=3)
           for i, s in enumerate(sizes)]
    return [[dev(f) for f in p[0]] for p in per], decoder.FieldConfig(**per[0][1])


def pose():
    eng = E.DecodeEngine()
    cif, caf = pose_batch('planted', 3, 33, 41, 11)
    mark('pose single-scale, full and compact records')
    recs, offsets, _ = eng.decode(cif, caf, SKEL, CFG)
    eng.decode(cif, caf, SKEL, CFG, compact=PACK_ALL)
    mark('pose cap=1 overflow retry')
    eng.decode(cif, caf, SKEL, CFG, cap=1, compact=PACK_ALL)
    mark('pose InitialAnnotations')
    init = E.InitialAnnotations([recs[offsets[i]:offsets[i] + 1] for i in range(3)],
                                _device.require())
    eng.decode(cif, caf, SKEL, CFG, initial=init)
    mark('pose HeadSet')
    lists, fc = multi([161, 161], 20)
    heads = E.HeadSet([torch.stack([f[j] for f in lists]) for j in range(len(lists[0]))], fc)
    eng.decode(None, None, SKEL, CFG, heads=heads, compact=PACK_ALL)
    eng.decode(None, None, SKEL, CFG, heads=heads, initial=E.InitialAnnotations(
        [recs[:1], recs[:0]], _device.require()))
    mark('pose RaggedFields')
    sizes = [(21, 33), (40, 27), (33, 33)]
    fields = [tuple(dev(a) for a in synthetic.planted(h, w, n_people=3, seed=40 + i))
              for i, (h, w) in enumerate(sizes)]
    eng.decode(None, None, SKEL, CFG, ragged=E.RaggedFields(fields), compact=PACK_ALL)
    mark('pose RaggedHeadSet')
    lists, fc = multi([129, 161, 97], 50)
    eng.decode(None, None, SKEL, CFG, ragged=E.RaggedHeadSet(lists, fc), compact=PACK_ALL)
    mark('decode_async compact, device_out')
    eng.decode_async(cif, caf, SKEL, CFG)[1].result()
    eng.decode_async(cif, caf, SKEL, CFG, device_out=True)[1].result()
    mark('fetch_coco_async')
    b = eng.launch_checked(cif, caf, SKEL, CFG)
    metas = [{'offset': np.array([0.0, 0.0]), 'scale': np.array([1.0, 1.0]), 'hflip': False,
              'width_height': np.array([400, 300]), 'image_id': 7 + i} for i in range(3)]
    d_metas, d_ids, d_swap = metas_device(metas, 17)
    E.DecodeEngine.fetch_coco_async(b, d_metas, d_ids, hswap=d_swap).result()
    mark('DecodePipeline: planted, uniform, planted, uniform')
    pipe = E.DecodePipeline()
    batches = [pose_batch(kind, 4, 40, 40, 100 * i)
               for i, kind in enumerate(('planted', 'uniform', 'planted', 'uniform'))]
    pending = [pipe.submit(c, f, SKEL, CFG, cap=1024, compact=(17, len(SKEL), PACK_ALL))[1]
               for c, f in batches]
    for p in pending:
        p.result()


def det():
    k = 3
    cats = ['c%d' % i for i in range(k)]
    decoder.CifHr.v_threshold = 0.1
    decoder.CifSeeds.threshold = 0.1
    cd = decoder.CifDet(decoder.FieldConfig(), cats)
    batch = dev(synthetic.det_batch('uniform', 4, 13, 17, n_categories=k))
    mark('CifDet decode_records single')
    cd.decode_records(batch)
    mark('CifDet cap=1 overflow retry')
    cd.decode_records(batch, cap=1)
    mark('CifDet decode_device, and at cap=1')
    cd.decode_device(batch)
    cd.decode_device(batch, cap=1)
    mark('CifDet ragged')
    fields = [dev(synthetic.det_uniform(h, w, n_categories=k, seed=60 + i))
              for i, (h, w) in enumerate([(13, 17), (9, 21), (16, 8)])]
    ragged = E.RaggedDetFields(fields)
    cd.decode_ragged_records(ragged)
    cd.decode_ragged_records(ragged, cap=1)
    cd.decode_ragged_device(ragged, cap=1)
    mark('CifDet two heads')
    fc = decoder.FieldConfig(cif_indices=[0, 1], cif_strides=[8, 16], cif_min_scales=[0.0, 2.0])
    two = decoder.CifDet(fc, cats)
    heads = [dev(synthetic.det_batch('uniform', 2, h, w, first_seed=70, n_categories=k))
             for h, w in ((17, 21), (9, 11))]
    two.decode_records(heads)
    two.decode_device(heads, cap=1)
    mark('DetPipeline: four batches')
    pipe = E.DetPipeline()
    pending = [pipe.submit(cd, b) for b in (batch, ragged, batch[:2], ragged)]
    for p in pending:
        p.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    _device.require()
    pose()
    det()
    torch.cuda.synchronize()
    text = '\n'.join(LINES) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == '__main__':
    main()
