"""Eval preprocessing with extended scale, turns and the multi-scale input pyramid on the
device (pp_preprocess_views through EvalViews.batch) against the reference's fixture
(tests/golden/preprocess_views.npz), the host twin and the existing device path
(EvalPreprocess.batch followed by the slicing of network/nets.py:116-128).  All comparisons
are exact; the fixture carries everything the reference contributes."""
import numpy as np
import pytest
import torch

import preprocess_util as pu
import preprocess_views_util as vu
from openpifpaf_amd import constants, eval_coco, preprocess, transforms
from openpifpaf_amd.annotation import Annotation
from openpifpaf_amd.transforms import EvalPreprocess, EvalViews

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cases():
    return vu.load()[1]


def as_input(src, kind):
    return src if kind == 'host' else torch.from_numpy(src.copy()).cuda()


# ---- 1. the device against the fixture --------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', vu.ALL_DTYPES)
def test_batches_equal_reference(cases, dtype, channels_last):
    """Every case, in the batches one object serves (one launch each; host arrays and device
    tensors alternate)."""
    for mode, group in vu.groups(cases).items():
        pp = vu.make(mode, dtype, channels_last)
        images = [as_input(c.src, ('host', 'device')[i % 2]) for i, c in enumerate(group)]
        metas_in = None if group[0].image_id is None else [c.given_meta() for c in group]
        out, metas = pp.batch(images, metas_in)
        for o in out if isinstance(out, list) else [out]:
            assert o.is_cuda and o.dtype == dtype
        for i, c in enumerate(group):
            vu.check_meta(metas[i], c)
            vu.check_image(c, out, i, dtype, channels_last)


# ---- 2. the device against the twin -----------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', vu.ALL_DTYPES)
def test_device_equals_host_twin(dtype, channels_last):
    """12 seeded non-square images at L = 47 (three workgroups per canvas, the last one
    partly past the end), ids 1 to 12, all modes on; every third image a device tensor."""
    rng = np.random.default_rng(13)
    long_edge, images = 47, []
    while len(images) < 12:
        h, w = (int(v) for v in rng.integers(8, 71, 2))
        try:
            ok = h != w and min(preprocess.rescaled_size(h, w, long_edge)) >= 2 and \
                min(preprocess.rescaled_size(h, w, (long_edge - 1) // 2 + 1)) >= 2
        except AssertionError:  # the reference's own: scipy's output size would differ
            continue
        if ok:
            images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    metas_in = [{'image_id': i + 1} for i in range(12)]
    pp = EvalViews(long_edge, extended_scale=True, orientation_invariant=True, multi_scale=True,
                   dtype=dtype, channels_last=channels_last)
    got, metas = pp.batch([as_input(im, 'device' if i % 3 == 0 else 'host')
                           for i, im in enumerate(images)], metas_in)
    want, metas_cpu = pp.batch_cpu(images, metas_in)
    assert len(got) == len(want) == 10
    for v in range(10):
        assert tuple(got[v].shape) == want[v].shape
        assert np.array_equal(pu.bits(vu.as_array(got[v])), pu.bits(vu.as_array(want[v]))), v
    assert {m['rotation']['angle'] for m in metas} == {0.0, 90, 180, 270}
    for a, b in zip(metas, metas_cpu):
        assert a['rotation'] == b['rotation']
        for k in pu.META_KEYS:
            assert np.array_equal(a[k], b[k])


# ---- 3. against the existing device path ------------------------------------------------
@pytest.mark.parametrize('tight', [False, True])
def test_flags_off_equals_eval_preprocess(tight):
    for (long_edge, case_tight), group in pu.groups(pu.load()[1]).items():
        if case_tight != tight:
            continue
        images = [c.src for c in group]
        want, _ = EvalPreprocess(long_edge, tight_padding=tight).batch(images)
        got, _ = EvalViews(long_edge, tight_padding=tight).batch(images)
        if not tight:
            want, got = [want], [got]
        assert len(want) == len(got)
        for w, g in zip(want, got):
            assert g.shape == w.shape and g.stride() == w.stride()
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))


def reduce_torch(x, hflip=True):
    """nets.py:116-128 on a (B, 3, n, n) tensor (bool masks for the ByteTensor ones)."""
    out = []
    for flip in ([False, True] if hflip else [False]):
        for reduction in [1, 1.5, 2, 3, 5]:
            if reduction == 1.5:
                x_red = torch.tensor([i % 3 != 2 for i in range(x.shape[3])], device=x.device)
                y_red = torch.tensor([i % 3 != 2 for i in range(x.shape[2])], device=x.device)
                reduced = x[:, :, y_red, :]
                reduced = reduced[:, :, :, x_red]
            else:
                reduced = x[:, :, ::reduction, ::reduction]
            if flip:
                reduced = torch.flip(reduced, dims=[3])
            out.append(reduced)
    return out


@pytest.mark.parametrize('dtype, channels_last', [(torch.float32, False), (torch.bfloat16, True)])
def test_workload_size_equals_sliced_eval_preprocess(dtype, channels_last):
    """480x640 and 427x640 at L = 641 (the workload's size: 402 workgroups per canvas,
    L mod 3 = 2): every view is the slicing and flip of EvalPreprocess.batch's tensor."""
    rng = np.random.default_rng(17)
    images = [torch.from_numpy(rng.integers(0, 256, (h, 640, 3), dtype=np.uint8)).cuda()
              for h in (480, 427)]
    base, _ = EvalPreprocess(641, dtype=dtype, channels_last=channels_last).batch(images)
    want = reduce_torch(base)
    got, _ = EvalViews(641, multi_scale=True, dtype=dtype, channels_last=channels_last).batch(images)
    assert [tuple(g.shape) for g in got] == [(2, 3, s, s) for s in (641, 428, 321, 214, 129)] * 2
    view = torch.int32 if dtype == torch.float32 else torch.int16
    for v, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and vu.is_channels_last(g) == channels_last, v
        assert torch.equal(g.contiguous().view(view), w.contiguous().view(view)), v


# ---- 4. buffer reuse --------------------------------------------------------------------
def test_consecutive_batches_reuse_and_fresh(cases):
    pyr = {c.long_edge: c for c in cases if c.ms and not c.ori}
    c = pyr[33]
    pp = vu.make(c)
    big, _ = pp.batch([c.src] * 5)
    for i in range(5):
        vu.check_image(c, big, i, torch.float32, False)
    ptr = pp._out.data_ptr()
    small, _ = pp.batch([c.src])  # a second, smaller call on the same object
    assert pp._out.data_ptr() == ptr and small[0].data_ptr() == ptr
    assert [tuple(v.shape) for v in small] == [(1,) + a.shape for a in c.views]
    vu.check_image(c, small, 0, torch.float32, False)
    kept, _ = pp.batch([c.src] * 2, fresh=True)
    saved = [k.clone() for k in kept]
    again, _ = pp.batch([c.src[::-1].copy()] * 3)
    assert all(k.data_ptr() != a.data_ptr() for k in kept for a in again)
    assert not torch.equal(again[0][0], kept[0][0])
    for k, s in zip(kept, saved):
        assert torch.equal(k, s)
    for i in range(2):
        vu.check_image(c, kept, i, torch.float32, False)


def test_call_has_the_reference_signature(cases):
    fx = vu.load()[0]
    edge, image_id = int(fx['anns_long_edge']), int(fx['anns_image_id'])
    src = fx['s%d_src' % edge]
    anns = [{'keypoints': fx['anns_in_keypoints'][a].reshape(-1).tolist(),
             'bbox': fx['anns_in_bbox'][a].tolist()} for a in range(2)]
    tensor, got, meta = EvalViews(edge, orientation_invariant=True)(src, anns, {'image_id': image_id})
    assert tuple(tensor.shape) == (3, edge, edge) and meta['rotation']['angle'] == 90
    for a in range(2):
        for key in ('keypoints', 'bbox', 'bbox_original'):
            assert got[a][key].tobytes() == fx['anns_turned_' + key][a].tobytes(), key
    c = next(x for x in cases if x.name == 'all_')
    views, _, meta = vu.make(c)(c.src, [], c.given_meta())
    assert [tuple(v.shape) for v in views] == [a.shape for a in c.views]
    vu.check_meta(meta, c)
    vu.check_image(c, [v[None] for v in views], 0, torch.float32, False)


# ---- 5. the inverse on the new metas ----------------------------------------------------
@pytest.mark.parametrize('label, flags', [('turned', dict(orientation_invariant=True)),
                                          ('half', dict(extended_scale=True))])
def test_annotations_inverse_on_the_new_metas(label, flags):
    fx = vu.load()[0]
    edge, image_id = int(fx['anns_long_edge']), int(fx['anns_image_id'])
    _, (meta,) = EvalViews(edge, **flags).batch([fx['s%d_src' % edge]], [{'image_id': image_id}])
    anns = []
    for a in range(2):
        ann = Annotation(constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON)
        ann.data = fx['inv_in_data'][a].copy()
        ann.joint_scales = fx['inv_in_scales'][a].copy()
        ann.decoding_order = [(t, t + 1, fx['inv_in_dxyv'][a, t, :3].copy(),
                               fx['inv_in_dxyv'][a, t, 3:].copy()) for t in range(3)]
        anns.append(ann)
    inv = transforms.Preprocess.annotations_inverse(anns, meta)
    assert pu.bits(np.stack([a.data for a in inv])).tolist() == \
        pu.bits(fx['inv_%s_data' % label].copy()).tolist()
    assert pu.bits(np.stack([a.joint_scales for a in inv])).tolist() == \
        pu.bits(fx['inv_%s_scales' % label].copy()).tolist()
    o = np.zeros_like(fx['inv_in_dxyv'])
    for a, ann in enumerate(inv):
        for t, (_, __, c1, c2) in enumerate(ann.decoding_order):
            o[a, t, :3], o[a, t, 3:] = c1[:3], c2[:3]
    assert pu.bits(o).tolist() == pu.bits(fx['inv_%s_dxyv' % label].copy()).tolist()
    d_metas, d_ids, _ = eval_coco.metas_device([meta])
    assert d_metas.cpu().numpy().tobytes() == transforms.meta_record(meta).tobytes()
    assert d_ids.cpu().tolist() == [image_id]
