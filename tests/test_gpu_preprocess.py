"""Eval preprocessing on the device (pp_preprocess_images through EvalPreprocess.batch) against
the reference's fixture (tests/golden/preprocess.npz) and the host twin.  All comparisons are
exact; the fixture carries everything the reference contributes."""
import numpy as np
import pytest
import torch

import preprocess_util as pu
from openpifpaf_amd import eval_coco, preprocess, transforms
from openpifpaf_amd.transforms import EvalPreprocess

pytestmark = pytest.mark.gpu

ALL_DTYPES = pu.DTYPES + (torch.uint8,)


@pytest.fixture(scope='module')
def cases():
    return pu.load()[1]


def check_case(case, got, dtype, channels_last):
    assert got.is_cuda and got.dtype == dtype
    if dtype == torch.uint8:
        assert tuple(got.shape) == case.u8.shape, case.name
        assert got.cpu().numpy().tobytes() == case.u8.tobytes(), case.name
        return
    assert tuple(got.shape) == (1,) + case.f32.shape, (case.name, tuple(got.shape))
    # a (1, 3, H, W) view of (1, H, W, 3) memory, or plain (1, 3, H, W) memory
    assert got.permute(0, 2, 3, 1).is_contiguous() == channels_last, case.name
    assert got.is_contiguous() != channels_last, case.name
    assert np.array_equal(pu.bits(got), pu.bits(pu.expected(case, dtype))), \
        (case.name, dtype, channels_last)


def as_input(src, kind):
    if kind == 'host':
        return src
    if kind == 'host_tensor':
        return torch.from_numpy(src.copy())
    return torch.from_numpy(src.copy()).cuda()


@pytest.mark.parametrize('kind', ['host', 'device'])
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', ALL_DTYPES)
def test_single_images_equal_reference(cases, dtype, channels_last, kind):
    for c in cases:
        pp = EvalPreprocess(c.long_edge, tight_padding=c.tight, dtype=dtype,
                            channels_last=channels_last)
        out, metas = pp.batch([as_input(c.src, kind)])
        pu.check_meta(metas[0], c)
        check_case(c, pu.one(out, 0, c.tight, dtype), dtype, channels_last)


@pytest.mark.parametrize('kind', ['host', 'device', 'mixed'])
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', ALL_DTYPES)
def test_mixed_batches_equal_reference(cases, dtype, channels_last, kind):
    """Every case that one object serves, in one launch; `mixed`: host arrays, host tensors
    and device tensors side by side."""
    kinds = ('device', 'host', 'host_tensor')
    for (long_edge, tight), group in pu.groups(cases).items():
        pp = EvalPreprocess(long_edge, tight_padding=tight, dtype=dtype,
                            channels_last=channels_last)
        images = [as_input(c.src, kinds[i % 3] if kind == 'mixed' else kind)
                  for i, c in enumerate(group)]
        out, metas = pp.batch(images)
        assert len(out) == len(metas) == len(group)
        for i, c in enumerate(group):
            pu.check_meta(metas[i], c)
            check_case(c, pu.one(out, i, tight, dtype), dtype, channels_last)


@pytest.mark.parametrize('tight', [False, True])
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('dtype', ALL_DTYPES)
def test_device_equals_host_twin(dtype, channels_last, tight):
    """32 seeded images with edges in [2, 70] (several workgroups per image, sizes that are no
    multiple of the workgroup): the device output is the twin's, bit for bit."""
    rng = np.random.default_rng(11)
    long_edge = 61
    images = []
    while len(images) < 32:
        h, w = (int(v) for v in rng.integers(2, 71, 2))
        try:
            if min(preprocess.rescaled_size(h, w, long_edge)) < 2:
                continue
        except AssertionError:  # the reference's own: scipy's output size would differ
            continue
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    pp =EvalPreprocess(long_edge, tight_padding=tight, dtype=dtype, channels_last=channels_last)
    got, metas = pp.batch(images)
    want, metas_cpu = pp.batch_cpu(images)
    assert len(got) == len(want) == 32
    for i in range(32):
        g, w = got[i], want[i]
        assert tuple(g.shape) == w.shape
        assert np.array_equal(pu.bits(g), pu.bits(np.ascontiguousarray(w))), i
        for k in pu.META_KEYS:
            assert np.array_equal(metas[i][k], metas_cpu[i][k])


def test_consecutive_batches_reuse_and_grow(cases):
    """A small batch, a larger one and the small one again on one object: the kept buffers
    and the grown tables serve each; fresh=True results survive the next call."""
    groups = pu.groups(cases)
    group = groups[(26, True)] + groups[(26, True)]
    big = [c for c in cases if c.tight and c.long_edge == 26] * 8
    pp = EvalPreprocess(26, tight_padding=True)
    small = group[:1]
    for batch in (small, big, small):
        out, metas = pp.batch([c.src for c in batch])
        for i, c in enumerate(batch):
            pu.check_meta(metas[i], c)
            check_case(c, out[i], torch.float32, False)
    kept, _ = pp.batch([c.src for c in group], fresh=True)
    ptr = pp._out.data_ptr()
    again, _ = pp.batch([c.src for c in reversed(group)])
    assert pp._out.data_ptr() == ptr and again[0].data_ptr() == ptr  # reused, not reallocated
    assert all(k.data_ptr() != a.data_ptr() for k in kept for a in again)
    for k, c in zip(kept, group):
        check_case(c, k, torch.float32, False)
    for a, c in zip(again, reversed(group)):
        check_case(c, a, torch.float32, False)
    # CenterPad on one object: two batch sizes
    pad_cases = [c for c in cases if not c.tight and c.long_edge == 26]
    pp = EvalPreprocess(26)
    for batch in (pad_cases[:1], pad_cases * 5, pad_cases):
        out, _ = pp.batch([c.src for c in batch])
        assert tuple(out.shape) == (len(batch), 3, 26, 26)
        for i, c in enumerate(batch):
            check_case(c, out[i:i + 1], torch.float32, False)


def test_call_has_the_reference_signature(cases):
    fx = pu.load()[0]
    c = next(x for x in cases if x.name == 'c0_')
    anns = [{'keypoints': fx['anns_in_keypoints'][a].reshape(-1).tolist(),
             'bbox': fx['anns_in_bbox'][a].tolist(), 'segmentation': [[0.0, 1.0]]}
            for a in range(2)]
    pp = EvalPreprocess(c.long_edge, tight_padding=c.tight)
    tensor, got, meta = pp(c.src, anns, {'image_id': 5})
    assert tuple(tensor.shape) == c.f32.shape
    check_case(c, tensor[None], torch.float32, False)
    pu.check_meta(meta, c)
    assert meta['image_id'] == 5
    for a in range(2):
        for key in ('keypoints', 'bbox', 'bbox_original'):
            assert got[a][key].tobytes() == fx['anns_' + key][a].tobytes(), key
    tight = next(x for x in cases if x.tight and x.long_edge == c.long_edge)
    tensor, _, meta = EvalPreprocess(c.long_edge, tight_padding=True)(tight.src, [], None)
    check_case(tight, tensor[None], torch.float32, False)
    pu.check_meta(meta, tight)


def test_metas_feed_metas_device(cases):
    group = [c for c in cases if c.tight and c.long_edge == 26]
    pp = EvalPreprocess(26, tight_padding=True)
    _, metas = pp.batch([c.src for c in group], [{'image_id': 100 + i} for i in range(len(group))])
    d_metas, d_ids, d_swap = eval_coco.metas_device(metas)
    want = np.concatenate([transforms.meta_record(dict(c.meta, hflip=False, rotation=None))
                           for c in group])
    assert d_metas.cpu().numpy().tobytes() == want.tobytes()
    assert d_ids.cpu().tolist() == [100 + i for i in range(len(group))]
    assert d_swap is None


def test_empty_batch():
    out, metas = EvalPreprocess(33, tight_padding=True).batch([])
    assert out == [] and metas == []
    out, _ = EvalPreprocess(33).batch([])
    assert tuple(out.shape) == (0, 3, 33, 33)
