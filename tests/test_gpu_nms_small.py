"""nms_kernel<W, 0>'s path for images of at most kNmsSmall (64) annotations, on an MI355X.

An image with up to 64 annotations is decided across lanes (csrc/nms.hip, nms_small); 65 is the
first size on the box-list path.  pp_nms_keypoints (the 8-wave instance) is compared with the
reference's nms.Keypoints as the oracle runs it and with the host twin: the survivors' input
indices and order, their records, their scores against oracle.ann_score, and the input records
as the kernel left them, all exactly.  Sizes 1, 2, 9, 40, 64 and 65 at K = 1, 3, 8, 17 and 24
under the three configurations of tests/test_kc_cpu.py; one launch with groups of 0, 9, 64 and
65 poses, so that both paths run in one grid; an empty occupancy grid (negative coordinates);
a grid far larger than any field (one joint at (6000, 6000)).  Then one pp_decode_batch (the
4-wave instance) over planted and uniform images of one field size, every record field against
the host twin's.  The counts asserted on the reference's own results keep the comparisons from
passing vacuously."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from test_kc_cpu import NMS_CFGS, nms_poses

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 9, 40, 64, 65)
KS = (1, 3, 8, 17, 24)
SUBSETS = {1: [0], 2: [44, 54], 9: [0, 1, 2, 3, 4, 5, 44, 54, 45]}  # rows of nms_poses(k, n=64)
DECODE_SIDE = 33


def _poses(k, n):
    if n in SUBSETS:
        data, scales = nms_poses(k, n=64)
        return data[SUBSETS[n]].copy(), scales[SUBSETS[n]].copy()
    return nms_poses(k, n=n)


def _config(c):
    from openpifpaf_amd._abi import make_config
    kt, it, sup = c
    return make_config(nms_keypoint_threshold=kt, nms_instance_threshold=it, nms_suppression=sup)


def _reference(data, scales, c):
    """The reference's result and the host twin's, which must agree: (survivors' input
    indices, their records, their scores, the input data as the NMS leaves it)."""
    from openpifpaf_amd import stages_cpu
    k = data.shape[1]
    order, recs = oracle.nms_keypoints(data, scales, *c)
    want = np.array([oracle.ann_score(d[:, 2]) for d in recs['data'][:, :k]], np.float64)
    left = data.copy()
    twin_order, twin_scores = stages_cpu.nms_keypoints(left, scales, _config(c))
    assert list(twin_order) == order.tolist()
    assert np.array_equal(np.asarray(twin_scores, np.float64), want)
    assert np.array_equal(left[order], recs['data'][:, :k])
    return order, recs, want, left


@functools.lru_cache(maxsize=None)
def _case(k, n, ci):
    data, scales = _poses(k, n)
    return (data, scales) + _reference(data, scales, NMS_CFGS[ci])


def _device_nms(groups, k, cfg, cap):
    """pp_nms_keypoints over groups of (data, scales) in one launch -> per group (survivors'
    input indices, their records, the input records as the kernel left them)."""
    import torch
    from openpifpaf_amd import _device
    from openpifpaf_amd._abi import ANN_DTYPE
    from openpifpaf_amd._lib import call, load
    n_img = len(groups)
    recs = np.zeros((n_img, cap), ANN_DTYPE)
    counts = np.zeros(n_img, np.int32)
    for i, (data, scales) in enumerate(groups):
        n = len(data)
        counts[i] = n
        recs['data'][i, :n, :k] = data
        recs['joint_scales'][i, :n, :k] = scales
    recs['n_keypoints'] = k
    d_in = torch.from_numpy(recs.view(np.uint8).reshape(n_img * cap, ANN_DTYPE.itemsize)).cuda()
    d_out = torch.zeros_like(d_in)
    d_counts = torch.from_numpy(counts).cuda()
    d_out_counts = torch.full((n_img,), -1, dtype=torch.int32, device='cuda')
    d_index = torch.zeros(n_img * cap, dtype=torch.int32, device='cuda')
    ws = torch.empty(int(load().pp_nms_workspace_size(n_img, cap)), dtype=torch.uint8,
                     device='cuda')
    call('pp_nms_keypoints', _device.ptr(d_in), _device.ptr(d_counts), n_img, k, cap,
         ctypes.byref(cfg), _device.ptr(d_out), _device.ptr(d_out_counts), _device.ptr(d_index),
         _device.ptr(ws), ctypes.c_size_t(ws.numel()), _device.stream())
    out_counts = d_out_counts.cpu().numpy()
    out = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=ANN_DTYPE).reshape(n_img, cap)
    edited = np.frombuffer(d_in.cpu().numpy().tobytes(), dtype=ANN_DTYPE).reshape(n_img, cap)
    index = d_index.cpu().numpy().reshape(n_img, cap)
    return [(index[i, :out_counts[i]], out[i, :out_counts[i]], edited[i, :counts[i]])
            for i in range(n_img)]


def _check(got, k, data, scales, order, recs, want, left, where):
    """The four comparisons of test_nms_keypoints_vs_oracle, and every input record against
    the host twin's."""
    index, out, edited = got
    assert index.tolist() == order.tolist(), where
    assert np.array_equal(out['data'], recs['data']), where
    assert np.array_equal(out['score'], want), where
    assert np.array_equal(edited['data'][order], recs['data']), where
    assert edited['data'][:, :k].tobytes() == left.tobytes(), where
    assert np.array_equal(edited['joint_scales'][:, :k], scales), where


def _stats(data, want, left):
    """(edited confidences, equal adjacent scores among the survivors)"""
    return int((left[:, :, 2] != data[:, :, 2]).sum()), int((np.diff(want) == 0).sum())


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', SIZES)
def test_sizes_vs_oracle(n, k):
    for ci, c in enumerate(NMS_CFGS):
        data, scales, order, recs, want, left = _case(k, n, ci)
        edited, ties = _stats(data, want, left)
        # what the inputs must exercise, on the reference's result
        if n >= 40:
            assert edited >= 7 and ties >= 10, (c, edited, ties)
            if ci == 1 and k <= 8:
                assert len(order) < n  # annotations dropped by the score filters
        if n == 9:
            assert ties >= 1
            assert k < 3 or edited >= {3: 1, 8: 3, 17: 2, 24: 19}[k]
        if n == 2:
            assert len(order) == 2 and ties == 1
        got, = _device_nms([(data, scales)], k, _config(c), n)
        _check(got, k, data, scales, order, recs, want, left, (n, k, c))


@pytest.mark.parametrize('k', (3, 17))
def test_mixed_groups_in_one_launch(k):
    """0, 9, 64 and 65 poses: both paths in one grid, and an image without annotations."""
    empty = (np.zeros((0, k, 3), np.float32), np.zeros((0, k), np.float32))
    for ci, c in enumerate(NMS_CFGS):
        cases = [_case(k, n, ci) for n in (9, 64, 65)]
        groups = [empty] + [(cs[0], cs[1]) for cs in cases]
        got = _device_nms(groups, k, _config(c), 65)
        assert len(got[0][0]) == 0 and len(got[0][1]) == 0
        for g, cs in zip(got[1:], cases):
            _check(g, k, *cs, (len(cs[0]), k, c))


@pytest.mark.parametrize('k', KS)
def test_negative_coordinates_empty_grid(k):
    """Every coordinate shifted by -500: int(max y + 1) <= 0, an occupancy grid without cells;
    nothing is occupied and nothing marked."""
    data, scales = _poses(k, 9)
    data[:, :, :2] -= np.float32(500.0)
    for c in NMS_CFGS:
        order, recs, want, left = _reference(data, scales, c)
        assert np.array_equal(left[:, :, 2], data[:, :, 2])  # no confidence edited
        if c[0] == 0.0:
            assert len(order) == 9 and np.array_equal(left, data)
        got, = _device_nms([(data, scales)], k, _config(c), 9)
        _check(got, k, data, scales, order, recs, want, left, (k, c))


@pytest.mark.parametrize('k', (3, 17))
def test_far_joint_large_grid(k):
    """Joint 0 of pose 0 at (6000, 6000): a grid of 3000 x 3000 cells per plane, far larger
    than any field (the reference allocates it densely: no further out)."""
    data, scales = nms_poses(k, n=64)
    data, scales = data[:9].copy(), scales[:9].copy()
    data[0, 0, :2] = np.float32(6000.0)
    for c in NMS_CFGS:
        order, recs, want, left = _reference(data, scales, c)
        edited, _ = _stats(data, want, left)
        assert edited == {3: 5, 17: 26}[k], (c, edited)
        got, = _device_nms([(data, scales)], k, _config(c), 9)
        _check(got, k, data, scales, order, recs, want, left, (k, c))


def test_through_the_decoder():
    """One pp_decode_batch (4-wave NMS) whose images take both paths: planted images with a
    handful of records, uniform ones with more than 64."""
    import torch
    from openpifpaf_amd import constants, engine, stages_cpu, synthetic
    from openpifpaf_amd._abi import EVAL_CONFIG, make_config
    cfg = make_config(**EVAL_CONFIG)
    skeleton = constants.COCO_PERSON_SKELETON
    cif_p, caf_p = synthetic.batch('planted', 2, DECODE_SIDE, DECODE_SIDE)
    cif_u, caf_u = synthetic.batch('uniform', 2, DECODE_SIDE, DECODE_SIDE)
    cif = np.stack([cif_p[0], cif_u[0], cif_p[1], cif_u[1]])
    caf = np.stack([caf_p[0], caf_u[0], caf_p[1], caf_u[1]])
    want, want_off = stages_cpu.decode_batch(cif, caf, skeleton, cfg)
    per_image = np.diff(want_off)
    assert (per_image > 64).any() and ((per_image >= 1) & (per_image <= 64)).any(), per_image
    recs, off, _ = engine.DecodeEngine().decode(torch.from_numpy(cif).cuda(),
                                                torch.from_numpy(caf).cuda(), skeleton, cfg)
    assert np.array_equal(np.array(off), want_off)
    assert len(recs) == len(want)
    for key in recs.dtype.names:  # every field of the record (not the padding between them)
        assert recs[key].tobytes() == want[key].tobytes(), key
