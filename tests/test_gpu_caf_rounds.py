"""The CafScored builds' memory rounds (csrc/stages.hip, caf_bucketed_body) on an MI355X.

Set B's stash form, where its launch is gated (after the seed loop), loads the confidence and
the four source rows of 13 cells per thread together (one round up to 13 * 512 = 6656 cells,
a second one above); ungated it scores two batches of 4096 cells.  Set A's one-head list
reads the confidence plane in rounds of 16 cells per thread (256 * 16 = 4096).  The field
sizes sit on those boundaries:

    1x1      1 cell     smallest field
    5x7      35         below one wave
    23x29    667        no multiple of 256 or 512
    64x104   6656       exactly 13 * 512: the last size of one set-B round
    81x83    6723       just above: the second round runs
    90x91    8190       top of the u16 form
    91x91    8281       first size of the non-stash form, whose code did not change

Each shape decodes a planted batch (set A lists its candidates) and a uniform batch (more than
kCandA cells pass, so set A falls back to the batched scan, and the images need set B) of three
images through the engine with eval defaults (force-complete on).  The planted batches at
1x1 and 5x7 are corners of a 16x16 planted field and hold few or no annotations: at those
sizes it is the uniform batch that gives the kernels work.  Every record field is
compared byte for byte with the host twin (stages_cpu.decode_batch).  Three more planted
batches: two with NaN confidences and NaN source coordinates in cells above the threshold (the
NaN bucket and the guards), and one in which the gate of set B takes its three outcomes.
"""
import numpy as np
import pytest

import kc_util as kc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (23, 29), (64, 104), (81, 83), (90, 91), (91, 91)]
N = 3
K = 17
# planted seeds of the gate case, picked on the host twin (the test asserts what they give)
GATE_SIZE = (33, 40)
GATE_SEEDS = (11, 0, 1)


@pytest.fixture(scope='module')
def eng():
    from openpifpaf_amd import engine
    return engine.DecodeEngine()


def _device(eng, cif, caf, skeleton, cfg):
    import torch
    recs, offsets, _ = eng.decode(torch.from_numpy(cif).cuda(), torch.from_numpy(caf).cuda(),
                                  skeleton, cfg)
    return recs.copy(), np.array(offsets)


def _same(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for key in got.dtype.names:  # every field of the record (not the padding between them)
        assert got[key].tobytes() == want[key].tobytes(), (where, key)


def _batch(gen, h, w, first_seed=0, n_people=4):
    from openpifpaf_amd import synthetic
    if gen == 'uniform':
        pairs = [synthetic.uniform(h, w, seed=first_seed + i) for i in range(N)]
    else:  # the generator needs 13 cells each way: smaller fields are a larger one's corner
        pairs = [synthetic.planted(max(h, 16), max(w, 16), n_people=n_people, seed=first_seed + i)
                 for i in range(N)]
    return (np.ascontiguousarray(np.stack([p[0] for p in pairs])[..., :h, :w]),
            np.ascontiguousarray(np.stack([p[1] for p in pairs])[..., :h, :w]))


def _check(eng, cif, caf, where):
    from openpifpaf_amd import constants, stages_cpu
    skeleton = constants.COCO_PERSON_SKELETON
    cfg = kc.config('eval')
    want, want_off = stages_cpu.decode_batch(cif, caf, skeleton, cfg)
    got, off = _device(eng, cif, caf, skeleton, cfg)
    assert np.array_equal(off, want_off), where
    _same(got, want, where)
    return want, want_off


def _unset_masks(cif, caf):
    """Per image: the joints left unset in any annotation before force-complete and NMS (the
    gate of set B), and the smallest number of set joints in an annotation (None: none)."""
    from openpifpaf_amd import constants, stages_cpu
    cfg = kc.config('eval', force_complete=False, apply_nms=False)
    recs, off = stages_cpu.decode_batch(cif, caf, constants.COCO_PERSON_SKELETON, cfg)
    out = []
    for i in range(len(off) - 1):
        is_set = recs['data'][off[i]:off[i + 1], :K, 2] > 0.0
        mask = 0
        for j in range(K):
            if len(is_set) and not is_set[:, j].all():
                mask |= 1 << j
        out.append((mask, int(is_set.sum(axis=1).min()) if len(is_set) else None))
    return out


@pytest.mark.parametrize('gen', ['planted', 'uniform'])
@pytest.mark.parametrize('shape', SHAPES, ids=['{}x{}'.format(*s) for s in SHAPES])
def test_batch_vs_twin(eng, shape, gen):
    h, w = shape
    cif, caf = _batch(gen, h, w)
    want, _ = _check(eng, cif, caf, (shape, gen))
    if h * w >= 667:
        assert len(want) >= N


def test_nan_confidences_and_sources_vs_twin(eng):
    """NaN in confidences and in source coordinates of cells far above both thresholds: a NaN
    confidence never passes, a NaN source goes to the NaN bucket.  The sources are the
    backward ones (x2, y2): with as many NaN (x1, y1) the host twin's decode itself ends in
    PP_ST_DEC_OVERFLOW; test_nan_forward_source_vs_twin has a single one per image."""
    h, w = 33, 40
    cif, caf = _batch('planted', h, w)
    for i in range(N):
        strong = np.argwhere(caf[i, :, 0] > 0.7)  # (field, y, x) of planted cells
        assert len(strong) >= 60
        for n, (f, y, x) in enumerate(strong[::7][:8]):
            caf[i, f, (0, 5, 6)[n % 3], y, x] = np.nan
    assert np.isnan(caf[:, :, 0]).sum() >= 3 and np.isnan(caf[:, :, (1, 2, 5, 6)]).sum() >= 9
    masks = _unset_masks(cif, caf)
    assert any(m for m, _ in masks), masks  # set B is built for some image
    _check(eng, cif, caf, 'nan')


def test_nan_forward_source_vs_twin(eng):
    """One NaN x1 per image, in a cell far above both thresholds: the forward direction's NaN
    bucket.  An image with every joint unset somewhere builds every set in both directions."""
    h, w = 33, 40
    cif, caf = _batch('planted', h, w)
    for i in range(N):
        f, y, x = np.argwhere(caf[i, :, 0] > 0.7)[370]
        caf[i, f, 1, y, x] = np.nan
    assert np.isnan(caf[:, :, 1]).sum() == N
    masks = _unset_masks(cif, caf)
    assert any(m == (1 << K) - 1 for m, _ in masks), masks  # every set, both directions
    want, _ = _check(eng, cif, caf, 'nan-forward')
    assert len(want) >= N


def test_gate_outcomes_vs_twin(eng):
    """One image with nothing to complete (its workgroups of set B write empty offsets), one
    with every joint unset in some annotation (both directions of every field), one between
    (some field needs one direction only)."""
    from openpifpaf_amd import constants, synthetic
    h, w = GATE_SIZE
    pairs = [synthetic.planted(h, w, n_people=4, seed=s) for s in GATE_SEEDS]
    cif, caf = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    masks = _unset_masks(cif, caf)
    print('gate masks', [(hex(m), n) for m, n in masks])
    full = (1 << K) - 1
    assert any(m == 0 and n == K for m, n in masks), masks
    assert any(m == full and n <= 2 for m, n in masks), masks
    one_dir = [m for m, _ in masks
               if any(((m >> (a - 1)) & 1) != ((m >> (b - 1)) & 1)
                      for a, b in constants.COCO_PERSON_SKELETON)]
    assert one_dir, masks
    _check(eng, cif, caf, 'gate')
