"""pp_fields_from_conv_ragged_interleaved on the device (heads.fields_from_conv_ragged,
engine.RaggedFields.from_conv, RaggedDetFields.from_conv with channels-last conv outputs):
the channels-last conv outputs of images of different sizes are read where they lie, straight
into the container of a ragged batch.  The expected value of every comparison comes from code
that existed before, on dense NCHW clones of the same values: heads.fields_from_conv per
image, zero-padded with torch into the container's shape (test_gpu_ingest_ragged._padded).
Every comparison is of bytes; containers are pre-filled with NaN so that an unwritten element
shows."""
import numpy as np
import pytest

from test_gpu_ingest_ragged import (EXTENTS, NAN, _batched, _caf_and_dense, _case,
                                    _field_extents, _padded, _planted, _same_annotations,
                                    cifcaf)  # noqa: F401  pylint: disable=unused-import
from test_gpu_ingest_strided import SENTINEL, _bytes, _head, _peak_rise
from test_gpu_ragged_det import _cifdet, _convs, dec  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

# conv rows of one full 16-pixel tile plus 1, two full tiles plus 1 and exactly one tile,
# beside a 1x1 image: some tiles of the container lie wholly outside an image
TILES = [(2, 17), (1, 33), (3, 16), (1, 1)]


def _nhwc(c):
    """The values of c (ch, h, w) as a channels-last tensor of its own, still (ch, h, w)."""
    import torch
    ch, h, w = c.shape
    t = torch.empty((h, w, ch), dtype=c.dtype, device=c.device).permute(2, 0, 1)
    t.copy_(c)
    assert tuple(t.stride()) == (1, w * ch, ch)
    return t


def _ingest(convs, n_fields, kind, quad=1, interleaved=True, **kw):
    """heads.fields_from_conv_ragged, and which symbol the call was classified for."""
    from openpifpaf_amd import heads
    ing = heads.RaggedIngest(convs, n_fields, kind, quad, kw.pop('hflip', None),
                             kw.pop('conv_extents', None), kw.pop('shape', None),
                             kw.pop('out', None), kw.pop('out_field0', 0))
    assert not kw and ing.interleaved is interleaved
    ing.launch()
    return ing.out, ing.extents, ing.extents_host


# ---- 1. the grid of small cases -----------------------------------------------------------
# CAF at quad 1 is 684 channels in two chunks (344, 340), at quad 2 2,736 in six; CIF at quad 0
# is 85 channels, no multiple of a 16-byte vector
@pytest.mark.parametrize('quad', [0, 1, 2])
@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('kind', ['cif', 'caf', 'cifdet'])
def test_grid(kind, dtype_name, flipped, quad):
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case(kind, dtype_name, flipped, quad)
    views = [_nhwc(c) for c in convs]
    out = torch.full(want.shape, NAN, device='cuda')
    got, ext, ext_host = _ingest(views, n_fields, kind, quad, hflip=flip, out=out)
    assert got is out and _bytes(got) == _bytes(want)
    assert ext.dtype == torch.int32 and ext_host.dtype == np.int32
    assert ext.cpu().numpy().tolist() == ext_host.tolist() == _field_extents(EXTENTS, quad)
    # a container of the call's own, and (1, ch, h, w) channels-last inputs
    four = [c[None].contiguous(memory_format=torch.channels_last) for c in convs]
    got, ext, _ = heads.fields_from_conv_ragged(four, n_fields, kind, quad, hflip=flip)
    assert got.shape == want.shape and _bytes(got) == _bytes(want)
    assert ext.cpu().numpy().tolist() == _field_extents(EXTENTS, quad)


# ---- 2. tile boundaries -------------------------------------------------------------------
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
@pytest.mark.parametrize('kind', ['cif', 'caf'])
def test_tile_boundaries(kind, dtype_name):
    import torch
    convs, n_fields, flip, want = _case(kind, dtype_name, True, 1, tuple(TILES))
    assert tuple(want.shape[3:]) == (5, 65)
    out = torch.full(want.shape, NAN, device='cuda')
    _ingest([_nhwc(c) for c in convs], n_fields, kind, 1, hflip=flip, out=out)
    assert _bytes(out) == _bytes(want)


# ---- 3. a larger container, and one 4 bytes off a 16-byte boundary ---------------------------
@pytest.mark.parametrize('flipped', [False, True])
def test_container_larger_than_every_image(flipped):
    """(11, 16) over fields of at most 9 x 13: the tile grid follows the container (6 conv
    rows of one tile), so the rows and columns past every image are written too."""
    import torch
    convs, n_fields, flip, _ = _case('cif', 'float32', flipped, 1)
    want = _padded(convs, n_fields, 'cif', 1, flip, shape=(11, 16))
    out = torch.full(want.shape, NAN, device='cuda')
    got, ext, _ = _ingest([_nhwc(c) for c in convs], n_fields, 'cif', 1, hflip=flip,
                          shape=(11, 16), out=out)
    assert got.shape == want.shape == (6, 17, 5, 11, 16)
    assert _bytes(got) == _bytes(want)
    assert ext.cpu().numpy().tolist() == _field_extents(EXTENTS, 1)
    # a container two tiles wide whose second tile no image reaches
    want = _padded(convs, n_fields, 'cif', 1, flip, shape=(9, 35))
    got, _, _ = _ingest([_nhwc(c) for c in convs], n_fields, 'cif', 1, hflip=flip,
                        shape=(9, 35), out=torch.full(want.shape, NAN, device='cuda'))
    assert _bytes(got) == _bytes(want)


@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_container_off_a_16_byte_boundary(dtype_name):
    import torch
    convs, n_fields, flip, want = _case('caf', dtype_name, True, 1)
    assert want.shape[4] == 13  # W odd: the planes start at every 4-byte phase
    flat = torch.full((1 + want.numel() + 3,), SENTINEL, device='cuda')
    out = flat[1:1 + want.numel()].view(want.shape)
    out.fill_(NAN)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    got, _, _ = _ingest([_nhwc(c) for c in convs], n_fields, 'caf', 1, hflip=flip, out=out)
    assert got is out and _bytes(out) == _bytes(want)
    assert flat[0].item() == SENTINEL and (flat[1 + want.numel():] == SENTINEL).all()


# ---- 4. the batched form ------------------------------------------------------------------
@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
@pytest.mark.parametrize('kind', ['cif', 'caf'])
def test_batched_channels_last_with_extents(kind, dtype_name, flipped):
    import torch
    convs, n_fields, flip, want = _case(kind, dtype_name, flipped, 1)
    ch = convs[0].shape[0]
    big = _batched(convs).contiguous(memory_format=torch.channels_last)
    assert big.shape == (6, ch, 5, 7) and big.stride() == (35 * ch, 1, 7 * ch, ch)
    assert big.isnan().any()
    for extents in (EXTENTS, np.array(EXTENTS), torch.tensor(EXTENTS)):
        out = torch.full(want.shape, NAN, device='cuda')
        got, ext, _ = _ingest(big, n_fields, kind, 1, hflip=flip, conv_extents=extents, out=out)
        assert _bytes(got) == _bytes(want) and not got.isnan().any()
        assert ext.cpu().numpy().tolist() == _field_extents(EXTENTS, 1)


# ---- 5. a channel slice of a wider channels-last tensor ---------------------------------------
@pytest.mark.parametrize('dtype_name', ['float16', 'bfloat16'])
@pytest.mark.parametrize('kind', ['cif', 'caf'])
def test_channel_slice_of_a_fused_conv(kind, dtype_name):
    """[:, 3:3 + ch] of 1,024 channels-last channels: every pixel's run starts 6 bytes off a
    16-byte boundary, so the single-element head (5 elements) and tail loads run."""
    import torch
    convs, n_fields, flip, want = _case(kind, dtype_name, True, 1)
    ch = convs[0].shape[0]
    fused = _batched(convs, channels0=3, channels=1024).contiguous(
        memory_format=torch.channels_last)
    view = fused[:, 3:3 + ch]
    assert view.stride() == (35 * 1024, 1, 7 * 1024, 1024) and view.data_ptr() % 16 == 6
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(view, n_fields, kind, 1, hflip=flip, conv_extents=EXTENTS, out=out)
    assert _bytes(got) == _bytes(want) and not got.isnan().any()
    # the same slices as a list of per-image views
    views = [view[i, :, :h, :w] for i, (h, w) in enumerate(EXTENTS)]
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(views, n_fields, kind, 1, hflip=flip, out=out)
    assert _bytes(got) == _bytes(want)


# ---- 6. row- and column-sliced views ------------------------------------------------------
@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_spatial_crops_of_larger_nhwc_tensors(dtype_name):
    """Row stride (w + 3) * ch > w_i * column stride; the rest of each larger tensor is NaN."""
    import torch
    convs, n_fields, flip, want = _case('caf', dtype_name, True, 1)
    views = []
    for c in convs:
        ch, h, w = c.shape
        big = torch.full((h + 2, w + 3, ch), NAN, dtype=c.dtype, device='cuda')
        big[1:1 + h, 2:2 + w] = c.permute(1, 2, 0)
        views.append(big[1:1 + h, 2:2 + w].permute(2, 0, 1))
        assert views[-1].stride() == (1, (w + 3) * ch, ch)
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(views, n_fields, 'caf', 1, hflip=flip, out=out)
    assert _bytes(got) == _bytes(want) and not got.isnan().any()
    # a column stride of two pixels: every other column of a tensor twice as wide
    wide = []
    for c in convs:
        ch, h, w = c.shape
        big = torch.full((h, 2 * w, ch), NAN, dtype=c.dtype, device='cuda')
        big[:, ::2] = c.permute(1, 2, 0)
        wide.append(big[:, ::2].permute(2, 0, 1))
    assert wide[3].stride() == (1, 14 * ch, 2 * ch)
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(wide, n_fields, 'caf', 1, hflip=flip, out=out)
    assert _bytes(got) == _bytes(want)


# ---- 7. a field range: caf_parts -------------------------------------------------------------
@pytest.mark.parametrize('flipped', [False, True])
def test_field_range_and_caf_parts(flipped):
    import torch
    from openpifpaf_amd import engine
    ((caf, _, caf_flip, caf_want), (dense, _, dense_flip, _)), want = _caf_and_dense(flipped)
    caf, dense = [_nhwc(c) for c in caf], [_nhwc(c) for c in dense]
    assert want.shape == (6, 44, 9, 9, 13)
    out = torch.full(want.shape, SENTINEL, device='cuda')
    res, _, _ = _ingest(caf, 19, 'caf', 1, hflip=caf_flip, out=out)
    assert res is out
    assert (out[:, 19:] == SENTINEL).all()  # zero region included
    assert _bytes(out[:, :19].contiguous()) == _bytes(caf_want)
    _ingest(dense, 25, 'caf', 1, hflip=dense_flip, out=out, out_field0=19)
    assert _bytes(out) == _bytes(want)
    # the same through RaggedFields.from_conv(caf_parts=)
    n_cif, cif_flip = _head('cif')
    cif, _, _, cif_want = _case('cif', 'float32', flipped, 1)
    ragged = engine.RaggedFields.from_conv(
        [_nhwc(c) for c in cif], None, n_cif, None, quad=1,
        cif_hflip=cif_flip if flipped else None,
        caf_parts=[(caf, 19, caf_flip), (dense, 25, dense_flip)])
    assert all(i.interleaved for i in ragged._ingests)  # pylint: disable=protected-access
    assert (ragged.k, ragged.c, ragged.h, ragged.w) == (17, 44, 9, 13)
    assert _bytes(ragged.caf) == _bytes(want) and _bytes(ragged.cif) == _bytes(cif_want)


# ---- 8. end to end ------------------------------------------------------------------------
def _ragged_pair():
    """RaggedFields.from_conv of the six planted images: from NCHW convs, from channels-last."""
    from openpifpaf_amd import engine
    convs, _ = _planted()
    cifs, cafs = [c[0] for c in convs], [c[1] for c in convs]
    planar = engine.RaggedFields.from_conv(cifs, cafs, 17, 19, quad=0)
    last = engine.RaggedFields.from_conv([_nhwc(c) for c in cifs], [_nhwc(c) for c in cafs],
                                         17, 19, quad=0)
    assert not any(i.interleaved for i in planar._ingests)  # pylint: disable=protected-access
    assert all(i.interleaved for i in last._ingests)  # pylint: disable=protected-access
    assert _bytes(last.cif) == _bytes(planar.cif) and _bytes(last.caf) == _bytes(planar.caf)
    assert last.extents.cpu().numpy().tolist() == planar.extents_host.tolist()
    return planar, last


def test_decode_ragged_from_channels_last_conv(cifcaf):  # noqa: F811  pylint: disable=redefined-outer-name
    from openpifpaf_amd import heads
    planar, last = _ragged_pair()
    got, want = cifcaf.decode_ragged(last), cifcaf.decode_ragged(planar)
    print(cifcaf.mode, 'annotations per image', [len(a) for a in got])
    assert len(got) == len(want) == 6 and sum(len(a) for a in got) >= 1
    for g, w in zip(got, want):
        _same_annotations(g, w)
    # RaggedCollector passes the tensors through; pack() runs the two launches again after
    # the convs were rewritten in place
    convs, _ = _planted()
    cifs, cafs = [_nhwc(c[0]) for c in convs], [_nhwc(c[1]) for c in convs]
    collected = heads.RaggedCollector(17, 19, quad=0)((cifs, cafs))
    assert _bytes(collected.cif) == _bytes(planar.cif)
    assert _bytes(collected.caf) == _bytes(planar.caf)
    for t in cifs + cafs:
        t.neg_()
    collected.pack()
    assert _bytes(collected.cif) != _bytes(planar.cif)
    for t in cifs + cafs:
        t.neg_()
    collected.cif.fill_(NAN)
    collected.caf.fill_(NAN)
    collected.extents.fill_(-1)
    collected.pack()
    assert _bytes(collected.cif) == _bytes(planar.cif)
    assert _bytes(collected.caf) == _bytes(planar.caf)
    assert collected.extents.cpu().numpy().tolist() == planar.extents_host.tolist()


def test_coco_ragged_from_channels_last_conv(cifcaf):  # noqa: F811  pylint: disable=redefined-outer-name
    from test_oracle_golden import inverse_metas
    planar, last = _ragged_pair()
    named = inverse_metas()
    metas = [dict(named[('shift', 'flip', 'rot')[i % 3]], image_id=70 + i) for i in range(6)]
    got = cifcaf.coco_ragged(last, metas, max_per_image=5)
    want = cifcaf.coco_ragged(planar, metas, max_per_image=5)
    assert got.offsets.tolist() == want.offsets.tolist() and got.offsets[-1] >= 1
    assert got.flags.tolist() == want.flags.tolist()
    assert got.records.tobytes() == want.records.tobytes()


@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_cifdet_decode_ragged_from_channels_last_conv(dec, dtype_name):  # noqa: F811  pylint: disable=redefined-outer-name
    import test_gpu_ragged_det as det
    from openpifpaf_amd import engine, heads
    convs, _ = _convs(dtype_name)
    cd = _cifdet(dec, 'uniform')
    planar = engine.RaggedDetFields.from_conv(convs, det.rd.K, quad=1)
    last = engine.RaggedDetFields.from_conv([_nhwc(c) for c in convs], det.rd.K, quad=1)
    assert last._ingests[0].interleaved and not planar._ingests[0].interleaved  # pylint: disable=protected-access
    assert _bytes(last.det) == _bytes(planar.det)
    assert last.extents.cpu().numpy().tolist() == planar.extents_host.tolist()
    collected = heads.RaggedDetCollector(det.rd.K, quad=1)(([_nhwc(c) for c in convs],))
    assert _bytes(collected.det) == _bytes(planar.det)
    got, want = cd.decode_ragged(last), cd.decode_ragged(planar)
    assert len(got) == 6 and min(len(a) for a in want) >= 1
    for g, w in zip(got, want):
        assert [a.field_i for a in g] == [a.field_i for a in w]
        for name in ('score', 'bbox'):
            assert np.array([getattr(a, name) for a in g], np.float32).tobytes() == \
                np.array([getattr(a, name) for a in w], np.float32).tobytes()


# ---- 9. no copy ---------------------------------------------------------------------------
def _tables_bytes(n):
    from openpifpaf_amd._lib import load
    return int(load().pp_ragged_conv_tables_size(n))


def test_channels_last_list_makes_no_copy():
    """Eight channels-last float16 convs of 340 x 40 x 40, 8.3 MiB together: the call allocates
    its container and its tables and nothing of the convs' size (the .contiguous() copies of
    the route before would add 8.3 MiB)."""
    import torch
    from openpifpaf_amd import heads
    convs = [_nhwc(torch.randn((340, 40, 40), device='cuda').to(torch.float16))
             for _ in range(8)]
    assert sum(c.nbytes for c in convs) >= 8 << 20
    (out, ext, _), raised = _peak_rise(
        lambda: heads.fields_from_conv_ragged(convs, 17, 'cif', 1))
    print('peak raised by', raised, 'bytes; out', out.nbytes, 'convs',
          sum(c.nbytes for c in convs))
    assert out.shape == (8, 17, 5, 79, 79) and ext.tolist() == [[79, 79]] * 8
    assert raised <= out.nbytes + _tables_bytes(8) + (1 << 20)
    want = heads.fields_from_conv(torch.stack(convs).contiguous(), 17, 'cif', 1)
    assert _bytes(out) == _bytes(want)


def test_batched_channels_last_makes_no_copy():
    import torch
    from openpifpaf_amd import heads
    conv = torch.randn((8, 340, 40, 40), device='cuda').to(torch.float16).contiguous(
        memory_format=torch.channels_last)
    assert conv.nbytes >= 8 << 20 and not conv.is_contiguous() and conv.stride()[1] == 1
    extents = [(40 - i, 33 + i) for i in range(8)]
    (out, ext, _), raised = _peak_rise(
        lambda: heads.fields_from_conv_ragged(conv, 17, 'cif', 1, conv_extents=extents))
    print('peak raised by', raised, 'bytes; out', out.nbytes, 'conv', conv.nbytes)
    assert out.shape == (8, 17, 5, 79, 79)
    assert ext.tolist() == [[2 * h - 1, 2 * w - 1] for h, w in extents]
    assert raised <= out.nbytes + _tables_bytes(8) + (1 << 20)


# ---- 10. classification -------------------------------------------------------------------
def test_mixed_list_stays_planar():
    """One channels-last image among planar ones (each readable by one symbol only): the call
    is the planar one, as before, and gives the same bytes."""
    import torch
    convs, n_fields, flip, want = _case('caf', 'float32', True, 1)
    views = list(convs)
    views[3] = _nhwc(convs[3])
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(views, n_fields, 'caf', 1, interleaved=False, hflip=flip, out=out)
    assert _bytes(got) == _bytes(want)
    # the 1x1 image is readable both ways and decides nothing
    views = [_nhwc(c) for c in convs]
    views[0] = convs[0]
    assert views[0].stride(0) == 1 and views[0].stride(2) == 1
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(views, n_fields, 'caf', 1, hflip=flip, out=out)
    assert _bytes(got) == _bytes(want)


@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_view_that_is_neither_is_copied_once(dtype_name):
    """A step along both the channels and the columns: that image is copied into the call's
    class, the others are read where they lie."""
    import torch
    from openpifpaf_amd import heads
    convs, n_fields, flip, want = _case('cif', dtype_name, True, 1)
    ch, h, w = convs[4].shape
    big = torch.full((2 * ch, h, 2 * w), NAN, dtype=convs[4].dtype, device='cuda')
    big[::2, :, ::2] = convs[4]
    neither = big[::2, :, ::2]
    assert neither.stride(0) != 1 and neither.stride(2) != 1
    for others, interleaved in ((_nhwc, True), (lambda c: c, False)):
        views = [others(c) for c in convs]
        views[4] = neither
        ing = heads.RaggedIngest(views, n_fields, 'cif', 1, flip,
                                 out=torch.full(want.shape, NAN, device='cuda'))
        assert ing.interleaved is interleaved
        kept = ing._convs  # pylint: disable=protected-access
        assert [k.data_ptr() == v.data_ptr() for k, v in zip(kept, views)] == \
            [True] * 4 + [False, True]
        ing.launch()
        assert _bytes(ing.out) == _bytes(want)
    # the batched form: copied whole, read as planar
    big = torch.full((6, 2 * ch, 5, 14), NAN, dtype=convs[0].dtype, device='cuda')
    for i, c in enumerate(convs):
        big[i, ::2, :c.shape[1], :2 * c.shape[2]:2] = c
    out = torch.full(want.shape, NAN, device='cuda')
    got, _, _ = _ingest(big[:, ::2, :, ::2], n_fields, 'cif', 1, interleaved=False, hflip=flip,
                        conv_extents=EXTENTS, out=out)
    assert _bytes(got) == _bytes(want) and not got.isnan().any()
