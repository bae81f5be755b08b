"""pp_fields_from_conv_strided on the device: channels-last conv outputs and views of larger
tensors (channel, batch and spatial slices) are read where they lie.  The expected value of
every comparison is heads.fields_from_conv on a dense NCHW clone of the same values, which
takes the kernel the dense tensors always took; every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

from openpifpaf_amd import constants

pytestmark = pytest.mark.gpu

KPS = constants.COCO_KEYPOINTS
SKEL = constants.COCO_PERSON_SKELETON
DENSE = constants.DENSER_COCO_PERSON_CONNECTIONS
PER = {'cif': 5, 'caf': 9, 'cifdet': 7}
EINVAL = -1
SENTINEL = -7.25

# +0, -0, smallest and largest subnormal, largest finite, +-inf as bit patterns
SPECIALS = {'float16': [0x0000, 0x8000, 0x0001, 0x83ff, 0x7bff, 0xfbff, 0x7c00, 0xfc00],
            'bfloat16': [0x0000, 0x8000, 0x0001, 0x807f, 0x7f7f, 0xff7f, 0x7f80, 0xff80]}


def _head(kind):
    from openpifpaf_amd import heads
    return {'cif': (17, heads.cif_hflip(KPS)), 'caf': (19, heads.caf_hflip(KPS, SKEL)),
            'dense': (25, heads.caf_hflip(KPS, DENSE)), 'cifdet': (3, heads.HFlip())}[kind]


def _values(rng, dtype_name, shape):
    """Dense NCHW device tensor of random values; a half one has the special values
    scattered over it."""
    import torch
    dtype = getattr(torch, dtype_name)
    conv = torch.from_numpy((2.0 * rng.standard_normal(shape)).astype(np.float32)).to(dtype)
    if dtype_name in SPECIALS:
        bits = conv.view(torch.int16).reshape(-1)
        where = rng.choice(bits.numel(), size=min(bits.numel() // 2, 4096), replace=False)
        vals = np.array(SPECIALS[dtype_name], np.uint16)[np.arange(len(where)) % 8]
        bits[torch.from_numpy(where)] = torch.from_numpy(vals.view(np.int16))
    return conv.cuda()


def _channels_last(x):
    """The values of x (B, C, h, w) in NHWC memory order, still shaped (B, C, h, w)."""
    import torch
    b, c, h, w = x.shape
    base = torch.empty((b, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    base.copy_(x)
    assert base.stride() == (h * w * c, 1, w * c, c)
    return base


def _bytes(t):
    import torch
    if t.dtype != torch.float32:
        t = t.view(torch.int16)
    return t.cpu().numpy().tobytes()


def _check(view, n_fields, kind, quad, flip, dense_input=False):
    """fields_from_conv(view) == fields_from_conv(dense NCHW clone), byte for byte."""
    import torch
    from openpifpaf_amd import heads
    clone = view.clone(memory_format=torch.contiguous_format)
    assert clone.is_contiguous() and clone.stride()[3] == 1
    assert _bytes(clone) == _bytes(view.contiguous())
    # torch calls a (B, C, 1, 1) tensor contiguous in every memory format: there the
    # strides are what tells the formats apart
    assert dense_input or not view.is_contiguous() or view.shape[2] * view.shape[3] == 1
    want = heads.fields_from_conv(clone, n_fields, kind, quad, hflip=flip)
    got = heads.fields_from_conv(view, n_fields, kind, quad, hflip=flip)
    assert got.shape == want.shape == (
        view.shape[0], n_fields, PER[kind], heads.fields_dim(view.shape[2], quad),
        heads.fields_dim(view.shape[3], quad))
    assert got.dtype == want.dtype == torch.float32
    assert _bytes(got) == _bytes(want)
    return got


# (2, 70, 1): the tile is 16 conv pixels of a row, so 70 is four full tiles and one of 6
@pytest.mark.parametrize('h,w,quad', [(1, 1, 1), (3, 4, 0), (4, 3, 0), (9, 10, 1), (2, 3, 2),
                                      (2, 70, 1)])
@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16', 'bfloat16'])
@pytest.mark.parametrize('kind', ['cif', 'caf', 'cifdet'])
def test_channels_last_equals_planar(kind, dtype_name, flipped, h, w, quad):
    n_fields, flip = _head(kind)
    rng = np.random.default_rng(1000 * h + 10 * w + quad)
    ch = n_fields * PER[kind] * 4 ** quad
    for b in (1, 3):
        nhwc = _channels_last(_values(rng, dtype_name, (b, ch, h, w)))
        assert nhwc.stride()[1] == 1 and nhwc.stride()[3] == ch
        _check(nhwc, n_fields, kind, quad, flip if flipped else None)


def test_dense_input_takes_the_existing_symbols_kernel():
    """The reference of every test here: a dense NCHW tensor through fields_from_conv is
    pp_fields_from_conv_ex and, unflipped float32, pp_fields_from_conv, byte for byte."""
    import torch
    from openpifpaf_amd import _device, heads
    from openpifpaf_amd._lib import call
    n_fields, flip = _head('caf')
    conv = _values(np.random.default_rng(5), 'float32', (2, 19 * 9 * 4, 9, 10))
    src, swap = flip.tables(n_fields)
    for hflip in (None, flip):
        new = heads.fields_from_conv(conv, n_fields, 'caf', 1, hflip=hflip)
        old = torch.full_like(new, SENTINEL)
        call('pp_fields_from_conv_ex', _device.ptr(conv), 0, 2, n_fields, 1, 9, 10, 1,
             int(hflip is not None), src if hflip else None, swap if hflip else None,
             _device.ptr(old), n_fields, 0, _device.stream())
        assert _bytes(new) == _bytes(old)
    old = torch.full_like(new, SENTINEL)
    call('pp_fields_from_conv', _device.ptr(conv), 2, n_fields, 1, 9, 10, 1, _device.ptr(old),
         _device.stream())
    assert _bytes(heads.fields_from_conv(conv, n_fields, 'caf', 1)) == _bytes(old)


def _fused(rng, dtype_name, fmt, b=2, h=5, w=6):
    """One fused head tensor of 1026 channels: NaN, CIF (340), CAF (684), NaN."""
    big = _values(rng, dtype_name, (b, 1026, h, w))
    big[:, 0] = float('nan')
    big[:, 1025] = float('nan')
    return _channels_last(big) if fmt == 'nhwc' else big


@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('fmt', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype_name', ['float32', 'float16'])
def test_channel_slices_of_a_fused_tensor(dtype_name, fmt, flipped):
    """big[:, 1:341] and big[:, 341:1025]: the odd channel offset leaves a channels-last
    half slice aligned to 2 bytes only."""
    big = _fused(np.random.default_rng(11), dtype_name, fmt)
    for kind, lo, hi in (('cif', 1, 341), ('caf', 341, 1025)):
        n_fields, flip = _head(kind)
        view = big[:, lo:hi]
        if fmt == 'nhwc':
            assert view.data_ptr() % (4 if dtype_name == 'float32' else 2) == 0
            assert view.data_ptr() % (8 if dtype_name == 'float32' else 4) != 0
        out = _check(view, n_fields, kind, 1, flip if flipped else None)
        assert not out.isnan().any()


@pytest.mark.parametrize('fmt', ['nchw', 'nhwc'])
def test_batch_slice(fmt):
    import torch
    n_fields, flip = _head('cif')
    big = _values(np.random.default_rng(13), 'float16', (4, 340, 3, 5))
    big[0] = float('nan')
    big[3] = float('nan')
    if fmt == 'nhwc':
        big = _channels_last(big)
    view = big[1:3]
    assert view.data_ptr() == big.data_ptr() + 2 * big.stride()[0]
    # a batch slice of a dense NCHW tensor is itself dense: nothing but the pointer moves
    out = _check(view, n_fields, 'cif', 1, flip, dense_input=fmt == 'nchw')
    assert not out.isnan().any() and torch.isnan(big[0].float()).all()


@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('fmt', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype_name', ['float32', 'bfloat16'])
def test_spatial_crop(dtype_name, fmt, flipped):
    n_fields, flip = _head('caf')
    big = _values(np.random.default_rng(17), dtype_name, (2, 19 * 9 * 4, 6, 21))
    big[:, :, 0] = float('nan')
    big[:, :, -1] = float('nan')
    big[:, :, :, :2] = float('nan')
    if fmt == 'nhwc':
        big = _channels_last(big)
    view = big[:, :, 1:-1, 2:]
    assert view.shape[2:] == (4, 19)  # two tiles a row: 16 conv pixels and 3
    out = _check(view, n_fields, 'caf', 1, flip if flipped else None)
    assert not out.isnan().any()


def _peak_rise(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


def test_channels_last_makes_no_copy():
    """An 8.3 MiB channels-last float16 conv: the call allocates its output and nothing of
    the conv's size (a .contiguous() copy would add 8.3 MiB)."""
    import torch
    from openpifpaf_amd import heads
    conv = torch.randn((8, 340, 40, 40), device='cuda').to(torch.float16).contiguous(
        memory_format=torch.channels_last)
    assert conv.nbytes >= 8 << 20 and not conv.is_contiguous() and conv.stride()[1] == 1
    out, raised = _peak_rise(lambda: heads.fields_from_conv(conv, 17, 'cif', 1))
    print('peak raised by', raised, 'bytes; out', out.nbytes, 'conv', conv.nbytes)
    assert out.shape == (8, 17, 5, 79, 79)
    assert raised <= out.nbytes + (1 << 20)


def test_channel_slice_makes_no_copy():
    """The same bound for the NCHW channel slice big[:, 1:341] of that size."""
    import torch
    from openpifpaf_amd import heads
    big = torch.randn((8, 341, 40, 40), device='cuda').to(torch.float16)
    conv = big[:, 1:341]
    assert conv.nbytes >= 8 << 20 and not conv.is_contiguous() and conv.stride()[3] == 1
    out, raised = _peak_rise(lambda: heads.fields_from_conv(conv, 17, 'cif', 1))
    print('peak raised by', raised, 'bytes; out', out.nbytes, 'conv', conv.nbytes)
    assert out.shape == (8, 17, 5, 79, 79)
    assert raised <= out.nbytes + (1 << 20)


@pytest.mark.parametrize('flipped', [False, True])
def test_out_field_range_with_channels_last_inputs(flipped):
    """caf (19) + dense caf (25), both channels-last, into one (B, 44, 9, H, W) tensor: the
    two separate ingests of the dense clones, and the other fields keep the sentinel."""
    import torch
    from openpifpaf_amd import heads
    rng = np.random.default_rng(29)
    _, caf_flip = _head('caf')
    _, dense_flip = _head('dense')
    if not flipped:
        caf_flip = dense_flip = None
    caf = _values(rng, 'float32', (2, 19 * 9 * 4, 3, 4))
    dense = _values(rng, 'float32', (2, 25 * 9 * 4, 3, 4))
    assert caf.is_contiguous() and dense.is_contiguous()
    want = torch.cat([heads.fields_from_conv(caf, 19, 'caf', 1, hflip=caf_flip),
                      heads.fields_from_conv(dense, 25, 'caf', 1, hflip=dense_flip)], dim=1)
    caf, dense = _channels_last(caf), _channels_last(dense)
    assert not caf.is_contiguous() and not dense.is_contiguous()
    out = torch.full((2, 44, 9, 5, 7), SENTINEL, dtype=torch.float32, device='cuda')
    res = heads.fields_from_conv(dense, 25, 'caf', 1, hflip=dense_flip, out=out, out_field0=19)
    assert res is out
    assert (out[:, :19] == SENTINEL).all()
    assert _bytes(out[:, 19:].contiguous()) == _bytes(want[:, 19:].contiguous())
    out[:, 19:] = SENTINEL
    heads.fields_from_conv(caf, 19, 'caf', 1, hflip=caf_flip, out=out)
    assert (out[:, 19:] == SENTINEL).all()
    heads.fields_from_conv(dense, 25, 'caf', 1, hflip=dense_flip, out=out, out_field0=19)
    assert _bytes(out) == _bytes(want)


@pytest.mark.parametrize('concat_dense', [False, True])
def test_multi_scale_collector_on_channels_last_bfloat16(concat_dense):
    """n_scales = 2 with the mirrored pass and a dense skeleton: 12 channels-last bfloat16
    conv outputs give, byte for byte, the list their contiguous clones give."""
    import torch
    from openpifpaf_amd import heads
    rng = np.random.default_rng(41)
    specs = [('cif', 17), ('caf', 19), ('caf', 25)]
    dense_convs = [_values(rng, 'bfloat16', (2, n * PER[kind] * 4, 5, 6))
                   for _ in range(4) for kind, n in specs]
    convs = [_channels_last(c) for c in dense_convs]
    assert all(c.is_contiguous() for c in dense_convs)
    assert not any(c.is_contiguous() for c in convs)
    collector = heads.MultiScaleCollector(KPS, SKEL, DENSE, quad=1, n_scales=2,
                                          include_hflip=True, concat_dense=concat_dense)
    want = collector(dense_convs)
    got = collector(convs)
    assert len(got) == len(want) == (8 if concat_dense else 12)
    for g, t in zip(got, want):
        assert g.dtype == torch.float32 and g.shape == t.shape
        assert _bytes(g) == _bytes(t)


def test_unsupported_strides_are_copied_once():
    """A step along both the channels and the columns: fields_from_conv copies the view
    (once: the peak rises by the output and one dense conv), the C call refuses its strides."""
    import torch
    from openpifpaf_amd import _device, heads
    from openpifpaf_amd._lib import load
    b, ch, h, w = 2, 340, 40, 40
    base = torch.full((b, h, ch, 2 * w), float('nan'), device='cuda')
    view = base.permute(0, 2, 1, 3)[..., ::2]
    view.copy_(torch.randn((b, ch, h, w), device='cuda'))
    assert view.shape == (b, ch, h, w) and view.stride() == (h * ch * 2 * w, 2 * w,
                                                             ch * 2 * w, 2)
    clone = view.clone(memory_format=torch.contiguous_format)
    assert clone.is_contiguous() and not view.is_contiguous()
    want = heads.fields_from_conv(clone, 17, 'cif', 1)
    got, raised = _peak_rise(lambda: heads.fields_from_conv(view, 17, 'cif', 1))
    assert _bytes(got) == _bytes(want) and not got.isnan().any()
    print('peak raised by', raised, 'bytes; out', got.nbytes, 'copy', clone.nbytes)
    assert got.nbytes + clone.nbytes <= raised <= got.nbytes + clone.nbytes + (1 << 20)

    lib = load()
    out = torch.full_like(got, SENTINEL)
    rc = lib.pp_fields_from_conv_strided(
        _device.ptr(view), 0, (ctypes.c_int64 * 4)(*view.stride()), b, 17, 0, h, w, 1, 0, None,
        None, _device.ptr(out), 17, 0, _device.stream())
    assert rc == EINVAL
    msg = lib.pp_last_error()
    assert b'channel' in msg and b'column' in msg, msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()  # nothing was launched
