"""The un-flip of a mirrored pass's head as exact NumPy data movement on the conv output
(heads.PifHFlip / PafHFlip on the unfused head's list, network/heads.py:145-214), so that
`oracle.fields_from_conv(compose(conv, ...), ..., quad=0)` is what the device ingest with
`hflip` and the original `quad` must give.  Test infrastructure."""
import numpy as np

META = {'cif': (1, 1, 1), 'caf': (1, 2, 2), 'cifdet': (1, 2, 0)}  # n_conf, n_vec, n_scales
PER = {'cif': 5, 'caf': 9, 'cifdet': 7}


def dequad(conv, quad):
    """`quad` times PixelShuffle(2), then [:, :, :-1, :-1] (heads.py:410-411)."""
    x = np.asarray(conv)
    for _ in range(quad):
        b, c, h, w = x.shape
        x = x.reshape(b, c // 4, 2, 2, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(
            b, c // 4, 2 * h, 2 * w)[:, :, :-1, :-1]
    return np.ascontiguousarray(x)


def compose(conv, n_fields, kind, quad, src_field=None, swap_ends=None, mirror=True):
    """conv (B, n_fields * per * 4^quad, h, w) -> the quad-0 conv (B, n_fields * per, H, W)
    whose plain ingest equals the un-flipped fields."""
    nc, nv, ns = META[kind]
    x = dequad(conv, quad)
    b, _, h, w = x.shape
    f0, f1, f2 = nc * n_fields, (nc + 2 * nv) * n_fields, (nc + 3 * nv) * n_fields
    conf = x[:, :f0].reshape(b, n_fields, nc, h, w).copy()
    vec = x[:, f0:f1].reshape(b, n_fields, nv, 2, h, w).copy()
    logb = x[:, f1:f2].reshape(b, n_fields, nv, h, w).copy()
    scale = x[:, f2:].reshape(b, n_fields, ns, h, w).copy()
    parts = [conf, vec, logb, scale]
    if src_field is not None:
        parts = [p[:, list(src_field)] for p in parts]
    if mirror:
        parts = [p[..., ::-1].copy() for p in parts]
        if kind == 'cifdet':  # only the vector the index grid is added to
            parts[1][:, :, 0, 0] *= np.float32(-1.0)
        else:
            parts[1][:, :, :, 0] *= np.float32(-1.0)
    if swap_ends is not None:
        assert kind == 'caf'
        for f, s in enumerate(swap_ends):
            if s:
                parts[1][:, f] = parts[1][:, f, ::-1].copy()
    return np.ascontiguousarray(
        np.concatenate([p.reshape(b, -1, h, w) for p in parts], axis=1))
