"""Generate tests/golden/heads_hflip.npz by running the REFERENCE's own modules.

Run in the build container only (needs the reference, imported through
oracle/ref_loader.py):
    python tests/golden/gen_heads_hflip.py

What a head of ShellMultiScale's mirrored pass goes through (network/nets.py:133-138,
network/heads.py:145-214), for random conv outputs at quad 0, 1 and 2:
  1. CompositeFieldFused with its conv replaced by the identity, eval mode;
  2. its 5-/6-d tuple split into the list format PifHFlip / PafHFlip index correctly
     ([conf (B,F,H,W), reg1 (B,F,2,H,W), reg2, logb1, logb2, scale1, scale2]);
  3. the reference's PifHFlip / PafHFlip;
  4. the list stacked back into the tuple and the reference's CifCafCollector.
Stored: the conv inputs (float32 values that float16 holds exactly, as float16), the
final float32 fields and the modules' flip_indices /
reverse_direction buffers.  Nothing of the reference is copied.

Precision.  The modules run on the float64 up-conversion of the float32 conv values and
the final fields are rounded to float32 once.  The hflip steps are data movement and a
sign, exact in any type; sigmoid and exp rounded once from float64 are the form
pp_fields_from_conv documents (include/pifpaf_amd.h), so the fixture can be compared bit
for bit.  torch's own float32 sigmoid / exp come within 2 ulp of that (the generator prints how
many elements of a float32 run differ); tests/golden/heads.npz keeps the float32 run
of the unflipped path.

The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'oracle'))

import ref_loader  # noqa: E402  pylint: disable=wrong-import-position
from openpifpaf_amd import constants  # noqa: E402  pylint: disable=wrong-import-position

B, H, W = 2, 4, 5
PER = {'cif': 5, 'caf': 9}


def to_list(res):
    """CompositeFieldFused's (classes, regs, logb, scales) -> the unfused head's list."""
    classes, regs, logb, scales = res
    assert classes.shape[2] == 1
    return ([classes[:, :, 0].clone()] +
            [regs[:, :, v].clone() for v in range(regs.shape[2])] +
            [logb[:, :, v].clone() for v in range(logb.shape[2])] +
            [scales[:, :, v].clone() for v in range(scales.shape[2])])


def to_tuple(lst, n_vec):
    import torch  # pylint: disable=import-outside-toplevel
    return (lst[0][:, :, None].contiguous(),
            torch.stack(lst[1:1 + n_vec], dim=2),
            torch.stack(lst[1 + n_vec:1 + 2 * n_vec], dim=2),
            torch.stack(lst[1 + 2 * n_vec:], dim=2))


def run(heads, metas, flips, convs, quad, dtype):
    import torch  # pylint: disable=import-outside-toplevel
    heads.CompositeFieldFused.quad = quad
    res = {}
    for kind, meta in metas.items():
        head = heads.CompositeFieldFused(meta, 4)
        head.conv = torch.nn.Identity()
        head.eval()
        with torch.no_grad():
            lst = to_list(head(torch.from_numpy(convs[kind]).to(dtype)))
            res[kind] = to_tuple(flips[kind](*lst), meta.n_vectors)
    with torch.no_grad():
        cif, caf = heads.CifCafCollector([0], [1])([res['cif'], res['caf']])
    return cif.float().numpy(), caf.float().numpy()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref_loader.load()
    import torch  # pylint: disable=import-outside-toplevel
    from openpifpaf.network import heads  # pylint: disable=import-outside-toplevel
    from openpifpaf.datasets.constants import HFLIP  # pylint: disable=import-outside-toplevel
    kps, skel = constants.COCO_KEYPOINTS, constants.COCO_PERSON_SKELETON
    metas = {'cif': heads.IntensityMeta('cif', kps, [0.05] * 17, None),
             'caf': heads.AssociationMeta('caf', kps, [0.05] * 17, None, skel)}
    flips = {'cif': heads.PifHFlip(kps, HFLIP), 'caf': heads.PafHFlip(kps, skel, HFLIP)}
    out = {
        'cif_flip_indices': flips['cif'].flip_indices.numpy().astype(np.int32),
        'caf_flip_indices': flips['caf'].flip_indices.numpy().astype(np.int32),
        'caf_reverse_direction': flips['caf'].reverse_direction.numpy().astype(np.int32),
    }
    rng = np.random.default_rng(23)
    for quad in (0, 1, 2):
        # on a 1/16 grid: as good as any values for data movement, exact in float16 (which
        # is how they are stored) and the archive deflates
        convs = {kind: (np.round(32.0 * rng.standard_normal(
            (B, meta.n_fields * PER[kind] * 4 ** quad, H, W))) / 16.0).astype(np.float32)
                 for kind, meta in metas.items()}
        cif, caf = run(heads, metas, flips, convs, quad, torch.float64)
        cif32, caf32 = run(heads, metas, flips, convs, quad, torch.float32)
        for kind, a, a32 in (('cif', cif, cif32), ('caf', caf, caf32)):
            assert np.array_equal(convs[kind].astype(np.float16).astype(np.float32), convs[kind])
            out['q%d_%s_conv' % (quad, kind)] = convs[kind].astype(np.float16)
            out['q%d_%s' % (quad, kind)] = a
            ulp = np.abs(a.view(np.int32).astype(np.int64) - a32.view(np.int32).astype(np.int64))
            print('quad', quad, kind, a.shape, 'float32 run differs in', int((ulp > 0).sum()),
                  'of', a.size, 'elements, max', int(ulp.max()), 'ulp')
    heads.CompositeFieldFused.quad = 1
    save_npz(os.path.join(HERE, 'heads_hflip.npz'), out)


if __name__ == '__main__':
    main()
