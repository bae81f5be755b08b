"""Generate tests/golden/enc_<case>.npz by running the REFERENCE's encoders
(openpifpaf/encoder/cif.py, caf.py, annrescaler.py).

Run in the build container only (needs the reference):
    python tests/golden/gen_encoder.py

Nothing of the reference is copied: a fixture holds what the encoders were given (pixel
size, annotations, meta, every option) and the tensors they returned, for every case of
tests/encoder_util.py at strides 4, 8 and 16, as compressed arrays.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))

# the reference uses aliases that NumPy has removed.  NumPy 2 has np.bool back (as np.bool_);
# replacing that one by the builtin breaks numpy.ma, so each is defined only where missing
for _alias, _type in (('int', int), ('bool', bool)):
    if not hasattr(np, _alias):
        setattr(np, _alias, _type)

import encoder_util  # noqa: E402  pylint: disable=wrong-import-position
import ref_loader  # noqa: E402  pylint: disable=wrong-import-position


class NoVisualizer:
    def processed_image(self, image):
        pass

    def targets(self, fields, *, keypoint_sets):
        pass


def main():
    ref_loader.load()
    from openpifpaf import encoder as ref_encoder  # pylint: disable=import-outside-toplevel
    for name in encoder_util.NAMES:
        c = encoder_util.case(name)
        h, w = c['size']
        image = np.zeros((3, h, w), np.float32)
        kps = [a['keypoints'] for a in c['anns']]
        out = {
            'size': np.array([h, w]),
            'ann_keypoints': np.stack(kps) if kps else np.zeros((0, c['k'], 3), np.float32),
            'ann_bbox': (np.stack([a['bbox'] for a in c['anns']]) if kps
                         else np.zeros((0, 4), np.float32)),
            'ann_iscrowd': np.array([a['iscrowd'] for a in c['anns']], bool),
            'k': np.array(c['k']), 'pose': np.array(c['pose'], np.float64),
            'has_sigmas': np.array(c['sigmas'] is not None),
            'sigmas': np.array(c['sigmas'] if c['sigmas'] is not None else [], np.float64),
            'skeleton': np.array(c['skeleton'], np.int32),
            'sparse_skeleton': np.array(c['sparse_skeleton'] or [], np.int32).reshape(-1, 2),
            'dense_to_sparse_radius': np.array(c['dense_to_sparse_radius']),
            'only_in_field_of_view': np.array(c['only_in_field_of_view']),
            'v_threshold': np.array(c['v_threshold']),
            'side': np.array(-1 if c['side'] is None else c['side']),
            'fixed_size': np.array(c['fixed_size']), 'has_cif': np.array(c['cif']),
            'strides': np.array(encoder_util.STRIDES),
        }
        if c['valid_area'] is not None:
            out['valid_area'] = np.array(c['valid_area'], np.float64)
        for stride in encoder_util.STRIDES:
            cif, caf = encoder_util.encoders(c, stride, ref_encoder)
            out['s%d_pose_45' % stride] = caf.rescaler.pose_45
            for enc, keys in ((cif, encoder_util.CIF_KEYS), (caf, encoder_util.CAF_KEYS)):
                if enc is None:
                    continue
                enc.visualizer = NoVisualizer()
                fresh = encoder_util.case(name)
                fields = enc(image, fresh['anns'], fresh['meta'])
                assert len(fields) == len(keys)
                for key, t in zip(keys, fields):
                    t = t.numpy()
                    assert t.dtype == np.float32
                    out['s%d_%s' % (stride, key)] = np.ascontiguousarray(t)
        path = encoder_util.fixture_path(name)
        np.savez_compressed(path, **out)
        print('{}: {} bytes'.format(os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
