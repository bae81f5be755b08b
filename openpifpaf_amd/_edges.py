"""Column sets and query tables of the batched connection_value / p2p_value entry points
(pp_connection_values, pp_p2p_values; csrc/edges.hip), shared by `functional`,
`functional_cpu` and the CifCaf members."""
import numpy as np
import torch

from ._abi import EDGE_QUERY_DTYPE, EXP_MODES


class PackedSets:
    """n_sets column sets in one buffer, the layout pp_caf_scored writes: `cols`
    (n_sets, 9, cap) float32 and `counts` (n_sets) int32, both NumPy arrays or both device
    tensors.  Set i holds cols[i, :, :counts[i]].  For a CafScored, set 2 * caf_i is the
    backward and 2 * caf_i + 1 the forward set, so the opposite direction of set s is s ^ 1."""

    def __init__(self, cols, counts):
        if cols.ndim != 3 or cols.shape[1] != 9 or counts.shape != (cols.shape[0],):
            raise ValueError('packed column sets need (n_sets, 9, cap) columns and (n_sets) '
                             'counts')
        self.cols = cols
        self.counts = counts

    @property
    def n_sets(self):
        return int(self.cols.shape[0])

    @property
    def cap(self):
        return int(self.cols.shape[2])

    @property
    def on_device(self):
        return isinstance(self.cols, torch.Tensor)


def _host_set(s):
    if isinstance(s, torch.Tensor):
        s = s.detach().cpu().numpy()
    s = np.asarray(s, dtype=np.float32)
    if s.ndim != 2 or s.shape[0] != 9:
        raise ValueError('a column set must have shape (9, N), got {}'.format(s.shape))
    return s


def pack_sets(sets, device=None):
    """PackedSets of a list of (9, N) arrays (NumPy or torch, converted to float32); `device`:
    a torch device to pack there (device tensors are copied on the device), None = host."""
    if isinstance(sets, PackedSets):
        if device is None:
            if not sets.on_device:
                return sets
            return PackedSets(sets.cols.cpu().numpy(), sets.counts.cpu().numpy())
        if sets.on_device:
            return sets
        return PackedSets(torch.from_numpy(np.ascontiguousarray(sets.cols)).to(device),
                          torch.from_numpy(np.ascontiguousarray(sets.counts)).to(device))
    sets = list(sets)
    for s in sets:
        if len(s.shape) != 2 or s.shape[0] != 9:
            raise ValueError('a column set must have shape (9, N), got {}'.format(tuple(s.shape)))
    counts = np.array([int(s.shape[1]) for s in sets], np.int32)
    cap = max(1, int(counts.max()) if len(sets) else 1)
    if device is not None and any(isinstance(s, torch.Tensor) and s.is_cuda for s in sets):
        cols = torch.zeros((len(sets), 9, cap), dtype=torch.float32, device=device)
        for i, s in enumerate(sets):
            if counts[i]:
                cols[i, :, :counts[i]] = torch.as_tensor(s).to(device=device, dtype=torch.float32)
        return PackedSets(cols, torch.from_numpy(counts).to(device))
    cols = np.zeros((len(sets), 9, cap), np.float32)
    for i, s in enumerate(sets):
        cols[i, :, :counts[i]] = _host_set(s)
    if device is None:
        return PackedSets(cols, counts)
    return PackedSets(torch.from_numpy(cols).to(device), torch.from_numpy(counts).to(device))


def caf_scored_sets(caf_scored, n_caf, device=None):
    """PackedSets of anything with the reference's directed(caf_i, forward) -> two (9, N)
    arrays: sets 2 * caf_i (backward) and 2 * caf_i + 1 (forward).  A CafScored of this
    package that one fill produced on the device hands out its own buffer."""
    packed = getattr(caf_scored, 'packed', None)
    sets = []
    for caf_i in range(n_caf):
        fwd, bwd = caf_scored.directed(caf_i, True)
        sets += [bwd, fwd]
    # (its lists are views of that buffer; one that a caller replaced is repacked)
    if (device is not None and isinstance(packed, PackedSets) and packed.on_device and
            packed.n_sets == len(sets) and
            all(isinstance(s, torch.Tensor) and s.data_ptr() == packed.cols[i].data_ptr()
                for i, s in enumerate(sets))):
        return packed
    return pack_sets(sets, device)


def queries(sources, set_index, targets=None):
    """The pp_edge_query table of sources (n, 4) = (x, y, v, scale), set_index (n) and,
    for p2p, targets (n, 3) = (x, y, scale); everything converted to float32 / int32."""
    sources = np.asarray(sources, dtype=np.float32).reshape(-1, 4)
    set_index = np.asarray(set_index).reshape(-1)
    if len(set_index) != len(sources):
        raise ValueError('{} set indices for {} sources'.format(len(set_index), len(sources)))
    q = np.zeros(len(sources), EDGE_QUERY_DTYPE)
    q['x'], q['y'], q['v'], q['s'] = sources.T
    q['set'] = set_index
    if targets is not None:
        targets = np.asarray(targets, dtype=np.float32).reshape(-1, 3)
        if len(targets) != len(sources):
            raise ValueError('{} targets for {} sources'.format(len(targets), len(sources)))
        q['tx'], q['ty'], q['ts'] = targets.T
    return q


def check_sets(q, n_sets):
    if len(q) and (q['set'].min() < 0 or q['set'].max() >= n_sets):
        raise ValueError('query set index outside [0, {})'.format(n_sets))


def method_bits(connection_method, exp_mode):
    """The `method` argument of pp_grow_connection and the edge entry points."""
    method = {'blend': 0, 'max': 1}.get(connection_method)
    if method is None:
        raise Exception('connection method not known')
    if exp_mode not in EXP_MODES:
        raise ValueError('exp_mode must be one of {}'.format(sorted(EXP_MODES)))
    return method | (EXP_MODES[exp_mode] << 1)


def annotation_table(anns, n_keypoints=None):
    """(n, K, 4) float32 = (x, y, v, joint scale) per joint of a list of annotations."""
    if not anns:
        return np.zeros((0, n_keypoints or 0, 4), np.float32)
    data = np.stack([np.asarray(a.data, dtype=np.float32) for a in anns])
    scales = np.stack([np.asarray(a.joint_scales, dtype=np.float32) for a in anns])
    return np.concatenate([data, scales[:, :, None]], axis=2)


def connection_queries(table, skeleton_m1):
    """Every directed skeleton edge of every annotation: (n_ann * 2C) queries, per CAF the
    forward edge (j1 -> j2, set 2 caf_i + 1) then the backward one (j2 -> j1, set 2 caf_i)."""
    skel = np.asarray(skeleton_m1, dtype=np.int64).reshape(-1, 2)
    starts = skel.reshape(-1)                        # j1, j2 per CAF
    sets = (2 * np.arange(len(skel))[:, None] + np.array([1, 0])).reshape(-1)
    src = table[:, starts, :]                        # (n, 2C, 4)
    return queries(src.reshape(-1, 4), np.tile(sets, len(table)))


def p2p_queries(src_table, tgt_table, skeleton_m1):
    """Every source annotation against every target annotation over every directed edge:
    (n_src * n_tgt * C * 2) queries, [.., c, 0] forward (source j1, target j2), [.., c, 1]
    backward (source j2, target j1)."""
    skel = np.asarray(skeleton_m1, dtype=np.int64).reshape(-1, 2)
    n_s, n_t, c = len(src_table), len(tgt_table), len(skel)
    starts = skel.reshape(-1)
    ends = skel[:, ::-1].reshape(-1)
    sets = (2 * np.arange(c)[:, None] + np.array([1, 0])).reshape(-1)
    src = np.broadcast_to(src_table[:, None, starts, :], (n_s, n_t, 2 * c, 4))
    tgt = np.broadcast_to(tgt_table[None, :, ends, :][..., [0, 1, 3]], (n_s, n_t, 2 * c, 3))
    return queries(src.reshape(-1, 4), np.tile(sets, n_s * n_t), tgt.reshape(-1, 3))
