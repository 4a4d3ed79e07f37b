"""Place lists from positions on the device: which submaps are the same place, decided from their (northing, easting) alone by
ops.radius_lists (lpd_radius_count / lpd_radius_fill; definition in include/lpd_hip.h).

Replaces the reference's generating_queries/ scripts, which run sklearn KDTree.query_radius searches on the host and pickle Python
dicts: generate_training_tuples_baseline.py:52-72 (positives at 10 m, non-negatives at 50 m) and generate_test_sets.py:99-109 (the
truth lists of the evaluation at 25 m).  With this module a training or evaluation run needs the clouds and a [T, 2] array of
positions:

    lists = training_lists(positions)                              # PlaceLists: two device CSRs + host lengths
    bank  = TupleBank.from_positions(clouds, positions)            # the same, installed in a tuple bank
    keep  = in_test_regions(positions, centres)                    # the reference's train / test split, centres are the caller's
    truth = evaluation_truth(db_positions, query_positions)        # TruthTable: goes where QUERY_SETS went (harness.evaluate_*)

Positions are float64: at a UTM northing of 5.7e6 an fp32 ulp is half a metre.  There is no CPU path: the lists come from the kernel.
"""
import numpy as np
import torch

from . import ops
from ._lib import LpdHipError


def _device(device, what):
    if device is None and not torch.cuda.is_available():
        raise LpdHipError(f"{what}: no GPU visible; the place lists come from the MI355X kernel (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise LpdHipError(f"{what}: device {dev}; the place lists come from the MI355X kernel (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _positions(p, what):
    a = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: positions must be [n, 2] (northing, easting), got {a.shape}")
    return a


def in_test_regions(positions, centres, x_width=150, y_width=150):
    """The reference's check_in_test_set (generate_test_sets.py:37-43) for every row of positions [n, 2] -> numpy bool [n]: inside
    ANY of the rectangles centre +- (x_width, y_width), with the reference's strict inequalities (a point exactly on an edge is
    outside).  centres [k, 2] are the caller's: the package ships no coordinates."""
    pos = _positions(positions, "in_test_regions")
    cen = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    inside = np.zeros(pos.shape[0], dtype=bool)
    for cx, cy in cen:
        inside |= (cx - x_width < pos[:, 0]) & (pos[:, 0] < cx + x_width) & (cy - y_width < pos[:, 1]) & (pos[:, 1] < cy + y_width)
    return inside


class PlaceLists:
    """positives[i] (within pos_radius, i itself removed) and near[i] (within near_radius, i kept) of T items as two device CSRs
    (int32 off [T+1], idx; rows ascending) plus host length arrays (int64 [T]), in the form TupleBank keeps them."""

    def __init__(self, T, pos_off, pos_idx, pos_len, near_off, near_idx, near_len, pos_radius, near_radius):
        self.T, self.pos_radius, self.near_radius = int(T), float(pos_radius), float(near_radius)
        self.pos_off, self.pos_idx, self.pos_len = pos_off, pos_idx, pos_len
        self.near_off, self.near_idx, self.near_len = near_off, near_idx, near_len
        self.max_pos = int(pos_len.max()) if self.T else 0
        self.max_near = int(near_len.max()) if self.T else 0

    def __len__(self):
        return self.T

    def to_lists(self):
        """-> (positives, near): two lists of T ascending int64 arrays (reads the CSRs back)"""
        out = []
        for off, idx in ((self.pos_off, self.pos_idx), (self.near_off, self.near_idx)):
            o, i = off.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
            out.append([i[o[t]:o[t + 1]] for t in range(self.T)])
        return out[0], out[1]


def training_lists(positions, pos_radius=10.0, near_radius=50.0, device=None):
    """construct_query_dict's two searches (generate_training_tuples_baseline.py:52-60) -> PlaceLists.  positions [T, 2] float64
    (host or device); two count / fill launch pairs, one read-back of a total each, and the row lengths (4 T bytes each) for the
    host length arrays."""
    dev = _device(device, "training_lists")
    if isinstance(positions, torch.Tensor) and positions.is_cuda:
        pos = positions.to(dev, torch.float64)
        if pos.dim() != 2 or pos.shape[1] != 2:
            raise ValueError(f"training_lists: positions must be [T, 2], got {tuple(pos.shape)}")
    else:
        pos = torch.from_numpy(_positions(positions, "training_lists")).to(dev)
    T = pos.shape[0]
    with torch.cuda.device(dev):
        me = torch.arange(T, dtype=torch.int32, device=dev)
        p_off, p_idx, p_cnt = ops.radius_lists(pos, pos, pos_radius, self_item=me)
        n_off, n_idx, n_cnt = ops.radius_lists(pos, pos, near_radius)
        lens = torch.stack((p_cnt, n_cnt)).cpu().numpy().astype(np.int64)
    return PlaceLists(T, p_off, p_idx, lens[0], n_off, n_idx, lens[1], pos_radius, near_radius)


class TruthTable:
    """The truth lists of an evaluation on the device, in the layout of harness.build_truth_csr: row g * n_db_runs + m of
    (truth_off, truth_idx) holds the items of database run m within the radius of global query g = sum(q_counts[:n]) + i, as
    ascending row numbers inside run m; the rows of a query's own run are empty (generate_test_sets.py:102).  harness.evaluate_pairs,
    evaluate_from_descriptors and evaluate_model take it in place of QUERY_SETS.  len() = number of runs."""

    def __init__(self, truth_off, truth_idx, q_counts, n_db_runs, radius):
        self.truth_off, self.truth_idx = truth_off, truth_idx
        self.q_counts = [int(c) for c in q_counts]
        self.n_db_runs, self.radius = int(n_db_runs), float(radius)

    def __len__(self):
        return len(self.q_counts)

    def to_query_sets(self):
        """The reference's nested layout, for small cases: QUERY_SETS[n][i][m] = list of row numbers (m != n; the own run has no
        entry, as in the reference's pickles).  O(queries x runs) Python objects."""
        off, idx = self.truth_off.cpu().numpy(), self.truth_idx.cpu().numpy()
        sets, g = [], 0
        for n, cnt in enumerate(self.q_counts):
            run = {}
            for i in range(cnt):
                row = (g + i) * self.n_db_runs
                run[i] = {m: idx[off[row + m]:off[row + m + 1]].tolist() for m in range(self.n_db_runs) if m != n}
            sets.append(run)
            g += cnt
        return sets


def evaluation_truth(db_positions, query_positions, radius=25.0, device=None):
    """generate_test_sets.py:99-109 -> TruthTable.  db_positions / query_positions: lists with one [n, 2] array per run (the queries
    of run n are the reference's test subset of run n: in_test_regions picks them); every query is searched in every OTHER run's
    database.  One count / fill launch pair over all (query, run) rows."""
    dev = _device(device, "evaluation_truth")
    if len(db_positions) != len(query_positions) or len(db_positions) < 1:
        raise ValueError(f"evaluation_truth: {len(db_positions)} database runs, {len(query_positions)} query runs (equal, >= 1)")
    db = [_positions(p, f"evaluation_truth: db_positions[{m}]") for m, p in enumerate(db_positions)]
    qs = [_positions(p, f"evaluation_truth: query_positions[{n}]") for n, p in enumerate(query_positions)]
    seg = np.zeros(len(db) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for a in db], out=seg[1:])
    q_counts = [a.shape[0] for a in qs]
    own = np.repeat(np.arange(len(qs), dtype=np.int32), q_counts)
    with torch.cuda.device(dev):
        off, idx, _ = ops.radius_lists(torch.from_numpy(np.concatenate(qs)).to(dev), torch.from_numpy(np.concatenate(db)).to(dev), radius,
                                       seg_off=seg.tolist(), skip_seg=torch.from_numpy(own).to(dev))
    return TruthTable(off, idx, q_counts, len(db), radius)


def to_queries_dict(lists, files):
    """PlaceLists -> the reference's pickle layout {i: {'query': files[i], 'positives': [...], 'negatives': [...]}} for tools that
    still read it: positives sorted, negatives = [0, T) without near[i], sorted (the reference shuffles them; its consumers shuffle
    again).  O(T^2) Python ints, like the reference's: about 21 k per item at T = 21711.  Interop only; TupleBank.from_positions needs
    none of it."""
    if len(files) != lists.T:
        raise ValueError(f"to_queries_dict: {lists.T} items, {len(files)} file names")
    positives, near = lists.to_lists()
    out, mask = {}, np.empty(lists.T, dtype=bool)
    for i in range(lists.T):
        mask[:] = True
        mask[near[i]] = False
        out[i] = {"query": files[i], "positives": positives[i].tolist(), "negatives": np.nonzero(mask)[0].tolist()}
    return out
