"""Reject inconsistent loop closures before pose-graph optimisation, on the device.

Every loop that passes the per-pair thresholds of verify.* becomes an edge of the graph, and a wrong one -- a repeated street front
aligned cleanly at the wrong place -- bends the whole drive: Huber's cost is convex, a gross loop still pulls with constant force.  The
cure is pairwise-consistency maximisation (Mangelson et al., ICRA 2018): two loops agree if the cycle through both and the odometry
between their ends closes within its uncertainty; a large set of mutually agreeing loops is kept and the rest dropped
(csrc/lpd_loops.hip; the definition is in include/lpd_hip.h).

    lp = posegraph.loop_edges(rf, pairs)                                           # (edge [P, 2], meas [P, 12], weight [P, 2])
    sel = consistency.consistent_loops(node_poses, lp)                             # LoopConsistency
    sel.accepted, sel.adjacency, sel.degree, sel.info                              # [P] bool, [P, ldw] int64, [P] int32, [8] int32
    res = posegraph.PoseGraph(node_poses, od, consistency.filter_loops(lp, sel.accepted)).optimize()
    res = posegraph.close_loops(sub, poses, rf, pairs, consistent=True)            # the same, in one call; res.selection = sel

Every launch gives the same bits, equal to the numpy restatement (tests/loops_ref.py).  Nothing is read back.  No CPU fallback.
"""
import math

import torch

from . import ops, posegraph
from .verify import _Frozen


class ConsistencySearch(_Frozen):
    """The selection of consistent_loops, validated and frozen.  gate: a pair of loops is consistent iff its statistic is <= gate (the
    default is the 0.99 quantile of chi-squared with 6 degrees of freedom); seeds: the greedy search starts from the `seeds` loops of the
    largest degree, 1 .. 64; min_size: a winning set smaller than this accepts nothing."""
    __slots__ = ("gate", "seeds", "min_size")

    def __init__(self, gate=16.81, seeds=8, min_size=3):
        if isinstance(gate, bool) or not isinstance(gate, (int, float)) or not 0.0 <= float(gate) < math.inf:
            raise ValueError(f"ConsistencySearch: gate={gate!r} (a finite number >= 0)")
        self._set("gate", float(gate))
        self._set("seeds", self._whole(seeds, "seeds", 1, ops.LOOPS_MAX_SEEDS))
        self._set("min_size", self._whole(min_size, "min_size", 1, ops.LOOPS_MAX))


class LoopConsistency:
    """What consistent_loops returns, all on the device: accepted [P] bool = the loops to keep; adjacency [P, ldw] int64 = the bit rows of
    the consistency matrix (the uint64 words' bit patterns: bit b & 63 of word b >> 6 of row a, local loop numbers); degree [P] int32 =
    a row's popcount, -1 for an invalid loop; info [8] int32 ([G, 8] with offsets) = (status, loops valid, loops chosen, seeds run, the
    winning seed's loop, consistent pairs, 0, 0)."""
    __slots__ = ("accepted", "adjacency", "degree", "info")

    def __init__(self, accepted, adjacency, degree, info):
        self.accepted, self.adjacency, self.degree, self.info = accepted, adjacency, degree, info

    @property
    def ok(self):
        return self.info[..., 0] == ops.LOOPS_OK


def _loops(what, loops):
    if not isinstance(loops, (tuple, list)) or len(loops) != 3 or not all(isinstance(t, torch.Tensor) for t in loops):
        raise TypeError(f"{what}: loops must be the tuple (edge, meas, weight) of posegraph.loop_edges")
    return tuple(loops)


def consistent_loops(node_poses, loops, odometry_weights=posegraph.ODOMETRY_WEIGHTS, search=ConsistencySearch(), node_off=None, loop_off=None):
    """The pairwise-consistent loops of a drive -> LoopConsistency.  node_poses [V, 12], [V, 3, 4] or [V, 4, 4] float64 on the device =
    the nodes' start (consecutive windows, as posegraph.odometry_edges links them); loops = (edge, meas, weight) of
    posegraph.loop_edges; odometry_weights = (w_rot, w_trans) > 0 of one odometry step; node_off, loop_off: None for one drive, or G + 1
    offsets as ops.loop_consistency takes them.  Two launches' worth of work is enqueued; nothing is read back."""
    what = "consistent_loops"
    poses = posegraph._node_poses(what, node_poses)
    edge, meas, weight = _loops(what, loops)
    if not isinstance(search, ConsistencySearch):
        raise TypeError(f"{what}: search must be a ConsistencySearch, got {type(search).__name__}")
    if not isinstance(odometry_weights, (tuple, list)) or len(odometry_weights) != 2:
        raise ValueError(f"{what}: odometry_weights is (w_rot, w_trans)")
    w_or, w_ot, gate = ops.loop_params(odometry_weights[0], odometry_weights[1], search.gate)
    adj, degree = ops.loop_consistency(poses, edge, meas, weight, w_or, w_ot, gate, node_off=node_off, loop_off=loop_off)
    accepted, info = ops.loop_select(adj, degree, loop_off=loop_off, seeds=search.seeds, min_size=search.min_size)
    return LoopConsistency(accepted.to(torch.bool), adj, degree, info[0] if loop_off is None else info)


def filter_loops(loops, accepted):
    """(edge, meas, weight) with the nodes of every loop that is not accepted set to -1: lpd_pgo_solve skips it, and no shape depends on
    the selection.  accepted [P] bool or uint8."""
    what = "filter_loops"
    edge, meas, weight = _loops(what, loops)
    if not isinstance(accepted, torch.Tensor) or accepted.dtype not in (torch.bool, torch.uint8) or tuple(accepted.shape) != (edge.shape[0],):
        raise ValueError(f"{what}: accepted must be a bool or uint8 tensor [P] = ({edge.shape[0]},)")
    keep = accepted.to(torch.bool)[:, None]
    return torch.where(keep, edge, torch.full_like(edge, -1)), meas, weight
