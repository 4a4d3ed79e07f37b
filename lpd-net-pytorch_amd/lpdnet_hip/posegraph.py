"""Pose-graph optimisation of a drive from its loop closures, on the device.

verify.refine_pairs ends with a relative 6-DoF pose between two windows of a drive: a loop-closure constraint.  This module is the
back end that uses it: a graph whose nodes are the windows' reference poses, whose edges are the odometry between consecutive windows
(from the input poses) and the verified loops, optimised by Levenberg-Marquardt around preconditioned conjugate gradients in one launch
(csrc/lpd_pgo.hip; the definition is in include/lpd_hip.h).  The corrected positions go where the uncorrected ones went.

    sub, positions = drive.submaps_from_drive(points, lengths, poses)             # frame="reference"
    rf = verify.refine_pairs(sub, sub, pairs, init=verify.align_pairs(sub, sub, pairs))
    res = posegraph.close_loops(sub, poses, rf, pairs)                             # PoseGraphResult
    res.poses, res.positions, res.cost, res.chi2, res.info, res.converged         # [V, 3, 4], [V, 2], [outer + 1], [E], [8], bool
    places.training_lists(res.positions, ...); TupleBank.from_positions(..., res.positions, ...)

    od = posegraph.odometry_edges(node_poses)                                      # (edge [V-1, 2], meas [V-1, 12], weight [V-1, 2])
    lp = posegraph.loop_edges(rf, pairs)                                           # pair (a, b) -> edge (i = b, j = a, Z = rf.matrix())
    res = posegraph.PoseGraph(node_poses, od, lp).optimize(outer=20, huber=3.0)
    res = posegraph.close_loops(sub, poses, rf, pairs, consistent=True)            # only a pairwise-consistent set of the loops (consistency.py)

Every launch gives the same bits, equal to the numpy restatement (tests/pgo_ref.py).  Nothing is read back.  No CPU fallback.
"""
import numpy as np
import torch

from . import ops, verify

ODOMETRY_WEIGHTS = (1.0e4, 1.0e2)      # 1 / (0.01 rad)^2, 1 / (0.1 m)^2
LOOP_WEIGHTS = (1.0e4, 1.0e2)


def _weights(what, w_rot, w_trans):
    out = []
    for v, name in ((w_rot, "w_rot"), (w_trans, "w_trans")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) < float("inf"):
            raise ValueError(f"{what}: {name}={v!r} (a finite number >= 0)")
        out.append(float(v))
    return out


def _node_poses(what, poses):
    """[V, 12], [V, 3, 4] or [V, 4, 4] float64 tensor -> the [V, 12] view; no device is looked at"""
    if not isinstance(poses, torch.Tensor) or poses.dtype != torch.float64:
        raise TypeError(f"{what}: poses must be a float64 tensor")
    if poses.dim() == 3 and tuple(poses.shape[1:]) in ((3, 4), (4, 4)):
        poses = poses[:, :3, :].reshape(poses.shape[0], 12)
    if poses.dim() != 2 or poses.shape[1] != 12:
        raise ValueError(f"{what}: poses must be [V, 12], [V, 3, 4] or [V, 4, 4], got {tuple(poses.shape)}")
    return poses


def _inverse_times(X, Y):
    """[.., 12] = X^-1 Y of poses [.., 12] (torch on the device; the measurement of an odometry edge)"""
    Rx, tx = X.reshape(-1, 3, 4)[:, :, :3], X.reshape(-1, 3, 4)[:, :, 3]
    Ry, ty = Y.reshape(-1, 3, 4)[:, :, :3], Y.reshape(-1, 3, 4)[:, :, 3]
    R = Rx.transpose(1, 2) @ Ry
    t = (Rx.transpose(1, 2) @ (ty - tx)[:, :, None])[:, :, 0]
    return torch.cat((R, t[:, :, None]), dim=2).reshape(-1, 12)


def odometry_edges(poses, offsets=None, w_rot=ODOMETRY_WEIGHTS[0], w_trans=ODOMETRY_WEIGHTS[1]):
    """The edges between consecutive nodes, Z = X_k^-1 X_{k+1}, made on the device -> (edge [V-1, 2] int32, meas [V-1, 12] float64,
    weight [V-1, 2] float64).  offsets: a host sequence of run offsets rising from 0 to V; an edge never crosses a run boundary (its
    nodes are -1 there: the solver skips it, and the shapes do not depend on the runs)."""
    what = "odometry_edges"
    poses = _node_poses(what, poses)
    w = _weights(what, w_rot, w_trans)
    V = poses.shape[0]
    if V < 1:
        raise ValueError(f"{what}: no node")
    if offsets is not None:
        offsets = [int(v) for v in offsets]
        if len(offsets) < 2 or offsets[0] != 0 or offsets[-1] != V or any(b < a for a, b in zip(offsets, offsets[1:])):
            raise ValueError(f"{what}: offsets must rise from 0 to V = {V}")
    ops._req(poses, "poses", torch.float64)
    dev = poses.device
    k = torch.arange(V - 1, device=dev, dtype=torch.int32)
    edge = torch.stack((k, k + 1), dim=1)
    if offsets is not None and len(offsets) > 2 and V > 1:
        last = torch.tensor([b - 1 for b in offsets[1:-1] if 0 < b < V], dtype=torch.int64, device=dev)      # k whose k + 1 starts a run
        edge[last] = -1
    meas = _inverse_times(poses[:-1], poses[1:])
    weight = torch.tensor(w, dtype=torch.float64, device=dev).repeat(V - 1, 1)
    return edge, meas, weight


def _is_reference(sub):
    return getattr(sub, "frame", None) == "reference"


def loop_edges(refinement, pairs, accepted=None, w_rot=LOOP_WEIGHTS[0], w_trans=LOOP_WEIGHTS[1]):
    """Loop-closure edges from verify.refine_pairs' Refinement (pairs [P, 2] = (row of a, row of b), both rows of ONE drive's submaps)
    or from refine_candidates' Verification (pairs = its topk_idx [Q, K]: query i against row topk_idx[i, r]) -> (edge [P, 2] int32,
    meas [P, 12] float64, weight [P, 2] float64).  matrix() takes A's frame into B's, so pair (a, b) is the edge (i = b, j = a, Z =
    matrix()): this holds for submaps in their reference scans' frames (drive.submaps_from_drive(frame="reference")).  accepted [P]
    (or [Q, K]) bool, default the Verification's own: a pair that is not valid or not accepted gets the nodes (-1, -1) and is skipped
    by the solver."""
    what = "loop_edges"
    w = _weights(what, w_rot, w_trans)
    if isinstance(refinement, verify.Verification):
        if refinement.refinement is None:
            raise ValueError(f"{what}: the Verification carries no refinement (verify.refine_candidates makes one)")
        if accepted is None:
            accepted = refinement.accepted
        refinement = refinement.refinement
    if not isinstance(refinement, verify.Refinement):
        raise TypeError(f"{what}: expected a verify.Refinement or a Verification with .refinement, got {type(refinement).__name__}")
    if not isinstance(pairs, torch.Tensor) or pairs.dtype not in (torch.int32, torch.int64) or pairs.dim() != 2:
        raise TypeError(f"{what}: pairs must be a [P, 2] (or [Q, K]) int32 or int64 tensor")
    lead = tuple(refinement.valid.shape)
    if len(lead) == 2:
        if tuple(pairs.shape) != lead:
            raise ValueError(f"{what}: the refinement is shaped {lead}; pairs must be the [Q, K] candidates, got {tuple(pairs.shape)}")
    elif tuple(pairs.shape) != lead + (2,):
        raise ValueError(f"{what}: the refinement holds {lead} pairs; pairs must be [P, 2], got {tuple(pairs.shape)}")
    if accepted is not None and (not isinstance(accepted, torch.Tensor) or accepted.dtype != torch.bool or tuple(accepted.shape) != lead):
        raise ValueError(f"{what}: accepted must be a bool tensor shaped {lead}")
    ops._req(pairs, "pairs", pairs.dtype)
    dev = pairs.device
    if len(lead) == 2:
        Q, K = lead
        rows = torch.arange(Q, device=dev, dtype=pairs.dtype)[:, None].expand(Q, K)
        pairs = torch.stack((rows, pairs), dim=2)
    pairs = pairs.reshape(-1, 2).to(torch.int64)
    ok = refinement.valid.reshape(-1).to(dev)
    if accepted is not None:
        ok = ok & accepted.reshape(-1).to(dev)
    ok = ok & (pairs >= 0).all(dim=1) & (pairs < (1 << 31) - 1).all(dim=1)
    edge = torch.where(ok[:, None], torch.stack((pairs[:, 1], pairs[:, 0]), dim=1), torch.full_like(pairs, -1)).to(torch.int32)
    meas = refinement.matrix().reshape(-1, 4, 4)[:, :3, :].reshape(-1, 12).contiguous()
    weight = torch.tensor(w, dtype=torch.float64, device=dev).repeat(edge.shape[0], 1)
    return edge, meas, weight


class PoseGraphResult:
    """What PoseGraph.optimize returns, all on the device: poses [V, 3, 4] float64; positions [V, 2] float64 = their x and y, what
    places.training_lists, places.evaluation_truth and TupleBank.from_positions take; cost [outer + 1] float64 = the cost before every
    trial and at the end; chi2 [E] float64 = every edge's final unweighted chi-squared, -1 for a skipped edge; info [8] int32 =
    (status, accepted, refused, CG iterations, edges used, edges skipped, nodes moved, 0); converged = a 0-d bool tensor; selection =
    the consistency.LoopConsistency behind close_loops(consistent=...), None otherwise."""
    __slots__ = ("poses", "cost", "chi2", "info", "selection")

    def __init__(self, poses, cost, chi2, info, selection=None):
        self.poses, self.cost, self.chi2, self.info, self.selection = poses, cost, chi2, info, selection

    @property
    def positions(self):
        return self.poses[:, :2, 3]

    @property
    def converged(self):
        return self.info[0] == ops.PGO_CONVERGED


class PoseGraph:
    """One graph: poses [V, 12], [V, 3, 4] or [V, 4, 4] float64 on the device = the nodes' start; every further argument a tuple (edge
    [E, 2] int32, meas [E, 12] float64, weight [E, 2] float64) as odometry_edges and loop_edges make them; fixed [V] bool or uint8 =
    the gauge nodes (None: node 0)."""

    def __init__(self, poses, *edges, fixed=None):
        what = "PoseGraph"
        self.poses = _node_poses(what, poses)
        V = self.poses.shape[0]
        if not 1 <= V <= ops.PGO_MAX_NODES:
            raise ValueError(f"{what}: {V} nodes (1 .. {ops.PGO_MAX_NODES})")
        if not edges:
            raise ValueError(f"{what}: no edges")
        for n, e in enumerate(edges):
            if not isinstance(e, (tuple, list)) or len(e) != 3 or not all(isinstance(t, torch.Tensor) for t in e):
                raise TypeError(f"{what}: edges[{n}] must be a tuple (edge, meas, weight) of tensors")
            ed, me, we = e
            if ed.dtype != torch.int32 or me.dtype != torch.float64 or we.dtype != torch.float64:
                raise TypeError(f"{what}: edges[{n}] must be (int32, float64, float64), got ({ed.dtype}, {me.dtype}, {we.dtype})")
            if ed.dim() != 2 or ed.shape[1] != 2 or tuple(me.shape) != (ed.shape[0], 12) or tuple(we.shape) != (ed.shape[0], 2):
                raise ValueError(f"{what}: edges[{n}] must be ([E, 2], [E, 12], [E, 2]), got ({tuple(ed.shape)}, {tuple(me.shape)}, {tuple(we.shape)})")
        if sum(e[0].shape[0] for e in edges) > ops.PGO_MAX_EDGES:
            raise ValueError(f"{what}: more than {ops.PGO_MAX_EDGES} edges")
        if fixed is not None and (not isinstance(fixed, torch.Tensor) or fixed.dtype not in (torch.bool, torch.uint8) or tuple(fixed.shape) != (V,)):
            raise ValueError(f"{what}: fixed must be a bool or uint8 tensor [V] = ({V},)")
        self.fixed = fixed
        self.edges = [tuple(e) for e in edges]

    def optimize(self, outer=20, cg_iters=400, cg_tol=1e-6, lambda0=1e-4, huber=0.0):
        """-> PoseGraphResult.  outer 0 .. 64 trials, cg_iters 1 .. 1024 a trial, cg_tol the relative residual at which a trial's
        conjugate gradients stop, lambda0 the first damping, huber the threshold on sqrt(chi2) (0: none).  One launch; nothing is
        read back."""
        ops.pgo_params(outer, cg_iters, cg_tol, lambda0, huber)
        ops._req(self.poses, "poses", torch.float64)
        edge = torch.cat([e[0] for e in self.edges])
        meas = torch.cat([e[1] for e in self.edges])
        weight = torch.cat([e[2] for e in self.edges])
        pose, cost, chi2, info = ops.pgo_solve(self.poses, edge, meas, weight, fixed=self.fixed, outer=outer, cg_iters=cg_iters, cg_tol=cg_tol,
                                               lambda0=lambda0, huber=huber)
        return PoseGraphResult(pose.reshape(-1, 3, 4), cost[0], chi2, info[0])


def close_loops(sub, poses, loops, pairs=None, odometry_weights=ODOMETRY_WEIGHTS, loop_weights=LOOP_WEIGHTS, accepted=None, fixed=None,
                consistent=None, **solver):
    """A drive's windows corrected by its loop closures -> PoseGraphResult.  sub: the drive.DriveSubmaps of submaps_from_drive(...,
    frame="reference"); poses: the drive's input poses, as drive takes them (the nodes start at the poses of sub.plan.ref, the windows'
    reference scans); loops: verify.refine_pairs' Refinement of `pairs` [P, 2] = (window a, window b), or refine_candidates'
    Verification with pairs = its topk_idx; consistent: None hands every loop to the solver; a consistency.ConsistencySearch (True: the
    default one) keeps a large set of pairwise-consistent loops, judged at the nodes' start with odometry_weights, and the result carries
    the LoopConsistency as .selection; **solver goes to PoseGraph.optimize.  Nothing is read back."""
    from . import drive
    what = "close_loops"
    if not isinstance(sub, drive.DriveSubmaps):
        raise TypeError(f"{what}: sub must be the DriveSubmaps of drive.submaps_from_drive, got {type(sub).__name__}")
    if not _is_reference(sub):
        raise ValueError(f"{what}: the submaps are in the frame {getattr(sub, 'frame', None)!r}; a loop's pose is an edge between the windows only "
                         "for submaps_from_drive(frame='reference')")
    if pairs is None:
        raise ValueError(f"{what}: pairs is missing (the [P, 2] pairs of refine_pairs, or the topk_idx of refine_candidates)")
    if len(odometry_weights) != 2 or len(loop_weights) != 2:
        raise ValueError(f"{what}: odometry_weights and loop_weights are (w_rot, w_trans)")
    _weights(what, *odometry_weights)
    _weights(what, *loop_weights)
    search = None
    if consistent is not None and consistent is not False:
        from . import consistency
        search = consistency.ConsistencySearch() if consistent is True else consistent
        if not isinstance(search, consistency.ConsistencySearch):
            raise TypeError(f"{what}: consistent must be None, True or a consistency.ConsistencySearch, got {type(consistent).__name__}")
    plan = sub.plan
    p = drive._poses(poses, plan.ref.device, what)
    nodes = p[plan.ref.to(torch.int64).clamp(min=0)]
    od = odometry_edges(nodes, None, *odometry_weights)
    lp = loop_edges(loops, pairs, accepted, *loop_weights)
    if search is None:
        return PoseGraph(nodes, od, lp, fixed=fixed).optimize(**solver)
    graph = PoseGraph(nodes, od, lp, fixed=fixed)      # the whole graph's arguments are checked before the selection runs
    selection = consistency.consistent_loops(nodes, lp, tuple(odometry_weights), search)
    graph.edges[1] = consistency.filter_loops(lp, selection.accepted)
    res = graph.optimize(**solver)
    res.selection = selection
    return res
