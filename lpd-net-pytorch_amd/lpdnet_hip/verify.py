"""Geometric verification of retrieved places on the device.

A descriptor ranks candidates; whether a candidate IS the query's place, and the relative pose to it (the loop-closure constraint a
mapper needs), is a question about the two clouds.  This module answers it without copying a cloud back: correlative scan matching
(csrc/lpd_align.hip; the definition is in include/lpd_hip.h) of bird's-eye occupancy bitmaps over every yaw and a window of cell
shifts, then a second, finer pass through the same kernel around the coarse winner; and, from that yaw and shift, trimmed
point-to-plane ICP (csrc/lpd_icp.hip) to the full rigid transform with a measure of how well the clouds fit.

    al = verify.align_pairs(sub_q, sub_db, pairs)                  # Submaps (scale and centre taken from them) or [T, N, 3] tensors
    al.yaw, al.translation, al.overlap, al.matrix()                # [P], [P, 2] metres, [P], [P, 4, 4]: A's metric frame -> B's
    v = verify.verify_candidates(sub_q, sub_db, topk_idx, min_overlap=0.3)
    v.order, v.accepted, v.overlap                                 # [Q, K]: the ranks re-sorted by score, the accepted candidates
    rf = verify.refine_pairs(sub_q, sub_db, pairs, init=al)        # 6-DoF: rf.pose [P, 3, 4], rf.inlier_share, rf.rms, rf.matrix()
    v = verify.refine_candidates(sub_q, sub_db, topk_idx, min_overlap=0.3)      # verify_candidates + v.refinement, shaped [Q, K]

Integer-only once the cells are assigned: the same bits in every launch, and equal to the numpy restatement (tests/align_ref.py).  The
(cos, sin) tables are made once on the host in float64 and rounded to fp32; the fine pass takes a window of the dense table by an
integer index, so that no trigonometric function runs on the device and the chain stays bit-exact.  Nothing is read back.  No CPU
fallback.
"""
import math

import numpy as np
import torch

from . import ops

_TABLES = {}


def rot_table(R):
    """[R, 2] fp32 numpy = (cos, sin) of 2 pi m / R, evaluated in float64 and rounded once"""
    ang = 2.0 * np.pi * np.arange(int(R), dtype=np.float64) / float(R)
    return np.stack((np.cos(ang), np.sin(ang)), axis=1).astype(np.float32)


class _Frozen:
    """A validated search: the subclass's __slots__ are its fields, set once by its __init__ (_set), compared and hashed by value"""
    __slots__ = ()

    def _set(self, name, value):
        object.__setattr__(self, name, value)

    def _whole(self, v, name, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{type(self).__name__}: {name}={v!r} (an integer in {lo} .. {hi})")
        return int(v)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is frozen")

    def __delattr__(self, name):
        raise AttributeError(f"{type(self).__name__} is frozen")

    def __repr__(self):
        return type(self).__name__ + "(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    def __eq__(self, other):
        return isinstance(other, type(self)) and all(getattr(self, n) == getattr(other, n) for n in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, n) for n in self.__slots__))


class AlignSearch(_Frozen):
    """The search of align_pairs, validated and frozen.  cell: metres per cell of the 128 x 128 grid (the coarse pass); shifts: S, the
    window is [-S, S]^2 cells; yaw_steps: H hypotheses 2 pi h / H; layers, z_lo, z_cell: the height layers [z_lo + l z_cell, z_lo +
    (l + 1) z_cell) in the cloud's centred metric frame; fine: a second pass with cell / 2, the 2 fine_div + 1 entries of the dense
    table 2 pi m / (H fine_div) around the coarse winner, and fine_shifts."""
    __slots__ = ("cell", "shifts", "yaw_steps", "layers", "z_lo", "z_cell", "fine", "fine_div", "fine_shifts")

    def __init__(self, cell=0.5, shifts=8, yaw_steps=120, layers=4, z_lo=0.0, z_cell=2.0, fine=True, fine_div=8, fine_shifts=4):
        def real(v, name, positive):
            v = float(v)
            if not math.isfinite(v) or (positive and not v > 0.0):
                raise ValueError(f"AlignSearch: {name}={v!r} (finite{', > 0' if positive else ''})")
            return v
        if not isinstance(fine, (bool, np.bool_)):
            raise ValueError(f"AlignSearch: fine={fine!r} (a bool)")
        self._set("cell", real(cell, "cell", True))
        self._set("shifts", self._whole(shifts, "shifts", 0, ops.ALIGN_MAX_S))
        self._set("yaw_steps", self._whole(yaw_steps, "yaw_steps", 1, ops.ALIGN_MAX_H))
        self._set("layers", self._whole(layers, "layers", 1, ops.ALIGN_MAX_LAYERS))
        self._set("z_lo", real(z_lo, "z_lo", False))
        self._set("z_cell", real(z_cell, "z_cell", True))
        self._set("fine", bool(fine))
        self._set("fine_div", self._whole(fine_div, "fine_div", 1, (ops.ALIGN_MAX_H - 1) // 2))
        self._set("fine_shifts", self._whole(fine_shifts, "fine_shifts", 0, ops.ALIGN_MAX_S))
        if self.fine and self.yaw_steps * self.fine_div > ops.ALIGN_MAX_R:
            raise ValueError(f"AlignSearch: yaw_steps * fine_div = {self.yaw_steps * self.fine_div} entries; at most {ops.ALIGN_MAX_R}")
        if self.fine and 2 * self.fine_div + 1 > self.yaw_steps * self.fine_div:
            raise ValueError(f"AlignSearch: the fine window of {2 * self.fine_div + 1} entries is longer than the dense table")

    @property
    def dense_steps(self):
        return self.yaw_steps * self.fine_div

    @staticmethod
    def _table(R, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:      # "cuda" and "cuda:0" are one device: one table
            device = torch.device("cuda", torch.cuda.current_device())
        key = (int(R), device.type, device.index)      # a table is R x 8 bytes and stays for the life of the process
        t = _TABLES.get(key)
        if t is None:
            t = _TABLES[key] = torch.from_numpy(rot_table(R)).to(device)
        return t

    def coarse_table(self, device):
        """[H, 2] fp32 on `device`: made on the host once, cached"""
        return self._table(self.yaw_steps, device)

    def dense_table(self, device):
        """[H * fine_div, 2] fp32 on `device`"""
        return self._table(self.dense_steps, device)


def _yaw_pose(yaw, translation):
    """[.., 3, 4] float64 = (R | t): the rotation by yaw [..] about z and the translation [.., 2] in the plane"""
    c, s = torch.cos(yaw), torch.sin(yaw)
    M = torch.zeros(tuple(yaw.shape) + (3, 4), dtype=torch.float64, device=yaw.device)
    M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1] = c, -s, s, c
    M[..., 2, 2] = 1.0
    M[..., 0, 3], M[..., 1, 3] = translation[..., 0], translation[..., 1]
    return M


class _PerPair:
    """A result with one entry per pair: the subclass's __slots__ are tensors (or None) of leading shape [P]; center_a / center_b are
    two of them"""
    __slots__ = ()

    def __init__(self, **kw):
        for n in self.__slots__:
            setattr(self, n, kw[n])

    def _shaped(self, Q, K):
        def v(t):
            return None if t is None else t.reshape((Q, K) + tuple(t.shape[1:]))
        return type(self)(**{n: v(getattr(self, n)) for n in self.__slots__})

    def _with_centres(self, pose):
        """[.., 4, 4] float64 of pose [.., 3, 4] = (R | t): p_B = R (p_A - c_A) + t + c_B"""
        M = torch.zeros(tuple(pose.shape[:-2]) + (4, 4), dtype=torch.float64, device=pose.device)
        M[..., :3, :] = pose
        M[..., 3, 3] = 1.0
        if self.center_a is not None:
            M[..., :3, 3] -= (M[..., :3, :3] @ self.center_a[..., None])[..., 0]
        if self.center_b is not None:
            M[..., :3, 3] += self.center_b
        return M


class Alignment(_PerPair):
    """What align_pairs returns, one entry per pair (leading shape [P], or [Q, K] from verify_candidates): yaw float64 radians in
    [0, 2 pi) from the table index; translation [.., 2] float64 metres, so that p_B ~ R(yaw) p_A + translation in the clouds' centred
    metric frames; score, cells_a (at the winning yaw), cells_b int32; overlap = score / min(cells_a, cells_b), 0 where that is 0;
    yaw_scores [.., H] int32 of the coarse pass; valid bool (False: the pair names a row outside its table); coarse [.., 8] and fine
    [.., 8] (or None) = the kernel's `best` of the two passes; center_a / center_b [.., 3] float64 or None."""
    __slots__ = ("yaw", "translation", "score", "cells_a", "cells_b", "overlap", "yaw_scores", "valid", "coarse", "fine", "center_a", "center_b")

    def matrix(self):
        """[.., 4, 4] float64 taking A's metric frame into B's: a rotation about z and a translation.  With centres
        p_B = R (p_A - c_A) + t + c_B; the z translation comes from the centres only."""
        return self._with_centres(_yaw_pose(self.yaw, self.translation))


def _cloud_args(what, t, scale, center, name):
    """-> (table, scale [T] fp32 or None, center [T, 3] or None) of a tensor or a Submaps"""
    from . import submap
    if isinstance(t, submap.Submaps):
        if scale is not None or center is not None:
            raise ValueError(f"{what}: {name} is a Submaps: its scale and centre are taken from it")
        return t.x, t.scale, t.center
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a device tensor or a Submaps, got {type(t).__name__}")
    if center is not None:
        if not isinstance(center, torch.Tensor) or center.dim() != 2 or center.shape[1] != 3 or center.shape[0] != t.shape[0]:
            raise ValueError(f"{what}: center_{name} must be a [T, 3] tensor")
    return t, scale, center


def _pair_args(what, a, b, pairs, scale_a, scale_b, center_a, center_b):
    """The clouds and pairs of align_pairs / refine_pairs -> (a, b, pairs [P, 2] int32, scale_a, scale_b, center_a, center_b): a, b
    Submaps or tensors, pairs int32 or int64; no device is looked at"""
    a, scale_a, center_a = _cloud_args(what, a, scale_a, center_a, "a")
    b, scale_b, center_b = _cloud_args(what, b, scale_b, center_b, "b")
    if not isinstance(pairs, torch.Tensor) or pairs.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: pairs must be an int32 or int64 tensor")
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"{what}: pairs must be [P, 2], got {tuple(pairs.shape)}")
    if pairs.dtype == torch.int64:      # a row number beyond int32 is outside every table: it becomes -1, "not read"
        pairs = torch.where((pairs >= 0) & (pairs < (1 << 31) - 1), pairs, torch.full_like(pairs, -1)).to(torch.int32)
    return a, b, pairs, scale_a, scale_b, center_a, center_b


def _centres(c, rows, valid):
    """[P, 3] float64 = the rows `rows` [P] of the centres c [T, 3], 0 where a pair is not valid; None without centres"""
    if c is None:
        return None
    rows = rows.to(torch.int64).clamp(0, c.shape[0] - 1)
    return torch.where(valid[:, None], c.to(device=valid.device, dtype=torch.float64)[rows], torch.zeros((), dtype=torch.float64, device=valid.device))


def align_pairs(a, b, pairs, search=AlignSearch(), scale_a=None, scale_b=None, center_a=None, center_b=None):
    """Align P (row of a, row of b) pairs: one coarse launch over every yaw, and with search.fine a second launch of the same kernel
    around the winner.  a, b: [T, N, 3] or [T, 1, N, 3] fp32 device tensors (scale_* [T] fp32 metres per unit, center_* [T, 3]
    optional), or submap.Submaps.  pairs [P, 2] integer tensor on the device.  -> Alignment.  Everything between the two launches is
    torch on the device; nothing is read back."""
    if not isinstance(search, AlignSearch):
        raise TypeError(f"align_pairs: search must be an AlignSearch, got {type(search).__name__}")
    a, b, pairs, scale_a, scale_b, center_a, center_b = _pair_args("align_pairs", a, b, pairs, scale_a, scale_b, center_a, center_b)
    ops._req(a, "a")
    dev = a.device
    s = search
    H = s.yaw_steps
    coarse, yaw_scores = ops.align_pairs(a, b, pairs, s.coarse_table(dev), H, 1.0 / s.cell, s.shifts, s.z_lo, 1.0 / s.z_cell, s.layers,
                                         scale_a=scale_a, scale_b=scale_b)
    valid = coarse[:, 6] == 1
    last, fine = coarse, None
    if s.fine:
        R = s.dense_steps
        first = torch.remainder(coarse[:, 0].to(torch.int64) * s.fine_div - s.fine_div, R).to(torch.int32)
        cell32 = torch.tensor(s.cell, dtype=torch.float32, device=dev)
        t0 = torch.stack((coarse[:, 2].to(torch.float32) * cell32, coarse[:, 1].to(torch.float32) * cell32), dim=1)
        fine, _ = ops.align_pairs(a, b, pairs, s.dense_table(dev), 2 * s.fine_div + 1, 1.0 / (s.cell / 2.0), s.fine_shifts, s.z_lo,
                                  1.0 / s.z_cell, s.layers, scale_a=scale_a, scale_b=scale_b, first=first, t0=t0, want_yaw_scores=False)
        last = fine
        m = torch.remainder(first.to(torch.int64) + fine[:, 0].to(torch.int64), R)
        yaw = m.to(torch.float64) * (2.0 * math.pi / R)
        translation = t0.to(torch.float64) + torch.stack((fine[:, 2], fine[:, 1]), dim=1).to(torch.float64) * (s.cell / 2.0)
    else:
        yaw = coarse[:, 0].to(torch.float64) * (2.0 * math.pi / H)
        translation = torch.stack((coarse[:, 2], coarse[:, 1]), dim=1).to(torch.float64) * s.cell
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    yaw = torch.where(valid, yaw, zero)
    translation = torch.where(valid[:, None], translation, zero)
    score, cells_a, cells_b = last[:, 3], last[:, 4], last[:, 5]
    least = torch.minimum(cells_a, cells_b)
    overlap = torch.where(least > 0, score.to(torch.float64) / least.clamp(min=1).to(torch.float64), zero)
    return Alignment(yaw=yaw, translation=translation, score=score, cells_a=cells_a, cells_b=cells_b, overlap=overlap, yaw_scores=yaw_scores,
                     valid=valid, coarse=coarse, fine=fine, center_a=_centres(center_a, pairs[:, 0], valid),
                     center_b=_centres(center_b, pairs[:, 1], valid))


class RefineSearch(_Frozen):
    """The search of refine_pairs, validated and frozen.  k: neighbours a normal of b is made from (4 .. 64); dmax: the trimming
    distance in metres, one number or a sequence of `iterations` numbers, one a pass; iterations: steps (0 .. 64); min_inliers: a
    step with fewer correspondences is refused (>= 6); final_dmax: the distance of the pass behind the last step, which makes
    inliers and rms (None: the last entry of dmax)."""
    __slots__ = ("k", "dmax", "iterations", "min_inliers", "final_dmax")

    def __init__(self, k=16, dmax=1.0, iterations=8, min_inliers=32, final_dmax=None):
        def dist(v, name):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"RefineSearch: {name}={v!r} (a number)")
            v = float(v)
            if not (0.0 < v <= ops.ICP_MAX_DMAX and 0.0 < float(np.float32(v)) <= ops.ICP_MAX_DMAX):      # false for NaN
                raise ValueError(f"RefineSearch: {name}={v!r} (finite, > 0, <= {ops.ICP_MAX_DMAX})")
            return v
        self._set("k", self._whole(k, "k", 4, 64))
        self._set("iterations", self._whole(iterations, "iterations", 0, ops.ICP_MAX_ITERS))
        self._set("min_inliers", self._whole(min_inliers, "min_inliers", ops.ICP_MIN_INLIERS, (1 << 31) - 1))
        if isinstance(dmax, (list, tuple, np.ndarray)):
            if len(dmax) != self.iterations:
                raise ValueError(f"RefineSearch: dmax holds {len(dmax)} entries; iterations = {self.iterations}")
            sched = tuple(dist(v, f"dmax[{i}]") for i, v in enumerate(dmax))
        else:
            sched = (dist(dmax, "dmax"),) * self.iterations
        if final_dmax is None:
            if not sched:
                if isinstance(dmax, (list, tuple, np.ndarray)):
                    raise ValueError("RefineSearch: iterations = 0 with an empty dmax needs a final_dmax")
                final_dmax = dmax
            else:
                final_dmax = sched[-1]
        self._set("dmax", sched)
        self._set("final_dmax", dist(final_dmax, "final_dmax"))

    @property
    def schedule(self):
        """the iterations + 1 distances of lpd_icp_pairs"""
        return self.dmax + (self.final_dmax,)


class Refinement(_PerPair):
    """What refine_pairs returns, one entry per pair (leading shape [P], or [Q, K] from refine_candidates): pose [.., 3, 4] float64 =
    (R | t), p_B ~ R p_A + t in the clouds' centred metric frames; valid bool (False: the pair names a row outside its table, or its
    alignment was not valid; its pose is the start); steps, refused int32 = the steps applied and refused; inliers int32 = the
    correspondences of the last pass, inlier_share = inliers / N; rms float64 metres = sqrt(sum ri^2 / m) / 1024 of the last pass, 0
    where m = 0; sums [.., iterations + 1, 32] int64 = every pass's sums; nn [.., N] int32 or None; center_a / center_b [.., 3]
    float64 or None."""
    __slots__ = ("pose", "valid", "steps", "refused", "inliers", "inlier_share", "rms", "sums", "nn", "center_a", "center_b")

    def matrix(self):
        """[.., 4, 4] float64 taking A's metric frame into B's.  With centres p_B = R (p_A - c_A) + t + c_B, as Alignment.matrix()."""
        return self._with_centres(self.pose)


def point_normals(b, k=16):
    """Unit normals [T, N, 3] fp32 of every point of b (a Submaps or a [T, N, 3] / [T, 1, N, 3] fp32 device tensor) from its k nearest
    neighbours (ops.knn_pm, then ops.point_normals); (0, 0, 0) where a neighbourhood has no extent or is not finite."""
    from . import submap
    x = b.x if isinstance(b, submap.Submaps) else b
    x = ops._cloud_table("point_normals", x, "b")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 4 <= int(k) <= 64 or int(k) > x.shape[1]:
        raise ValueError(f"point_normals: k={k!r} (an integer in 4 .. 64, at most N = {x.shape[1]})")
    ops._req(x, "b")
    T, N = x.shape[0], x.shape[1]
    rows = x.contiguous().reshape(T * N, 3)
    idx = ops.knn_pm(rows, T, N, int(k))
    return ops.point_normals(rows, idx, T, N).reshape(T, N, 3)


def _check_init(init, P):
    """type and shape of refine_pairs' `init`, before any device is looked at"""
    if init is None:
        return
    if isinstance(init, Alignment):
        if tuple(init.yaw.shape) != (P,):
            raise ValueError(f"refine_pairs: init is an Alignment of {tuple(init.yaw.shape)} pairs; pairs holds {P}")
        return
    if not isinstance(init, torch.Tensor) or init.dtype != torch.float64:
        raise TypeError("refine_pairs: init must be an Alignment, a float64 tensor or None")
    if tuple(init.shape) not in ((P, 12), (P, 3, 4), (P, 4, 4)):
        raise ValueError(f"refine_pairs: init must be [P, 12], [P, 3, 4] or [P, 4, 4] with P = {P}, got {tuple(init.shape)}")


def _init_pose(init, P, dev):
    """-> (pose [P, 12] float64, ok [P] bool or None) of refine_pairs' `init`"""
    if init is None:
        return torch.eye(3, 4, dtype=torch.float64, device=dev).reshape(1, 12).repeat(P, 1), None
    if isinstance(init, Alignment):
        return _yaw_pose(init.yaw, init.translation).reshape(P, 12), init.valid
    ops._req(init, "init", torch.float64)
    if init.dim() == 3 and init.shape[1] == 4:
        init = init[:, :3, :]
    return init.reshape(P, 12), None


def refine_pairs(a, b, pairs, init=None, search=RefineSearch(), normals_b=None, want_nn=False, scale_a=None, scale_b=None, center_a=None,
                 center_b=None):
    """Refine P (row of a, row of b) pairs to a full rigid transform by trimmed point-to-plane ICP (ops.icp_pairs).  a, b, pairs and the
    scale / centre arguments are those of align_pairs.  init: the start -- an Alignment of the same pairs (the pose is made from its
    yaw and translation on the device; a pair whose alignment is not valid is not read), a [P, 12], [P, 3, 4] or [P, 4, 4] float64
    tensor, or None for the identity.  normals_b [T, N, 3]: the normals of b's clouds when the caller has them (point_normals), made
    here otherwise.  -> Refinement.  Nothing is read back."""
    if not isinstance(search, RefineSearch):
        raise TypeError(f"refine_pairs: search must be a RefineSearch, got {type(search).__name__}")
    a, b, pairs, scale_a, scale_b, center_a, center_b = _pair_args("refine_pairs", a, b, pairs, scale_a, scale_b, center_a, center_b)
    a3, b3 = ops._cloud_table("refine_pairs", a, "a"), ops._cloud_table("refine_pairs", b, "b")
    TB, N, P = b3.shape[0], a3.shape[1], pairs.shape[0]
    _check_init(init, P)
    ops._req(a3, "a")
    dev = a3.device
    pose0, ok = _init_pose(init, P, dev)
    if ok is not None:
        pairs = torch.where(ok[:, None], pairs, torch.full_like(pairs, -1))
    if normals_b is None:
        normals_b = point_normals(b3, min(search.k, N)) if N >= 4 else torch.zeros((TB, N, 3), dtype=torch.float32, device=dev)
    pose, info, sums, nn = ops.icp_pairs(a3, b3, normals_b, pairs, pose0, search.schedule, search.min_inliers, scale_a=scale_a,
                                         scale_b=scale_b, want_nn=want_nn)
    valid = info[:, 0] == 1
    last = sums[-1]
    m = last[:, 0]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    rms = torch.where(m > 0, torch.sqrt(last[:, 28].to(torch.float64) / m.clamp(min=1).to(torch.float64)) / 1024.0, zero)
    return Refinement(pose=pose.reshape(P, 3, 4), valid=valid, steps=info[:, 1], refused=info[:, 2], inliers=info[:, 3],
                      inlier_share=info[:, 3].to(torch.float64) / float(N), rms=rms, sums=sums.permute(1, 0, 2), nn=nn,
                      center_a=_centres(center_a, pairs[:, 0], valid), center_b=_centres(center_b, pairs[:, 1], valid))


class Verification:
    """What verify_candidates and refine_candidates return: every field of Alignment shaped [Q, K] (translation [Q, K, 2], matrix() [Q, K, 4, 4]), plus
    order [Q, K] int64 = the ranks 0 .. K-1 of every query re-sorted by descending score (ties keep the retrieval order, skipped
    entries come last) and accepted [Q, K] bool (valid and overlap >= min_overlap), or None when no min_overlap was given.
    refinement: refine_candidates' Refinement of every pair from its alignment, shaped [Q, K]; None from verify_candidates."""
    __slots__ = ("alignment", "order", "accepted", "refinement")

    def __init__(self, alignment, order, accepted, refinement=None):
        self.alignment, self.order, self.accepted, self.refinement = alignment, order, accepted, refinement

    def __getattr__(self, name):
        if name in Alignment.__slots__ or name == "matrix":
            return getattr(self.alignment, name)
        raise AttributeError(name)


def _verify(what, query, database, topk_idx, search, min_overlap, refine):
    if not isinstance(topk_idx, torch.Tensor) or topk_idx.dtype not in (torch.int32, torch.int64) or topk_idx.dim() != 2:
        raise TypeError(f"{what}: topk_idx must be a [Q, K] int32 or int64 tensor")
    if min_overlap is not None:
        min_overlap = float(min_overlap)
        if not 0.0 <= min_overlap <= 1.0:
            raise ValueError(f"{what}: min_overlap={min_overlap} outside 0 .. 1")
    Q, K = topk_idx.shape
    if Q < 1 or K < 1:
        raise ValueError(f"{what}: topk_idx must be [Q >= 1, K >= 1], got {tuple(topk_idx.shape)}")
    rows = torch.arange(Q, device=topk_idx.device, dtype=topk_idx.dtype)[:, None].expand(Q, K)
    pairs = torch.stack((torch.where(topk_idx >= 0, rows, torch.full_like(rows, -1)), topk_idx), dim=2).reshape(Q * K, 2)
    flat = align_pairs(query, database, pairs, search)
    refinement = None if refine is None else refine_pairs(query, database, pairs, init=flat, search=refine)._shaped(Q, K)
    al = flat._shaped(Q, K)
    rank_key = torch.where(al.valid, al.score, torch.full_like(al.score, -1))
    order = torch.sort(rank_key, dim=1, descending=True, stable=True).indices
    accepted = None if min_overlap is None else al.valid & (al.overlap >= min_overlap)
    return Verification(al, order, accepted, refinement)


def verify_candidates(query, database, topk_idx, search=AlignSearch(), min_overlap=None):
    """Align every (query i, database row topk_idx[i, r]) pair -- topk_idx [Q, K] as lpd_recall_pairs / lpd_retrieval_topk leave it on
    the device, entries -1 are skipped (never read) -- and re-rank the candidates by the score of the last pass.  query / database:
    Submaps or [T, N, 3] device tensors.  -> Verification.  Nothing is read back."""
    return _verify("verify_candidates", query, database, topk_idx, search, min_overlap, None)


def refine_candidates(query, database, topk_idx, search=AlignSearch(), min_overlap=None, refine=RefineSearch()):
    """verify_candidates, and every pair refined from its alignment to a full rigid transform (refine_pairs with `refine`, a
    RefineSearch): the Verification carries .refinement, a Refinement shaped [Q, K]; everything else is what verify_candidates
    returns for the same arguments.  Nothing is read back."""
    if not isinstance(refine, RefineSearch):
        raise TypeError(f"refine_candidates: refine must be a RefineSearch, got {type(refine).__name__}")
    return _verify("refine_candidates", query, database, topk_idx, search, min_overlap, refine)
