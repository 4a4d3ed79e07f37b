"""Geometric verification of retrieved places on the device.

A descriptor ranks candidates; whether a candidate IS the query's place, and the relative pose to it (the loop-closure constraint a
mapper needs), is a question about the two clouds.  This module answers it without copying a cloud back: correlative scan matching
(csrc/lpd_align.hip; the definition is in include/lpd_hip.h) of bird's-eye occupancy bitmaps over every yaw and a window of cell
shifts, then a second, finer pass through the same kernel around the coarse winner.

    al = verify.align_pairs(sub_q, sub_db, pairs)                  # Submaps (scale and centre taken from them) or [T, N, 3] tensors
    al.yaw, al.translation, al.overlap, al.matrix()                # [P], [P, 2] metres, [P], [P, 4, 4]: A's metric frame -> B's
    v = verify.verify_candidates(sub_q, sub_db, topk_idx, min_overlap=0.3)
    v.order, v.accepted, v.overlap                                 # [Q, K]: the ranks re-sorted by score, the accepted candidates

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


class AlignSearch:
    """The search of align_pairs, validated and frozen.  cell: metres per cell of the 128 x 128 grid (the coarse pass); shifts: S, the
    window is [-S, S]^2 cells; yaw_steps: H hypotheses 2 pi h / H; layers, z_lo, z_cell: the height layers [z_lo + l z_cell, z_lo +
    (l + 1) z_cell) in the cloud's centred metric frame; fine: a second pass with cell / 2, the 2 fine_div + 1 entries of the dense
    table 2 pi m / (H fine_div) around the coarse winner, and fine_shifts."""
    __slots__ = ("cell", "shifts", "yaw_steps", "layers", "z_lo", "z_cell", "fine", "fine_div", "fine_shifts")

    def __init__(self, cell=0.5, shifts=8, yaw_steps=120, layers=4, z_lo=0.0, z_cell=2.0, fine=True, fine_div=8, fine_shifts=4):
        def whole(v, name, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"AlignSearch: {name}={v!r} (an integer in {lo} .. {hi})")
            return int(v)

        def real(v, name, positive):
            v = float(v)
            if not math.isfinite(v) or (positive and not v > 0.0):
                raise ValueError(f"AlignSearch: {name}={v!r} (finite{', > 0' if positive else ''})")
            return v
        if not isinstance(fine, (bool, np.bool_)):
            raise ValueError(f"AlignSearch: fine={fine!r} (a bool)")
        set_ = object.__setattr__
        set_(self, "cell", real(cell, "cell", True))
        set_(self, "shifts", whole(shifts, "shifts", 0, ops.ALIGN_MAX_S))
        set_(self, "yaw_steps", whole(yaw_steps, "yaw_steps", 1, ops.ALIGN_MAX_H))
        set_(self, "layers", whole(layers, "layers", 1, ops.ALIGN_MAX_LAYERS))
        set_(self, "z_lo", real(z_lo, "z_lo", False))
        set_(self, "z_cell", real(z_cell, "z_cell", True))
        set_(self, "fine", bool(fine))
        set_(self, "fine_div", whole(fine_div, "fine_div", 1, (ops.ALIGN_MAX_H - 1) // 2))
        set_(self, "fine_shifts", whole(fine_shifts, "fine_shifts", 0, ops.ALIGN_MAX_S))
        if self.fine and self.yaw_steps * self.fine_div > ops.ALIGN_MAX_R:
            raise ValueError(f"AlignSearch: yaw_steps * fine_div = {self.yaw_steps * self.fine_div} entries; at most {ops.ALIGN_MAX_R}")
        if self.fine and 2 * self.fine_div + 1 > self.yaw_steps * self.fine_div:
            raise ValueError(f"AlignSearch: the fine window of {2 * self.fine_div + 1} entries is longer than the dense table")

    def __setattr__(self, name, value):
        raise AttributeError("AlignSearch is frozen")

    def __delattr__(self, name):
        raise AttributeError("AlignSearch is frozen")

    def __repr__(self):
        return "AlignSearch(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    def __eq__(self, other):
        return isinstance(other, AlignSearch) and all(getattr(self, n) == getattr(other, n) for n in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, n) for n in self.__slots__))

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


class Alignment:
    """What align_pairs returns, one entry per pair (leading shape [P], or [Q, K] from verify_candidates): yaw float64 radians in
    [0, 2 pi) from the table index; translation [.., 2] float64 metres, so that p_B ~ R(yaw) p_A + translation in the clouds' centred
    metric frames; score, cells_a (at the winning yaw), cells_b int32; overlap = score / min(cells_a, cells_b), 0 where that is 0;
    yaw_scores [.., H] int32 of the coarse pass; valid bool (False: the pair names a row outside its table); coarse [.., 8] and fine
    [.., 8] (or None) = the kernel's `best` of the two passes; center_a / center_b [.., 3] float64 or None."""
    __slots__ = ("yaw", "translation", "score", "cells_a", "cells_b", "overlap", "yaw_scores", "valid", "coarse", "fine", "center_a", "center_b")

    def __init__(self, **kw):
        for n in self.__slots__:
            setattr(self, n, kw[n])

    def matrix(self):
        """[.., 4, 4] float64 taking A's metric frame into B's: a rotation about z and a translation.  With centres
        p_B = R (p_A - c_A) + t + c_B; the z translation comes from the centres only."""
        c, s = torch.cos(self.yaw), torch.sin(self.yaw)
        M = torch.zeros(tuple(self.yaw.shape) + (4, 4), dtype=torch.float64, device=self.yaw.device)
        M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1] = c, -s, s, c
        M[..., 2, 2] = 1.0
        M[..., 3, 3] = 1.0
        M[..., 0, 3], M[..., 1, 3] = self.translation[..., 0], self.translation[..., 1]
        if self.center_a is not None:
            M[..., :3, 3] -= (M[..., :3, :3] @ self.center_a[..., None])[..., 0]
        if self.center_b is not None:
            M[..., :3, 3] += self.center_b
        return M

    def _shaped(self, Q, K):
        def v(t):
            return None if t is None else t.reshape((Q, K) + tuple(t.shape[1:]))
        return Alignment(**{n: v(getattr(self, n)) for n in self.__slots__})


def _cloud_args(t, scale, center, name):
    """-> (table, scale [T] fp32 or None, center [T, 3] or None) of a tensor or a Submaps"""
    from . import submap
    if isinstance(t, submap.Submaps):
        if scale is not None or center is not None:
            raise ValueError(f"align_pairs: {name} is a Submaps: its scale and centre are taken from it")
        return t.x, t.scale, t.center
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"align_pairs: {name} must be a device tensor or a Submaps, got {type(t).__name__}")
    if center is not None:
        if not isinstance(center, torch.Tensor) or center.dim() != 2 or center.shape[1] != 3 or center.shape[0] != t.shape[0]:
            raise ValueError(f"align_pairs: center_{name} must be a [T, 3] tensor")
    return t, scale, center


def align_pairs(a, b, pairs, search=AlignSearch(), scale_a=None, scale_b=None, center_a=None, center_b=None):
    """Align P (row of a, row of b) pairs: one coarse launch over every yaw, and with search.fine a second launch of the same kernel
    around the winner.  a, b: [T, N, 3] or [T, 1, N, 3] fp32 device tensors (scale_* [T] fp32 metres per unit, center_* [T, 3]
    optional), or submap.Submaps.  pairs [P, 2] integer tensor on the device.  -> Alignment.  Everything between the two launches is
    torch on the device; nothing is read back."""
    if not isinstance(search, AlignSearch):
        raise TypeError(f"align_pairs: search must be an AlignSearch, got {type(search).__name__}")
    a, scale_a, center_a = _cloud_args(a, scale_a, center_a, "a")
    b, scale_b, center_b = _cloud_args(b, scale_b, center_b, "b")
    if not isinstance(pairs, torch.Tensor) or pairs.dtype not in (torch.int32, torch.int64):
        raise TypeError("align_pairs: pairs must be an int32 or int64 tensor")
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"align_pairs: pairs must be [P, 2], got {tuple(pairs.shape)}")
    ops._req(a, "a")
    dev = a.device
    TA, TB = a.shape[0], b.shape[0]
    if pairs.dtype == torch.int64:      # a row number beyond int32 is outside every table: it becomes -1, "not read"
        pairs = torch.where((pairs >= 0) & (pairs < (1 << 31) - 1), pairs, torch.full_like(pairs, -1)).to(torch.int32)
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

    def centre(c, col, T):
        if c is None:
            return None
        rows = pairs[:, col].to(torch.int64).clamp(0, T - 1)
        return torch.where(valid[:, None], c.to(device=dev, dtype=torch.float64)[rows], zero)
    return Alignment(yaw=yaw, translation=translation, score=score, cells_a=cells_a, cells_b=cells_b, overlap=overlap, yaw_scores=yaw_scores,
                     valid=valid, coarse=coarse, fine=fine, center_a=centre(center_a, 0, TA), center_b=centre(center_b, 1, TB))


class Verification:
    """What verify_candidates returns: every field of Alignment shaped [Q, K] (translation [Q, K, 2], matrix() [Q, K, 4, 4]), plus
    order [Q, K] int64 = the ranks 0 .. K-1 of every query re-sorted by descending score (ties keep the retrieval order, skipped
    entries come last) and accepted [Q, K] bool (valid and overlap >= min_overlap), or None when no min_overlap was given."""
    __slots__ = ("alignment", "order", "accepted")

    def __init__(self, alignment, order, accepted):
        self.alignment, self.order, self.accepted = alignment, order, accepted

    def __getattr__(self, name):
        if name in Alignment.__slots__ or name == "matrix":
            return getattr(self.alignment, name)
        raise AttributeError(name)


def verify_candidates(query, database, topk_idx, search=AlignSearch(), min_overlap=None):
    """Align every (query i, database row topk_idx[i, r]) pair -- topk_idx [Q, K] as lpd_recall_pairs / lpd_retrieval_topk leave it on
    the device, entries -1 are skipped (never read) -- and re-rank the candidates by the score of the last pass.  query / database:
    Submaps or [T, N, 3] device tensors.  -> Verification.  Nothing is read back."""
    if not isinstance(topk_idx, torch.Tensor) or topk_idx.dtype not in (torch.int32, torch.int64) or topk_idx.dim() != 2:
        raise TypeError("verify_candidates: topk_idx must be a [Q, K] int32 or int64 tensor")
    if min_overlap is not None:
        min_overlap = float(min_overlap)
        if not 0.0 <= min_overlap <= 1.0:
            raise ValueError(f"verify_candidates: min_overlap={min_overlap} outside 0 .. 1")
    Q, K = topk_idx.shape
    if Q < 1 or K < 1:
        raise ValueError(f"verify_candidates: topk_idx must be [Q >= 1, K >= 1], got {tuple(topk_idx.shape)}")
    rows = torch.arange(Q, device=topk_idx.device, dtype=topk_idx.dtype)[:, None].expand(Q, K)
    pairs = torch.stack((torch.where(topk_idx >= 0, rows, torch.full_like(rows, -1)), topk_idx), dim=2).reshape(Q * K, 2)
    al = align_pairs(query, database, pairs, search)._shaped(Q, K)
    rank_key = torch.where(al.valid, al.score, torch.full_like(al.score, -1))
    order = torch.sort(rank_key, dim=1, descending=True, stable=True).indices
    accepted = None if min_overlap is None else al.valid & (al.overlap >= min_overlap)
    return Verification(al, order, accepted)
