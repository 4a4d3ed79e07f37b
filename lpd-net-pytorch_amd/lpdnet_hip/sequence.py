"""Sequence-consistent place retrieval on the device: the stage between retrieval and verify.

A descriptor ranks candidates from ONE frame, which is weakest where loop closure matters most (repetitive streets, seasonal change).
submaps_from_drive cuts windows at a constant stride in drive order, so row i + 1 of a descriptor table is the next place along the
road.  This module scores every retrieved candidate over a short sequence of consecutive queries against a line of consecutive
database rows (SeqSLAM; on LPD-Net's descriptors SeqLPD), at a few velocities and shifts of the candidate row
(csrc/lpd_seqmatch.hip; the definition is in include/lpd_hip.h), re-ranks the candidates by the mean distance along the line, and
moves each one to the best nearby row:

    idx, _ = ops.retrieval_topk(q_desc, d_desc, 25)                # or recall_pairs' topk_idx, or self_candidates for one drive
    m = sequence.match_sequences(q_desc, d_desc, idx, q_offsets, d_offsets, max_mean=0.5)
    m.order, m.row, m.valid, m.accepted, m.mean                    # [Q, K]
    v = verify.verify_candidates(sub_q, sub_db, m.topk(5))         # a shorter, better list for the expensive stages

Integers only behind the quantisation of the distances: the same bits in every launch, and equal to the numpy restatement
(tests/seq_ref.py).  The velocities become an integer table of row steps on the host, so that the device never sees a velocity as a
float.  Nothing is read back.  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import ops
from .verify import _Frozen


class SeqSearch(_Frozen):
    """The search of match_sequences, validated and frozen.  velocities: database rows per query row of every line that is tried
    (negative: the database drive runs the other way); half_length: h, a sequence is the 2h + 1 query rows i - h .. i + h; shifts:
    S, the candidate row is moved by -S .. S rows; min_terms: a line must keep at least that many of its 2h + 1 terms inside the runs
    (None: h + 1)."""
    __slots__ = ("velocities", "half_length", "shifts", "min_terms")

    def __init__(self, velocities=(-2.0, -1.0, -0.5, 0.5, 1.0, 2.0), half_length=5, shifts=2, min_terms=None):
        if isinstance(velocities, (str, bytes)) or not isinstance(velocities, (list, tuple, np.ndarray)) or len(velocities) < 1:
            raise ValueError(f"SeqSearch: velocities={velocities!r} (a non-empty sequence of numbers)")
        vs = []
        for v in velocities:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
                raise ValueError(f"SeqSearch: velocity {v!r} (a finite number)")
            vs.append(float(v))
        self._set("velocities", tuple(vs))
        self._set("half_length", self._whole(half_length, "half_length", 1, ops.SEQ_BAND))
        self._set("shifts", self._whole(shifts, "shifts", 0, ops.SEQ_BAND))
        L = 2 * self.half_length + 1
        self._set("min_terms", self.half_length + 1 if min_terms is None else self._whole(min_terms, "min_terms", 1, L))
        if len(vs) * (2 * self.shifts + 1) > ops.SEQ_MAX_HYP:
            raise ValueError(f"SeqSearch: {len(vs)} velocities x {2 * self.shifts + 1} shifts = {len(vs) * (2 * self.shifts + 1)} hypotheses; "
                             f"at most {ops.SEQ_MAX_HYP}")
        reach = max(abs(float(np.rint(v * self.half_length))) for v in vs)
        if reach + self.shifts > ops.SEQ_BAND:
            raise ValueError(f"SeqSearch: max|steps| + shifts = {int(reach)} + {self.shifts} exceeds the band of {ops.SEQ_BAND} rows")

    @property
    def hypotheses(self):
        return len(self.velocities) * (2 * self.shifts + 1)

    def steps_table(self):
        """[V, 2h + 1] int32 numpy, made on the host: steps[v][t + h] = rint(velocity_v * t) in float64, halves rounded to the even
        integer (numpy's rint and Python's round agree); the middle column is 0"""
        t = np.arange(-self.half_length, self.half_length + 1, dtype=np.float64)
        return np.rint(np.asarray(self.velocities, dtype=np.float64)[:, None] * t[None, :]).astype(np.int32)


class SequenceMatch:
    """What match_sequences returns, every field [Q, K] on the device: hypothesis int32 = the winning e, -1 where the candidate is not
    valid; velocity float64 and shift int32 of that hypothesis (0 where not valid); row int32 = the candidate moved by the shift, -1
    where not valid; sum, terms int32 = the quantised distances along the line and how many were counted; valid bool; order int64 =
    the ranks 0 .. K-1 of every query, valid candidates first by ascending mean (ties keep the retrieval order), the others behind
    in retrieval order; mean float64 = sum / terms / 2^14, inf where not valid -- for reading, never for a decision; accepted bool
    (valid and mean <= max_mean, decided in integers) or None when no max_mean was given."""
    __slots__ = ("hypothesis", "velocity", "shift", "row", "sum", "terms", "valid", "order", "accepted", "mean", "best")

    def __init__(self, **kw):
        for n in self.__slots__:
            setattr(self, n, kw[n])

    def topk(self, k=None):
        """[Q, k] int32: the moved rows of the first k candidates in `order`, -1 for those that are not valid -- what
        verify.verify_candidates and refine_candidates take.  k None: all K."""
        K = self.row.shape[1]
        if k is None:
            k = K
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K:
            raise ValueError(f"SequenceMatch.topk: k={k!r} (an integer in 1 .. {K})")
        return torch.gather(self.row, 1, self.order[:, :int(k)])


def _candidates(what, topk_idx):
    if not isinstance(topk_idx, torch.Tensor) or topk_idx.dtype not in (torch.int32, torch.int64) or topk_idx.dim() != 2:
        raise TypeError(f"{what}: topk_idx must be a [Q, K] int32 or int64 tensor")
    if topk_idx.dtype == torch.int64:      # a row number beyond int32 is outside every table: it becomes -1, "skipped"
        topk_idx = torch.where((topk_idx >= 0) & (topk_idx < (1 << 31) - 1), topk_idx, torch.full_like(topk_idx, -1)).to(torch.int32)
    return topk_idx


def match_sequences(q_desc, d_desc, topk_idx, q_offsets=None, d_offsets=None, search=SeqSearch(), max_mean=None):
    """Score the candidates topk_idx [Q, K] (as lpd_retrieval_topk / lpd_recall_pairs leave them on the device; entries < 0 are
    skipped) of the queries q_desc [Q, dim] against d_desc [nd, dim], both fp32 on the device in drive order (they may be one tensor).
    q_offsets / d_offsets: int32 run offsets on the host, rising from 0 to the table's rows (None: one run); a sequence never crosses
    a run boundary.  max_mean: accept a candidate whose mean squared distance along its best line is at most this.
    -> SequenceMatch.  Nothing is read back."""
    what = "match_sequences"
    if not isinstance(search, SeqSearch):
        raise TypeError(f"{what}: search must be a SeqSearch, got {type(search).__name__}")
    topk_idx = _candidates(what, topk_idx)
    if max_mean is not None:
        if isinstance(max_mean, bool) or not isinstance(max_mean, (int, float, np.integer, np.floating)) or not 0.0 <= float(max_mean) <= 16.0:
            raise ValueError(f"{what}: max_mean={max_mean!r} (a number in 0 .. 16)")
        max_mean = float(max_mean)
    best, order, _ = ops.seq_match(q_desc, d_desc, topk_idx, search.steps_table(), search.shifts, search.min_terms, q_off=q_offsets,
                                   d_off=d_offsets)
    dev = best.device
    e, total, terms, row = best[..., 0], best[..., 1], best[..., 2], best[..., 3]
    valid = e >= 0
    W = 2 * search.shifts + 1
    ec = e.clamp(min=0)
    vel = torch.tensor(search.velocities, dtype=torch.float64, device=dev)[torch.div(ec, W, rounding_mode="floor").to(torch.int64)]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    velocity = torch.where(valid, vel, zero)
    shift = torch.where(valid, torch.remainder(ec, W) - search.shifts, torch.zeros_like(e))
    mean = torch.where(valid, total.to(torch.float64) / terms.clamp(min=1).to(torch.float64) / float(1 << ops.SEQ_QBITS),
                       torch.full((), float("inf"), dtype=torch.float64, device=dev))
    accepted = None
    if max_mean is not None:
        bound = int(np.rint(max_mean * float(1 << ops.SEQ_QBITS)))
        accepted = valid & (total.to(torch.int64) <= bound * terms.to(torch.int64))
    return SequenceMatch(hypothesis=e, velocity=velocity, shift=shift, row=row, sum=total, terms=terms, valid=valid,
                         order=order.to(torch.int64), accepted=accepted, mean=mean, best=best)


def self_candidates(desc, offsets=None, k=25, exclude=10):
    """Candidates for loop closure inside ONE table: the k nearest rows of every row of desc [n, dim] that are not its own
    neighbourhood along the drive -- rows of the same run with |i - j| <= exclude are dropped.  ops.retrieval_topk with k + 2 exclude
    + 1 neighbours (at most n), a stable compaction of the rows that stay, the first k of them, padded with -1.  offsets: int32 run
    offsets on the host (None: one run).  -> [n, k] int32 on the device, in plain torch.  Nothing is read back."""
    what = "self_candidates"
    ops._tensor_arg(what, desc, "desc", torch.float32)
    if desc.dim() != 2 or desc.shape[0] < 1:
        raise ValueError(f"{what}: desc must be [n >= 1, dim], got {tuple(desc.shape)}")
    n = desc.shape[0]
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= ops.SEQ_KMAX:
        raise ValueError(f"{what}: k={k!r} (an integer in 1 .. {ops.SEQ_KMAX})")
    if isinstance(exclude, bool) or not isinstance(exclude, (int, np.integer)) or int(exclude) < 0:
        raise ValueError(f"{what}: exclude={exclude!r} (an integer >= 0)")
    k, exclude = int(k), int(exclude)
    off = ops._seq_offsets(offsets, "offsets", n)
    ops._req(desc, "desc")
    dev = desc.device
    kk = min(k + 2 * exclude + 1, n)
    idx, _ = ops.retrieval_topk(desc, desc, kk)
    rows = torch.arange(n, device=dev, dtype=torch.int64)
    run = torch.bucketize(rows, torch.from_numpy(off[1:].astype(np.int64)).to(dev), right=True)
    j = idx.to(torch.int64)
    drop = (j < 0) | ((run[j.clamp(min=0)] == run[:, None]) & ((j - rows[:, None]).abs() <= exclude))      # (-1: the retrieval ran out of rows)
    pos = torch.sort(drop.to(torch.int8), dim=1, stable=True).indices      # the rows that stay first, in retrieval order
    kept = torch.gather(idx, 1, pos)
    count = (~drop).sum(dim=1, keepdim=True)
    kept = torch.where(torch.arange(kk, device=dev)[None, :] < count, kept, torch.full_like(kept, -1))
    if kk >= k:
        return kept[:, :k].contiguous()
    return torch.cat((kept, torch.full((n, k - kk), -1, dtype=torch.int32, device=dev)), dim=1)
