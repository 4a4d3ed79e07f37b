"""Submaps from raw LiDAR scans on the device.

Every model here takes a finished submap: exactly N points, zero mean, inside [-1, 1].  The reference's .bin files come from an
offline preprocessing step that is not part of it.  This module is that step, as one kernel launch for a ragged batch of scans of
any length (csrc/lpd_submap.hip; the definition is in include/lpd_hip.h): a voxel-grid average whose cell size is searched so that
the number of occupied cells lands just under N, filled up to exactly N with raw points, centred and scaled.

    sub = submap.make_submaps(scans)                     # list of [n_i, >=3] arrays / tensors  ->  sub.x [B,1,4096,3]
    sub = submap.make_submaps(points, lengths)           # one concatenated [sum n, >=3] tensor + host lengths (KITTI n x 4 rows as they are)
    sub = submap.make_submaps(scans, clean=submap.RoadRemoval(r_max=50.0))      # range crop + road removal on the device first
    kept = submap.clean_scans(scans, clean=submap.RoadRemoval())                # that step alone: kept.points, kept.offsets, kept.plane
    points, lengths = submap.filter_scans(points, lengths, mask)      # the escape hatch: any rule of the caller's own, as a mask
    model = submap.ScanInput(model)                      # ragged scans in, submaps made on the way

Deterministic: the result does not depend on thread order, and the cell rows do not depend on the order of the raw points.  No CPU
fallback: the work is done on the GPU (host arrays are uploaded to the current device).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops

NUM_POINTS = 4096


class Submaps:
    """What make_submaps returns.  x [B,1,N,3] fp32, the model input; per cloud: level = the rung j* of the resolution ladder,
    cells = M rows that are cell averages (rows M .. N-1 are raw points), n_raw = points of the scan, center [B,3] and scale [B]
    with row = x * scale + center (0 and 1 when normalize=False); counts [B,N] int32 = points per cell, 0 on fill rows, or None.
    cleaned: the CleanedScans of make_submaps(clean=...), else None; n_raw then counts the rows that survived the cleaning, and a
    scan that it emptied is the zero submap with level -1, cells 0, n_raw 0 (what lpd_make_submaps defines for an empty cloud)."""
    __slots__ = ("x", "level", "cells", "n_raw", "center", "scale", "counts", "cleaned")

    def __init__(self, x, info, xform, counts, cleaned=None):
        self.x = x
        self.cleaned = cleaned
        self.level, self.cells, self.n_raw = info[:, 0], info[:, 1], info[:, 2]
        self.center, self.scale = xform[:, :3], xform[:, 3]
        self.counts = counts

    def restore(self):
        """-> [B,N,3] rows in the scans' own coordinates"""
        return self.x[:, 0] * self.scale[:, None, None] + self.center[:, None, :]


def _as_tensor(a, what):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"make_submaps: {what} must be [n, >=3], got {tuple(t.shape)}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"make_submaps: {what} must hold floating-point coordinates, got {t.dtype}")
    return t


def _lengths(lengths, S, what):
    """-> the rows of every scan as a numpy int64 array (a numpy array passes through: no per-element work for a long drive)"""
    a = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what}: lengths must be a sequence of integers, got {a.dtype} {a.shape}")
    a = a.astype(np.int64, copy=False)
    if S is not None and a.size != S:
        raise ValueError(f"{what}: {a.size} scan lengths for {S} poses")
    if a.size and int(a.min()) < 0:
        raise ValueError(f"{what}: a scan length is negative")
    return a


def _gather_input(scans_or_points, lengths, what="make_submaps", empty_ok=False):
    """-> (points [rows, >=3] tensor on the caller's device, host lengths) for the caller `what`.  Every scan has 1 .. 2^20 rows and the
    lengths come back as a list; empty_ok: the scans of a drive, of which one may have no rows and whose lengths come back as a numpy
    int64 array (_lengths)."""
    if lengths is None:
        if isinstance(scans_or_points, (torch.Tensor, np.ndarray)):
            scans_or_points = [scans_or_points] if scans_or_points.ndim == 2 else list(scans_or_points)
        scans = [_as_tensor(s, f"scan {i}") for i, s in enumerate(scans_or_points)]
        if not scans:
            raise ValueError(f"{what}: no scans")
        lengths = [int(s.shape[0]) for s in scans]
        if not empty_ok:
            ops.check_submap_lengths(lengths, None, what)
        if len({(s.dtype, s.device) for s in scans}) != 1:
            raise ValueError(f"{what}: the scans of one {'drive' if empty_ok else 'batch'} must share dtype and device")
        points = scans[0] if len(scans) == 1 else torch.cat([s[:, :3] for s in scans], 0)
        return points, np.array(lengths, dtype=np.int64) if empty_ok else lengths
    points = _as_tensor(scans_or_points, "points")
    if empty_ok:
        lengths = _lengths(lengths, None, what)
        if not lengths.size or int(lengths.sum()) != points.shape[0]:
            raise ValueError(f"{what}: lengths must be non-negative and sum to the {points.shape[0]} rows of points")
        return points, lengths
    lengths = [int(n) for n in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if not lengths:
        raise ValueError(f"{what}: no scans")
    total = ops.check_submap_lengths(lengths, points.shape[0], what)
    if total != points.shape[0]:
        raise ValueError(f"{what}: lengths sum to {total}, points has {points.shape[0]} rows")
    return points, lengths


def _device_rows(points, device):
    """-> fp32 CUDA rows with unit column stride (fp64 is narrowed on the device; fp32 [rows, 4] stays as it is: ld = 4)"""
    if not points.is_cuda:
        if not torch.cuda.is_available():
            raise ops._lib.LpdHipError("make_submaps: no GPU visible; submaps are made on the MI355X only (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        points = points.to(dev, non_blocking=True)
    if points.dtype == torch.float64:
        points = ops.f64_to_f32(points if points.shape[1] == 3 else points[:, :3])
    elif points.dtype != torch.float32:
        points = points.float()
    if points.stride(1) != 1 or points.stride(0) < 3:
        points = points.contiguous()
    return points


class RoadRemoval:
    """The parameters of the range crop and the road removal (include/lpd_hip.h states what each does), validated.  A row is live when
    it is finite, r_min <= its range in plan view <= r_max (metres, at most 512) and z_lo <= z <= z_hi.  H plane hypotheses (0: crop
    only, at most 1024), each through three live rows inside the seed band [seed_z_lo, seed_z_hi] (a sensor-height prior), at least
    min_det (twice the triangle's plan area, m^2) apart and no steeper than max_slope (the norm of the gradient; 0.27 = 15 degrees);
    the one with the most live rows within tau of it wins, needs min_inliers of them, is refined by one least-squares round over them
    (refine), and every live row no higher than `clearance` above it is removed.  seed: 64 bits, the key of the draws."""
    __slots__ = ("r_min", "r_max", "z_lo", "z_hi", "seed_z_lo", "seed_z_hi", "H", "tau", "min_det", "max_slope", "min_inliers", "refine",
                 "clearance", "seed")

    def __init__(self, r_min=0.0, r_max=512.0, z_lo=-math.inf, z_hi=math.inf, seed_z_lo=-math.inf, seed_z_hi=math.inf, H=256, tau=0.15,
                 min_det=4.0, max_slope=0.27, min_inliers=16, refine=1, clearance=0.3, seed=0):
        self.r_min, self.r_max, self.z_lo, self.z_hi = float(r_min), float(r_max), float(z_lo), float(z_hi)
        self.seed_z_lo, self.seed_z_hi = float(seed_z_lo), float(seed_z_hi)
        self.tau, self.min_det, self.max_slope, self.clearance = float(tau), float(min_det), float(max_slope), float(clearance)
        for name in ("H", "min_inliers", "refine", "seed"):
            v = locals()[name]
            if isinstance(v, bool):
                v = int(v)
            if not isinstance(v, (int, np.integer)):
                raise ValueError(f"RoadRemoval: {name}={v!r} must be an integer")
            setattr(self, name, int(v))
        if not 0.0 <= self.r_min <= self.r_max <= ops.CLEAN_MAX_RANGE:
            raise ValueError(f"RoadRemoval: 0 <= r_min={self.r_min} <= r_max={self.r_max} <= {ops.CLEAN_MAX_RANGE:g} required")
        for name in ("z_lo", "z_hi", "seed_z_lo", "seed_z_hi"):
            if math.isnan(getattr(self, name)):
                raise ValueError(f"RoadRemoval: {name} is NaN")
        if self.z_lo > self.z_hi or self.seed_z_lo > self.seed_z_hi:
            raise ValueError("RoadRemoval: a z band is empty (lo > hi)")
        if not 0 <= self.H <= ops.CLEAN_MAX_H:
            raise ValueError(f"RoadRemoval: H={self.H} outside 0 .. {ops.CLEAN_MAX_H}")
        for name in ("tau", "min_det", "max_slope"):
            v = getattr(self, name)
            if not (0.0 <= v < math.inf):
                raise ValueError(f"RoadRemoval: {name}={v} (finite, >= 0)")
        if not math.isfinite(self.clearance):
            raise ValueError(f"RoadRemoval: clearance={self.clearance} (finite)")
        if not 0 <= self.min_inliers < 1 << 31:
            raise ValueError(f"RoadRemoval: min_inliers={self.min_inliers} (>= 0)")
        if self.refine not in (0, 1):
            raise ValueError(f"RoadRemoval: refine={self.refine} (0 or 1)")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"RoadRemoval: seed={self.seed} outside 0 .. 2^64-1")

    def c_params(self):
        """-> ops.CleanParams, the C struct the entry points read (every float rounded to fp32)"""
        return ops.CleanParams(self.r_min, self.r_max, self.z_lo, self.z_hi, self.seed_z_lo, self.seed_z_hi, self.tau, self.min_det,
                               self.max_slope, self.clearance, self.H, self.min_inliers, self.refine, self.seed & 0xFFFFFFFF,
                               self.seed >> 32, 0)

    def __repr__(self):
        return "RoadRemoval(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"


class CleanedScans:
    """What clean_scans returns, all on the device: points [rows,3] fp32 -- the kept rows of scan 0, then scan 1, ... (rows behind
    offsets[-1] are not written); offsets [B+1] int32; plane [B,4] = (a, b, c, 0) with the road at z = a x + b y + c (zeros: no road
    found, or H = 0); info [B,4] int32 = (live rows, the winning hypothesis or -1, its inliers, inliers of the final plane) -- (-1, -1,
    0, 0) marks a scan that was not read; mask [rows] uint8 (1 = kept) or None.  lengths() is the one method that reads back."""
    __slots__ = ("points", "offsets", "plane", "info", "mask")

    def __init__(self, points, offsets, plane, info, mask):
        self.points, self.offsets, self.plane, self.info, self.mask = points, offsets, plane, info, mask

    def lengths(self):
        """-> the kept rows per scan as a host list (waits for the device)"""
        return torch.diff(self.offsets).cpu().tolist()


def _offsets_of(lengths, device, too_many="make_submaps: {} rows in one batch exceed 2^31"):
    """host lengths -> the scan table's offsets [len + 1] int32 on the device; too_many: the caller's message for 2^31 rows and more"""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    if off[-1] >= 1 << 31:
        raise ValueError(too_many.format(int(off[-1])))
    return torch.from_numpy(off.astype(np.int32)).to(device, non_blocking=True)


def _clean_rows(rows, offsets, lengths, clean, want_mask):
    if not isinstance(clean, RoadRemoval):
        raise TypeError(f"clean must be a submap.RoadRemoval, got {type(clean).__name__}")
    if len(lengths) > 65535:
        raise ValueError(f"clean_scans: {len(lengths)} scans in one batch; at most 65535")
    prm, B, longest = clean.c_params(), len(lengths), max(lengths)
    plane, info = ops.road_planes(rows, offsets, B, longest, prm)
    if clean.H > 0:
        out, out_offsets, mask = ops.clean_scans(rows, offsets, B, longest, prm, plane, info, want_mask)
    else:
        out, out_offsets, mask = ops.clean_scans(rows, offsets, B, longest, prm, None, None, want_mask)
    return CleanedScans(out, out_offsets, plane, info, mask)


def clean_scans(scans_or_points, lengths=None, clean=RoadRemoval(), want_mask=False, device=None):
    """Range crop and road removal of raw scans on the device (lpd_road_planes, lpd_clean_count, lpd_clean_fill; the definition is in
    include/lpd_hip.h) -> CleanedScans.  Input as make_submaps takes it; NaN / inf rows are simply dropped.  want_mask: also return
    the per-row keep mask (to carry intensity or labels along: extra[mask.bool()]).  Nothing is read back."""
    points, lengths = _gather_input(scans_or_points, lengths)
    with torch.no_grad():
        rows = _device_rows(points, device)
        return _clean_rows(rows, _offsets_of(lengths, rows.device), lengths, clean, want_mask)


def make_submaps(scans_or_points, lengths=None, num_points=NUM_POINTS, normalize=True, check_finite=True, want_counts=False, device=None,
                 clean=None):
    """Raw scans -> Submaps (x [B,1,num_points,3] on the GPU).  scans_or_points: a list of [n_i, >=3] tensors / arrays (columns
    behind the third are ignored), or ONE concatenated [sum n, >=3] tensor / array with host `lengths`.  Every scan has 1 .. 2^20
    points; 128 <= num_points <= 4096.  check_finite: reject NaN / inf coordinates (the definition is for finite input; on device
    tensors the check waits for the device once).  clean: a RoadRemoval -- the scans are cropped and their road is removed on the
    device first (clean_scans; the result is `.cleaned`), the submaps are made from the rows that are left through the device-side
    offsets: no wait for the device, and no check_finite pass (rows that are not finite are not live).  A scan that the cleaning
    emptied gives the zero submap with level = -1, cells = 0, n_raw = 0."""
    N = int(num_points)
    if not ops.SUBMAP_MIN_N <= N <= ops.SUBMAP_MAX_N:
        raise ValueError(f"make_submaps: num_points={N} outside {ops.SUBMAP_MIN_N} .. {ops.SUBMAP_MAX_N}")
    if clean is not None and not isinstance(clean, RoadRemoval):
        raise TypeError(f"make_submaps: clean must be a submap.RoadRemoval or None, got {type(clean).__name__}")
    points, lengths = _gather_input(scans_or_points, lengths)
    if clean is None and check_finite and not bool(torch.isfinite(points[:, :3]).all()):
        raise ValueError("make_submaps: a scan holds NaN or inf coordinates")
    with torch.no_grad():
        rows = _device_rows(points, device)
        offsets = _offsets_of(lengths, rows.device)
        B = len(lengths)
        cleaned = None
        if clean is not None:
            cleaned = _clean_rows(rows, offsets, lengths, clean, False)
            rows, offsets = cleaned.points, cleaned.offsets
        out, info, xform, counts = ops._make_submaps(rows, offsets, B, N, normalize, want_counts, None)
    return Submaps(out.view(B, 1, N, 3), info, xform, counts, cleaned)


def filter_scans(points, lengths, mask):
    """Ragged compaction: keep the rows of `points` [sum n, C] where `mask` [sum n] is true -> (points, lengths) of the same kind.
    Range crops and ground removal are the caller's: compute the mask (e.g. points[:, 2] > -1.5), pass it here, hand the result to
    make_submaps.  Plain torch; `lengths` is a host sequence and so is the returned one (a device mask is read back once)."""
    points = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points))
    mask = torch.as_tensor(mask, device=points.device)
    lengths = [int(n) for n in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if mask.dtype != torch.bool or mask.dim() != 1 or mask.numel() != points.shape[0] or sum(lengths) != points.shape[0]:
        raise ValueError("filter_scans: mask must be a bool vector with one entry per row, and lengths must sum to the rows")
    ends = torch.as_tensor(np.cumsum(lengths), device=points.device)
    kept = torch.cat((ends.new_zeros(1), torch.cumsum(mask.to(torch.int64), 0)))      # kept[i] = rows kept among the first i
    at_end = kept[ends]
    new = torch.diff(at_end, prepend=at_end.new_zeros(1)).tolist()
    return points[mask], [int(n) for n in new]


class ScanInput(nn.Module):
    """A model behind a raw-scan interface: forward(scans, lengths=None) = module(make_submaps(scans, lengths, ...).x) on the
    current stream, in eval and in train mode (the submaps carry no gradient).  The wrapped model is `.module`, as with
    features.LocalFeatureInput and nn.DataParallel: harness.save_checkpoint / load_pretrained see the real model."""

    def __init__(self, module, num_points=NUM_POINTS, normalize=True, check_finite=True, clean=None):
        super().__init__()
        self.module = module
        self.num_points, self.normalize, self.check_finite = int(num_points), bool(normalize), bool(check_finite)
        if clean is not None and not isinstance(clean, RoadRemoval):
            raise TypeError(f"ScanInput: clean must be a submap.RoadRemoval or None, got {type(clean).__name__}")
        self.clean = clean      # range crop + road removal on the device in front of the submaps

    def forward(self, scans, lengths=None):
        return self.module(make_submaps(scans, lengths, self.num_points, self.normalize, self.check_finite, clean=self.clean).x)
