"""Submaps from raw LiDAR scans on the device.

Every model here takes a finished submap: exactly N points, zero mean, inside [-1, 1].  The reference's .bin files come from an
offline preprocessing step that is not part of it.  This module is that step, as one kernel launch for a ragged batch of scans of
any length (csrc/lpd_submap.hip; the definition is in include/lpd_hip.h): a voxel-grid average whose cell size is searched so that
the number of occupied cells lands just under N, filled up to exactly N with raw points, centred and scaled.

    sub = submap.make_submaps(scans)                     # list of [n_i, >=3] arrays / tensors  ->  sub.x [B,1,4096,3]
    sub = submap.make_submaps(points, lengths)           # one concatenated [sum n, >=3] tensor + host lengths (KITTI n x 4 rows as they are)
    points, lengths = submap.filter_scans(points, lengths, mask)      # the caller's own range crop / ground removal, as a mask
    model = submap.ScanInput(model)                      # ragged scans in, submaps made on the way

Deterministic: the result does not depend on thread order, and the cell rows do not depend on the order of the raw points.  No CPU
fallback: the work is done on the GPU (host arrays are uploaded to the current device).
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops

NUM_POINTS = 4096


class Submaps:
    """What make_submaps returns.  x [B,1,N,3] fp32, the model input; per cloud: level = the rung j* of the resolution ladder,
    cells = M rows that are cell averages (rows M .. N-1 are raw points), n_raw = points of the scan, center [B,3] and scale [B]
    with row = x * scale + center (0 and 1 when normalize=False); counts [B,N] int32 = points per cell, 0 on fill rows, or None."""
    __slots__ = ("x", "level", "cells", "n_raw", "center", "scale", "counts")

    def __init__(self, x, info, xform, counts):
        self.x = x
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


def _gather_input(scans_or_points, lengths):
    """-> (points [rows, >=3] tensor on the caller's device, host lengths)"""
    if lengths is None:
        if isinstance(scans_or_points, (torch.Tensor, np.ndarray)):
            scans_or_points = [scans_or_points] if scans_or_points.ndim == 2 else list(scans_or_points)
        scans = [_as_tensor(s, f"scan {i}") for i, s in enumerate(scans_or_points)]
        if not scans:
            raise ValueError("make_submaps: no scans")
        lengths = [int(s.shape[0]) for s in scans]
        ops.check_submap_lengths(lengths)
        if len(scans) == 1:
            return scans[0], lengths
        if len({(s.dtype, s.device) for s in scans}) != 1:
            raise ValueError("make_submaps: the scans of one batch must share dtype and device")
        return torch.cat([s[:, :3] for s in scans], 0), lengths
    points = _as_tensor(scans_or_points, "points")
    lengths = [int(n) for n in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if not lengths:
        raise ValueError("make_submaps: no scans")
    total = ops.check_submap_lengths(lengths, points.shape[0])
    if total != points.shape[0]:
        raise ValueError(f"make_submaps: lengths sum to {total}, points has {points.shape[0]} rows")
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


def make_submaps(scans_or_points, lengths=None, num_points=NUM_POINTS, normalize=True, check_finite=True, want_counts=False, device=None):
    """Raw scans -> Submaps (x [B,1,num_points,3] on the GPU).  scans_or_points: a list of [n_i, >=3] tensors / arrays (columns
    behind the third are ignored), or ONE concatenated [sum n, >=3] tensor / array with host `lengths`.  Every scan has 1 .. 2^20
    points; 128 <= num_points <= 4096.  check_finite: reject NaN / inf coordinates (the definition is for finite input; on device
    tensors the check waits for the device once)."""
    N = int(num_points)
    if not ops.SUBMAP_MIN_N <= N <= ops.SUBMAP_MAX_N:
        raise ValueError(f"make_submaps: num_points={N} outside {ops.SUBMAP_MIN_N} .. {ops.SUBMAP_MAX_N}")
    points, lengths = _gather_input(scans_or_points, lengths)
    if check_finite and not bool(torch.isfinite(points[:, :3]).all()):
        raise ValueError("make_submaps: a scan holds NaN or inf coordinates")
    with torch.no_grad():
        rows = _device_rows(points, device)
        off = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        if off[-1] >= 1 << 31:
            raise ValueError(f"make_submaps: {int(off[-1])} rows in one batch exceed 2^31")
        offsets = torch.from_numpy(off.astype(np.int32)).to(rows.device, non_blocking=True)
        B = len(lengths)
        out, info, xform, counts = ops._make_submaps(rows, offsets, B, N, normalize, want_counts, None)
    return Submaps(out.view(B, 1, N, 3), info, xform, counts)


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

    def __init__(self, module, num_points=NUM_POINTS, normalize=True, check_finite=True):
        super().__init__()
        self.module = module
        self.num_points, self.normalize, self.check_finite = int(num_points), bool(normalize), bool(check_finite)

    def forward(self, scans, lengths=None):
        return self.module(make_submaps(scans, lengths, self.num_points, self.normalize, self.check_finite).x)
