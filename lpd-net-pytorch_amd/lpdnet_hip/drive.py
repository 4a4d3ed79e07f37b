"""Submaps from a drive on the device: posed scans cut by distance travelled.

The reference starts from finished .bin submaps and a csv of their (northing, easting); both come from an offline step that is not
part of it: take a drive -- a sequence of scans, each with a sensor pose in a world frame -- cut it by distance travelled into windows
(20 m every 10 m for training, 20 m every 20 m for testing), bring the scans of each window into one frame, and record where each
window is.  This module is that step (csrc/lpd_drive.hip; the definition is in include/lpd_hip.h):

    plan = drive.plan_windows(poses, length=20.0, stride=10.0)             # DrivePlan: first / end / ref / rows / positions / offsets
    rows = drive.accumulate(points, lengths, poses, plan)                  # the windows' rows in their reference scans' frames
    sub, positions = drive.submaps_from_drive(points, lengths, poses, 20.0, 10.0, clean=submap.RoadRemoval(r_max=50.0))
    lists = places.training_lists(positions)                               # ... and on into TupleBank.from_positions

poses are [S, 12] float64 (a KITTI poses.txt line each: the top three rows of the sensor-to-world matrix; ingest.load_poses reads the
file), [S, 3, 4] or [S, 4, 4].  Distances are integers in units of 2^-16 m, so the windows do not depend on the order of any sum.  There
is no CPU path: the work is done on the GPU (host arrays are uploaded once, to the current device).
"""
import numpy as np
import torch

from . import ops, submap
from ._lib import LpdHipError
from .submap import _lengths

FRAMES = {"world": 0, "reference": 1}


def _device(device, what):
    if device is None and not torch.cuda.is_available():
        raise LpdHipError(f"{what}: no GPU visible; a drive is cut into submaps on the MI355X only (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise LpdHipError(f"{what}: device {dev}; a drive is cut into submaps on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _poses(poses, device, what):
    """-> [S, 12] float64 on the device (a device tensor stays where it is; a host array is uploaded)"""
    if not isinstance(poses, torch.Tensor):
        a = np.asarray(poses)
        if a.dtype.kind == "f" and a.dtype != np.float64:
            raise ValueError(f"{what}: poses must be float64 (an fp32 ulp at a UTM northing is half a metre), got {a.dtype}")
        poses = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    t = poses
    if t.dtype != torch.float64:
        raise ValueError(f"{what}: poses must be float64 (an fp32 ulp at a UTM northing is half a metre), got {t.dtype}")
    if t.dim() == 3 and tuple(t.shape[1:]) in ((3, 4), (4, 4)):
        t = t[:, :3, :].reshape(t.shape[0], 12)
    if t.dim() != 2 or t.shape[1] != 12 or t.shape[0] < 1:
        raise ValueError(f"{what}: poses must be [S, 12], [S, 3, 4] or [S, 4, 4] with S >= 1, got {tuple(t.shape)}")
    if t.shape[0] > ops.DRIVE_MAX_SCANS:
        raise ValueError(f"{what}: {t.shape[0]} scans; at most 2^22")
    if t.is_cuda:
        return t.contiguous()
    return t.to(_device(device, what), non_blocking=True).contiguous()


class DrivePlan:
    """The windows of a drive.  On the device: first / end / ref / rows [W] int32 -- window w is the scans first[w] .. end[w]-1, ref[w]
    its reference scan (it indexes the caller's timestamps; -1 for an empty window), rows[w] its rows; position [W, 3] float64 = the
    translation of the reference scan (bit-copies), positions = its first two columns [W, 2]: what places.training_lists,
    places.evaluation_truth and TupleBank.from_positions take; offsets [W+1] int32 = the exclusive scan of rows.  On the host:
    row_counts (numpy int64 [W]), length_units / stride_units (2^-16 m), distance_units (the drive's length), and -- for accumulate --
    the device tensors the plan was made from (poses, scan_offsets) and input_rows, the rows of the scans it was made for."""
    __slots__ = ("first", "end", "ref", "rows", "position", "offsets", "row_counts", "length_units", "stride_units", "distance_units", "poses",
                 "scan_offsets", "distance", "input_rows")

    def __len__(self):
        return int(self.first.shape[0])

    @property
    def positions(self):
        return self.position[:, :2]


def _plan(poses, lengths, length, stride):
    """poses [S, 12] on the device and the host lengths of the scans -> DrivePlan; the two waits for the device are here"""
    L, T = ops.drive_units(length, "length"), ops.drive_units(stride, "stride")
    dev = poses.device
    scan_offsets = _scan_offsets(lengths, dev)
    with torch.cuda.device(dev), torch.no_grad():
        _, D = ops.drive_distance(poses)
        total = int(D[-1].item())      # wait 1: the drive's length sizes W
        W = (total - L) // T + 1 if total >= L else 0
        if W > ops.DRIVE_MAX_WINDOW_NO:
            raise ValueError(f"plan_windows: {W} windows; at most 2^22")
        plans, positions = [], []
        for w0 in range(0, W, ops.DRIVE_MAX_WINDOWS):
            p, x = ops.drive_plan(D, scan_offsets, poses, L, T, w0, min(ops.DRIVE_MAX_WINDOWS, W - w0))
            plans.append(p)
            positions.append(x)
        plan = torch.cat(plans) if W else torch.empty((0, 4), dtype=torch.int32, device=dev)
        off64 = torch.zeros((W + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(plan[:, 3], 0, dtype=torch.int64, out=off64[1:])
        counts = plan[:, 3].cpu().numpy().astype(np.int64)      # wait 2: the windows' rows size the grids and the output
    if int(counts.sum()) >= 1 << 31:
        raise ValueError(f"plan_windows: the windows hold {int(counts.sum())} rows; fewer than 2^31 (a longer stride, or fewer scans per call)")
    P = DrivePlan()
    P.first, P.end, P.ref, P.rows = plan[:, 0], plan[:, 1], plan[:, 2], plan[:, 3]
    P.position = torch.cat(positions) if W else torch.empty((0, 3), dtype=torch.float64, device=dev)
    P.offsets = off64.to(torch.int32)
    P.row_counts, P.length_units, P.stride_units, P.distance_units = counts, L, T, total
    P.poses, P.scan_offsets, P.distance, P.input_rows = poses, scan_offsets, D, int(lengths.sum())
    return P


def plan_windows(poses, length=20.0, stride=10.0, device=None, lengths=None):
    """The windows of a drive -> DrivePlan (lpd_drive_steps, a torch.cumsum, lpd_drive_plan).  poses as the module takes them; length
    and stride in metres.  lengths: the rows of every scan (host) -- without it the plan's `rows` count one row per scan.  Waits for
    the device twice: once for the drive's length, which sizes the number of windows, and once for the windows' row counts."""
    p = _poses(poses, device, "plan_windows")
    S = p.shape[0]
    lengths = np.ones(S, dtype=np.int64) if lengths is None else _lengths(lengths, S, "plan_windows")
    return _plan(p, lengths, length, stride)


def _scan_offsets(lengths, device):
    return submap._offsets_of(lengths, device, "a drive of {} rows in one call exceeds 2^31")


class DriveRows:
    """What accumulate returns, on the device: points [rows, 3] fp32 -- the rows of the first window asked for, then the next, ...;
    offsets [W+1] int32.  row_counts is the host's copy of the lengths (numpy int64 [W]); first_window the number of the first."""
    __slots__ = ("points", "offsets", "row_counts", "first_window")

    def __init__(self, points, offsets, row_counts, first_window):
        self.points, self.offsets, self.row_counts, self.first_window = points, offsets, row_counts, first_window

    def lengths(self):
        return [int(n) for n in self.row_counts]


def _window_range(windows, W):
    if windows is None:
        return 0, W
    if isinstance(windows, range):
        if windows.step != 1:
            raise ValueError("accumulate: windows must be a contiguous range")
        a, b = windows.start, windows.stop
    else:
        a, b = (int(v) for v in windows)
    if not 0 <= a <= b <= W:
        raise ValueError(f"accumulate: windows {a} .. {b} outside 0 .. {W}")
    return a, b


def _rows_of(rows, plan, a, b, frame):
    """the launches of accumulate for the windows a .. b-1 (device rows, a plan): no wait for the device"""
    counts = plan.row_counts[a:b]
    total, longest = int(counts.sum()), int(counts.max()) if b > a else 0
    if longest > ops.SUBMAP_MAX_POINTS:
        raise ValueError(f"accumulate: a window holds {longest} rows; at most 2^20 (a shorter window, or fewer rows per scan)")
    dev = rows.device
    off = plan.offsets[a:b + 1] - plan.offsets[a:a + 1] if a else plan.offsets[:b + 1]
    out = torch.empty((max(total, 1), 3), dtype=torch.float32, device=dev)[:total]
    table = torch.stack((plan.first, plan.end, plan.ref, plan.rows), 1)
    for w0 in range(a, b, ops.DRIVE_MAX_WINDOWS):
        w1 = min(b, w0 + ops.DRIVE_MAX_WINDOWS)
        if total and int(plan.row_counts[w0:w1].sum()):
            ops.drive_rows(rows, plan.scan_offsets, plan.poses, table[w0:w1], off[w0 - a:w1 - a + 1], max(longest, 1), total, frame, out)
    return DriveRows(out, off, counts, a)


def accumulate(points, lengths, poses=None, plan=None, length=20.0, stride=10.0, frame="reference", windows=None, device=None):
    """The rows of a drive's windows, each window in one frame -> DriveRows (lpd_drive_rows).  points / lengths as submap.make_submaps
    takes them (a list of [n_i, >=3] scans, or one concatenated tensor with host lengths; a scan may be empty here), each scan in its
    own sensor frame; poses as the module takes them, or plan = a DrivePlan made for these scans (plan_windows(poses, ...,
    lengths=lengths)).  frame: "reference" = the reference scan's own frame, "world" = world axes moved to the reference scan's position.
    windows: a (start, stop) pair or a range -- those windows only.  Without a plan this waits for the device twice (plan_windows);
    with one, not at all: every launch is sized from the plan's host row counts."""
    if frame not in FRAMES:
        raise ValueError(f"accumulate: frame={frame!r} ('reference' or 'world')")
    if plan is None and poses is None:
        raise TypeError("accumulate: poses or a plan")
    pts, lengths = _drive_input(points, lengths)
    with torch.no_grad():
        if plan is None:
            p = _poses(poses, device, "accumulate")
            plan = _plan(p, _lengths(lengths, p.shape[0], "accumulate"), length, stride)
        elif not isinstance(plan, DrivePlan):
            raise TypeError(f"accumulate: plan must be a drive.DrivePlan, got {type(plan).__name__}")
        if len(lengths) != plan.poses.shape[0] or pts.shape[0] != plan.input_rows:
            raise ValueError(f"accumulate: {len(lengths)} scans of {pts.shape[0]} rows, the plan was made for {plan.poses.shape[0]} scans of "
                             f"{plan.input_rows} rows (plan_windows(poses, ..., lengths=lengths))")
        rows = submap._device_rows(pts, plan.poses.device)
        if rows.device != plan.poses.device:
            raise ValueError(f"accumulate: points on {rows.device}, the plan on {plan.poses.device}")
        a, b = _window_range(windows, len(plan))
        with torch.cuda.device(rows.device):
            return _rows_of(rows, plan, a, b, FRAMES[frame])


def _drive_input(points, lengths):
    """submap._gather_input for the scans of a drive: one may have no rows"""
    return submap._gather_input(points, lengths, "accumulate", empty_ok=True)


def submaps_from_drive(points, lengths, poses, length=20.0, stride=10.0, num_points=submap.NUM_POINTS, clean=None, frame="reference",
                       window_batch=1024, normalize=True, device=None):
    """A drive -> (Submaps, positions): accumulate, then the existing cleaning (clean = a submap.RoadRemoval, or None) and
    lpd_make_submaps through their device-side offsets.  positions [W, 2] float64 on the device goes straight into
    places.training_lists, places.evaluation_truth and TupleBank.from_positions; the returned Submaps carries the DrivePlan as `.plan`
    (plan.ref indexes the caller's timestamps).  An empty window, or one the cleaning emptied, is the zero submap with level = -1.
    window_batch (1 .. 65535) windows are accumulated, cleaned and averaged at a time, which bounds the memory of the intermediate
    rows; the road removal draws its hypotheses by a window's number WITHIN its batch, so its planes depend on window_batch.
    Waits for the device: two per drive (plan_windows: the drive's length and the windows' row counts), none per window batch.  Host
    poses and points are uploaded once."""
    N, window_batch = int(num_points), int(window_batch)
    if not ops.SUBMAP_MIN_N <= N <= ops.SUBMAP_MAX_N:
        raise ValueError(f"submaps_from_drive: num_points={N} outside {ops.SUBMAP_MIN_N} .. {ops.SUBMAP_MAX_N}")
    if clean is not None and not isinstance(clean, submap.RoadRemoval):
        raise TypeError(f"submaps_from_drive: clean must be a submap.RoadRemoval or None, got {type(clean).__name__}")
    if not 1 <= window_batch <= ops.DRIVE_MAX_WINDOWS:
        raise ValueError(f"submaps_from_drive: window_batch={window_batch} outside 1 .. {ops.DRIVE_MAX_WINDOWS}")
    if frame not in FRAMES:
        raise ValueError(f"submaps_from_drive: frame={frame!r} ('reference' or 'world')")
    pts, lengths = _drive_input(points, lengths)
    with torch.no_grad():
        p = _poses(poses, device, "submaps_from_drive")
        plan = _plan(p, _lengths(lengths, p.shape[0], "submaps_from_drive"), length, stride)
        W, dev = len(plan), p.device
        if W == 0:
            raise ValueError(f"submaps_from_drive: the drive is {plan.distance_units / ops.DRIVE_UNITS_PER_METRE:.3f} m long, shorter than one window")
        rows = submap._device_rows(pts, dev)
        x = torch.empty((W, N, 3), dtype=torch.float32, device=dev)
        infos, xforms, cleaned = [], [], []
        with torch.cuda.device(dev):
            for a in range(0, W, window_batch):
                b = min(W, a + window_batch)
                got = _rows_of(rows, plan, a, b, FRAMES[frame])
                r, off = got.points, got.offsets
                if r.shape[0] == 0:      # every window of the batch is empty: one row that no offset reaches
                    r = torch.zeros((1, 3), dtype=torch.float32, device=dev)
                if clean is not None:
                    c = submap._clean_rows(r, off, [max(int(n), 1) for n in got.row_counts], clean, False)
                    r, off = c.points, c.offsets
                    cleaned.append(c)
                _, info, xform, _ = ops._make_submaps(r, off, b - a, N, normalize, False, x[a:b])
                infos.append(info)
                xforms.append(xform)
    sub = DriveSubmaps(x.view(W, 1, N, 3), torch.cat(infos), torch.cat(xforms), None, cleaned[0] if len(cleaned) == 1 else (cleaned or None))
    sub.plan, sub.frame = plan, frame
    return sub, plan.positions


class DriveSubmaps(submap.Submaps):
    """submap.Submaps of a drive's windows, with `.plan` (the DrivePlan); `.cleaned` is the CleanedScans of the one window batch, a list
    of them when there were several, or None; `.frame` is the frame of the windows' points ("reference" or "world")."""
    __slots__ = ("plan", "frame")
