"""LiDAR odometry on the device: the scan poses of a drive from its scans alone.

Every stage from drive.submaps_from_drive onward takes poses [S, 12]; this module makes them for a LiDAR log without an INS file, in the
KISS-ICP style: a sliding local voxel map and a constant-velocity start.  It is the hash map that scans are averaged into
(csrc/lpd_map.hip) and the trimmed point-to-plane ICP of a whole scan against it (csrc/lpd_localize.hip), run in turn scan after scan,
plus the three pieces that keep the chain on the device (csrc/lpd_odom.hip; the definition is in include/lpd_hip.h): the prediction
and the acceptance of a scan, the crop of the map around the sensor, and the surface rows of the touched cells only.

    odo = odometry.estimate_poses(points, lengths)                             # Odometry; start = identity
    odo.poses, odo.valid, odo.inliers                                          # [S, 12] float64 on the device, [S] bool, [S] float64
    sub, positions = drive.submaps_from_drive(points, lengths, odo.poses)      # ... and on into close_loops, build_map, localize_scans

A spinning LiDAR measures a scan over the whole period of its sweep, and the sensor moves meanwhile.  With the time of every row the
sweep is brought into the frame of one instant first (csrc/lpd_deskew.hip), KISS-ICP's motion compensation:

    times = odometry.scan_fractions(stamps, lengths)                           # or azimuth_fractions(points, lengths) without stamps
    odo = odometry.estimate_poses(points, lengths, times=times)                # every scan deskewed from the predicted motion, then localised
    odo.points, odo.passed                                                     # the deskewed rows [R, 3] on the device; rows passed through
    rows, info = odometry.deskew_scans(points, lengths, times, poses=ins)      # the INS path: the motion from the poses of the drive

Every sum is an integer and the lookup of a cell does not depend on the slot it landed in, so the poses are the same bits in every
launch and at every table size, and equal tests/odom_ref.py bit for bit.  No CPU fallback.
"""
import math

import numpy as np
import torch

from . import drive, mapping, ops
from ._lib import LpdHipError
from .verify import _Frozen

SURFACES = ("touched", "full")


class OdometrySearch(_Frozen):
    """The search of estimate_poses, validated and frozen.  cell: the local map's cell in metres (2^-10 .. 16); keep: the half width
    in metres of the cube of cells a crop keeps around the sensor, keep_cells = ceil(keep / cell); refresh: the scans between two crops
    (None: never) -- a schedule the host knows, because whether the sensor moved far enough is not known there without a read-back;
    capacity: the slots of each of the two tables, a power of two (None: sized from the largest scan and refresh); localize: the
    mapping.LocalizeSearch of every scan; min_share: a scan whose last pass keeps a smaller share of its rows is lost (DESIGN.md 13q has
    the measurement behind the default); max_jump: so is one that ends further than this many metres from its prediction; first_motion:
    the motion from scan 0 to scan 1 as a [12] / [3, 4] float64 pose, None = none (scan 1 starts at scan 0's pose); surface: "touched"
    remakes the surface rows of the cells an insert touched, "full" those of the whole table after every scan -- the same bits."""
    __slots__ = ("cell", "keep", "refresh", "capacity", "localize", "min_share", "max_jump", "first_motion", "surface")

    def __init__(self, cell=1.0, keep=60.0, refresh=10, capacity=None, localize=mapping.LocalizeSearch(), min_share=0.19, max_jump=5.0,
                 first_motion=None, surface="touched"):
        what = "OdometrySearch"
        try:
            ops.map_inv_cell(cell, what)
        except TypeError as e:
            raise ValueError(str(e)) from None
        self._set("cell", float(cell))
        if isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)) or not math.isfinite(float(keep)) or float(keep) < 0.0:
            raise ValueError(f"{what}: keep={keep!r} (metres, finite, >= 0)")
        if math.ceil(float(keep) / self.cell) > ops.ODOM_MAX_KEEP_CELLS:
            raise ValueError(f"{what}: keep={keep!r} m is more than 2^21 cells of {self.cell} m")
        self._set("keep", float(keep))
        self._set("refresh", None if refresh is None else self._whole(refresh, "refresh", 1, ops.DRIVE_MAX_SCANS))
        if capacity is not None:
            capacity = self._whole(capacity, "capacity", ops.MAP_MIN_CAPACITY, ops.MAP_MAX_CAPACITY)
            if capacity & (capacity - 1):
                raise ValueError(f"{what}: capacity={capacity} is not a power of two")
        self._set("capacity", capacity)
        if not isinstance(localize, mapping.LocalizeSearch):
            raise ValueError(f"{what}: localize must be a mapping.LocalizeSearch, got {type(localize).__name__}")
        self._set("localize", localize)
        ops.odom_share_q(min_share, what)
        self._set("min_share", float(min_share))
        if isinstance(max_jump, bool) or not isinstance(max_jump, (int, float, np.integer, np.floating)) or not 0.0 <= float(max_jump) <= ops.ODOM_MAX_JUMP:
            raise ValueError(f"{what}: max_jump={max_jump!r} outside 0 .. {ops.ODOM_MAX_JUMP:g} m")
        self._set("max_jump", float(max_jump))
        if first_motion is not None:
            m = np.asarray(first_motion.cpu() if isinstance(first_motion, torch.Tensor) else first_motion)
            if m.dtype != np.float64 or m.shape not in ((12,), (3, 4)) or not np.isfinite(m).all():
                raise ValueError(f"{what}: first_motion must be a finite float64 pose, [12] or [3, 4]")
            first_motion = tuple(float(v) for v in m.reshape(12))
        self._set("first_motion", first_motion)
        if surface not in SURFACES:
            raise ValueError(f"{what}: surface={surface!r} (one of {SURFACES})")
        self._set("surface", surface)

    @property
    def keep_cells(self):
        return int(math.ceil(self.keep / self.cell))

    @property
    def share_q(self):
        return ops.odom_share_q(self.min_share)


class Odometry:
    """What estimate_poses returns, on the device, one entry a scan: poses [S, 12] float64 (a lost scan keeps its prediction); valid
    [S] bool (False: lost); steps, refused [S] int32 = the ICP steps applied and refused; inliers [S] float64 = the last pass's
    correspondences over the scan's length (0 for scan 0, which is not localised, and for an empty scan); rms [S] float64 metres of
    the last pass.  lost: the number of lost scans (a Python int, counted at the one wait); capacity: the slots of each table at the
    end; left_behind: the cells that the crops left behind, in all (a Python int, from the same wait); keys, acc: the final local
    table, origin [3] float64 and cell with it (cells() extracts it).  With times: points [R, 3] fp32 on the device = the deskewed rows
    that every scan was localised and inserted with, in the row order of the input; passed: the rows among them that were passed
    through as they came (a Python int, from the same wait).  Without: points is None and passed 0."""
    __slots__ = ("poses", "valid", "steps", "refused", "inliers", "rms", "lost", "capacity", "keys", "acc", "origin", "cell", "left_behind",
                 "points", "passed")

    def __init__(self, **kw):
        for n in self.__slots__:
            setattr(self, n, kw[n])

    def __len__(self):
        return int(self.poses.shape[0])

    def cells(self):
        """the final local map -> mapping.MapCells, in ascending key order"""
        with torch.no_grad():
            return mapping.extract_cells(self.keys, self.acc, self.origin, self.cell)


def _start_pose(start, dev, what):
    if start is None:
        return torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=dev)
    s = start if isinstance(start, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(start))
    if s.dtype != torch.float64 or tuple(s.shape) not in ((12,), (3, 4)):
        raise ValueError(f"{what}: start must be a float64 pose, [12] or [3, 4], got {s.dtype} {tuple(s.shape)}")
    return s.reshape(12).to(dev).contiguous()


def _row_times(what, times, R, dev):
    """times: a [R] float32 tensor or array, or a sequence of them (one a scan) -> contiguous [R] float32 on the device"""
    if isinstance(times, (list, tuple)):
        parts = [t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t)) for t in times]
        times = torch.cat([t.reshape(-1) for t in parts]) if parts else torch.zeros(0)
    elif not isinstance(times, torch.Tensor):
        times = torch.from_numpy(np.ascontiguousarray(times))
    if times.dtype != torch.float32 or times.dim() != 1 or times.shape[0] != R:
        raise ValueError(f"{what}: times must be float32, one value a row = [{R}], got {times.dtype} {tuple(times.shape)}")
    return times.to(dev).contiguous()


def _run(rows, offsets, lengths, start, search, cap, dev, times=None, ref=0.5):
    """the whole drive at one capacity, nothing waited for -> (Odometry fields, the tables' counters, state, the deskew's counters)"""
    S = len(lengths)
    inv_cell = ops.map_inv_cell(search.cell)
    loc = search.localize
    dmax = loc.schedule(search.cell)
    pose = torch.zeros((S, 12), dtype=torch.float64, device=dev)
    pose[0] = start
    pred = torch.zeros_like(pose)
    insert_pose = torch.zeros_like(pose)
    info = torch.zeros((S, 4), dtype=torch.int32, device=dev)
    state = torch.zeros((S,), dtype=torch.int32, device=dev)
    last = torch.zeros((S, 2), dtype=torch.int64, device=dev)      # the last pass's (correspondences, sum of squared residuals)
    origin = start[[3, 7, 11]].contiguous()
    motion = None if search.first_motion is None else torch.tensor(search.first_motion, dtype=torch.float64, device=dev)
    keys, acc, tinfo, info5 = ops.map_crop_table(cap, dev)
    counters = [info5]
    surf = torch.zeros((cap, ops.LOC_SURF), dtype=torch.float32, device=dev)
    dirty = torch.zeros((cap,), dtype=torch.uint8, device=dev)
    # every call sees ONE scan as a table of its own -- its rows, the offsets (0, n) and its pose -- so that a launch's grid is the
    # scan's chunks, not the drive's; the sums are integers, so how the rows fall into chunks does not change a bit of the result
    one = torch.stack((torch.zeros_like(offsets[:-1]), offsets[1:] - offsets[:-1]), dim=1).contiguous()
    bounds = np.concatenate(([0], np.cumsum(lengths)))
    desk = dinfo = None
    if times is not None:      # the deskewed rows, the motion of every scan and the counters: the call's own
        desk = torch.zeros((rows.shape[0], 3), dtype=torch.float32, device=dev)
        motions = torch.zeros_like(pose)
        dinfo = torch.zeros((2,), dtype=torch.int64, device=dev)
    for t in range(S):
        ops.odom_predict(pose, pred, t, motion)
        a, b = (bounds[t], bounds[t + 1]) if lengths[t] else (0, 1)      # an empty scan: offsets (0, 0) on any row
        scan = rows[a:b]
        if times is not None:      # the sweep into the frame of time `ref` under the predicted motion; every later step reads that
            ops.odom_motion(pose, t, motions, motion)
            ops.scan_deskew(scan, one[t], times[a:b], motions[t:t + 1], ref, desk[a:b], dinfo)
            scan = desk[a:b]
        if t > 0:
            p1, i1, s1, _ = ops.map_localize(scan, one[t], pose[t:t + 1], origin, inv_cell, keys, surf, dmax, loc.min_inliers, loc.max_flat)
            pose[t] = p1[0]
            info[t] = i1[0]
            last[t, 0] = s1[-1, 0, 0]
            last[t, 1] = s1[-1, 0, 28]
        ops.odom_accept(pred, pose, info, offsets, t, search.share_q, search.max_jump, insert_pose, state)
        ops.map_insert(scan, one[t], insert_pose[t:t + 1], origin, inv_cell, keys, acc, tinfo)
        if search.refresh is not None and (t + 1) % search.refresh == 0 and t + 1 < S:
            k2, a2, tinfo2, info5 = ops.map_crop_table(cap, dev)
            ops.map_crop(keys, acc, pose[t], origin, inv_cell, search.keep_cells, k2, a2, info5)
            counters.append(info5)
            keys, acc, tinfo = k2, a2, tinfo2
            surf = ops.map_surface(keys, acc, loc.reach, loc.min_cells)[0]
            dirty.zero_()
        elif search.surface == "touched":
            ops.map_touch(scan, one[t], insert_pose[t:t + 1], origin, inv_cell, keys, dirty, loc.reach)
            ops.map_surface_touched(keys, acc, surf, dirty, loc.reach, loc.min_cells)
        else:
            surf = ops.map_surface(keys, acc, loc.reach, loc.min_cells)[0]
    inliers, rms = mapping.fit_quality(info[:, 3], lengths, last[:, 0], last[:, 1])
    fields = dict(poses=pose, valid=state == 1, steps=info[:, 1].contiguous(), refused=info[:, 2].contiguous(), inliers=inliers, rms=rms,
                  capacity=cap, keys=keys, acc=acc, origin=origin, cell=search.cell, points=desk)
    return fields, torch.stack(counters), state, dinfo


def estimate_poses(points, lengths, start=None, search=OdometrySearch(), device=None, times=None, time_ref=0.5):
    """The scan poses of a drive from its scans (lpd_odom_*, lpd_map_crop, lpd_map_touch with lpd_map_insert and lpd_map_localize) ->
    Odometry.  points / lengths as VoxelMap.insert takes them, each scan in its own sensor frame; start: the first scan's pose, [12] or
    [3, 4] float64, identity by default -- the map's origin is its translation.  For each scan, in order: its start from the two
    poses before it; the ICP of that scan against the local map; the decision (a lost scan keeps its prediction and is not inserted);
    its insert at the accepted pose; the surface rows it touched.  Every `refresh` scans the map is cropped to `keep` metres around the
    last pose, into the second of two tables.  Nothing waits inside the loop; ONE wait at the end reads the tables' lost-rows counters
    and the number of lost scans -- when rows were lost the capacity is doubled and the whole drive run again, at most
    mapping.MAX_DOUBLINGS times.

    times: the fraction of its scan's period at which every row was measured, [R] float32 (scan_fractions, azimuth_fractions) or one
    array a scan.  Then every scan is deskewed before it is localised (lpd_odom_motion, lpd_scan_deskew): its rows are brought into
    the frame of the time time_ref of its sweep under the motion the constant-velocity model predicts -- the one between the two poses
    before it, search.first_motion for scans 0 and 1 -- and a pose is the sensor's at that time.  Localisation, decision, insert and
    touch read the deskewed rows, which Odometry.points keeps.  Two more launches a scan, no wait more.  Without times no launch is
    added and every result is what it was."""
    what = "estimate_poses"
    if not isinstance(search, OdometrySearch):
        raise TypeError(f"{what}: search must be an OdometrySearch, got {type(search).__name__}")
    dev = drive._device(device, what)
    rows, lengths = mapping.scan_input(what, points, lengths, dev, owner="the odometry")
    if times is not None:
        time_ref = ops.deskew_ref(time_ref, what)
    with torch.no_grad():
        S = len(lengths)
        if rows.shape[0] == 0:
            raise ValueError(f"{what}: the drive has no rows")
        with torch.cuda.device(dev):
            if times is not None:
                times = _row_times(what, times, rows.shape[0], dev)
            start = _start_pose(start, dev, what)
            offsets = drive._scan_offsets(lengths, dev)
            cap = search.capacity
            if cap is None:
                longest = int(max(lengths))
                n = int(np.sum(lengths)) if search.refresh is None else min(int(np.sum(lengths)), 2 * search.refresh * longest)
                cap = mapping.first_capacity(n)
            for _ in range(mapping.MAX_DOUBLINGS + 1):
                fields, counters, state, dinfo = _run(rows, offsets, lengths, start, search, cap, dev, times, time_ref)
                c = (counters.sum(dim=0), (S - state.sum(dtype=torch.int64)).reshape(1)) + (() if dinfo is None else (dinfo[1:],))
                c = torch.cat(c).tolist()      # the wait
                if c[2] == 0:
                    return Odometry(lost=c[5], left_behind=c[4], passed=0 if dinfo is None else c[6], **fields)
                cap *= 2
                if cap > ops.MAP_MAX_CAPACITY:
                    break
    raise LpdHipError(f"{what}: rows were still lost after {mapping.MAX_DOUBLINGS} doublings of the table")


# ---- motion compensation ------------------------------------------------------------------------------------------------------------------
def deskew_scans(points, lengths, times, poses=None, motions=None, ref=0.5, scans=None, device=None):
    """The sweeps of a drive brought into the frame of ONE instant each (lpd_scan_deskew; definition in include/lpd_hip.h) -> (rows
    [R, 3] fp32 on the device, info [2] int64 on the device = rows transformed, rows passed through).  points / lengths as
    VoxelMap.insert takes them; times [R] float32 = the fraction of its scan's period at which a row was measured (scan_fractions,
    azimuth_fractions), or one array a scan.  EXACTLY ONE of poses and motions: motions [S, 12] float64 = the sensor's pose at the end
    of every scan's period in the frame of its start; poses [S, 12] float64 = the poses of the drive (an INS file, an earlier
    odometry), whose differences are taken as the motions (lpd_drive_motions: the last scan repeats the motion before it).  ref: the
    time of the sweep whose frame the rows get, 0.5 = its middle; a pose of the scan is then the sensor's at that time.  scans: a
    (start, stop) pair or range, only those are deskewed and the rows of the others are copies of the input.  A row with a time
    outside 0 .. 1 or a motion that is not finite is a copy of its input and counted in info[1].  The result goes straight into
    drive.submaps_from_drive, mapping.build_map, VoxelMap.insert and localize_scans.  Nothing is read back."""
    what = "deskew_scans"
    if (poses is None) == (motions is None):
        raise ValueError(f"{what}: exactly one of poses and motions")
    ref = ops.deskew_ref(ref, what)
    dev = drive._device(device, what)
    with torch.no_grad():
        given = drive._poses(poses if motions is None else motions, dev, what)
    S = given.shape[0]
    rows, lengths = mapping.scan_input(what, points, lengths, dev, S, owner="the drive")
    if given.device != dev:
        raise ValueError(f"{what}: points on {rows.device}, {'poses' if motions is None else 'motions'} on {given.device}")
    a, b = mapping._scan_range(what, scans, S)
    with torch.no_grad(), torch.cuda.device(dev):
        R = rows.shape[0]
        if R == 0 or a == b:
            return rows[:, :3].contiguous().clone(), torch.zeros((2,), dtype=torch.int64, device=dev)
        times = _row_times(what, times, R, dev)
        offsets = drive._scan_offsets(lengths, dev)
        motion = ops.drive_motions(given) if motions is None else given
        whole = (a, b) == (0, S)
        out = torch.empty((R, 3), dtype=torch.float32, device=dev) if whole else rows[:, :3].contiguous().clone()
        src = rows if whole else out      # in place on the copy: the rows of the other scans stay the input's
        return ops.scan_deskew(src, offsets, times, motion, ref, out, None, a, b)


def _scan_index(lengths, S, n, dev):
    lengths = torch.as_tensor(np.asarray(lengths, dtype=np.int64)).to(dev)
    return torch.repeat_interleave(torch.arange(S, device=dev), lengths, output_size=n)


def scan_fractions(stamps, lengths):
    """Absolute time stamps, one a row, float64 -> times [R] float32 for deskew_scans / estimate_poses, where stamps lives (a numpy
    array: on the host): (t - min) / (max - min) over the row's scan, the division in float64 and ONE rounding to fp32; 0 for a scan
    whose stamps are all the same (a scan of one row).  Plain torch, no wait."""
    what = "scan_fractions"
    t = stamps if isinstance(stamps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(stamps))
    if t.dtype != torch.float64 or t.dim() != 1:
        raise ValueError(f"{what}: stamps must be float64, one a row, got {t.dtype} {tuple(t.shape)}")
    lengths = drive._lengths(lengths, None, what)
    if int(lengths.sum()) != t.shape[0]:
        raise ValueError(f"{what}: {int(lengths.sum())} rows in lengths, {t.shape[0]} stamps")
    S = len(lengths)
    if t.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.float32, device=t.device)
    with torch.no_grad():
        idx = _scan_index(lengths, S, t.shape[0], t.device)
        lo = torch.full((S,), math.inf, dtype=torch.float64, device=t.device).scatter_reduce(0, idx, t, "amin")
        hi = torch.full((S,), -math.inf, dtype=torch.float64, device=t.device).scatter_reduce(0, idx, t, "amax")
        span = (hi - lo)[idx]
        f = torch.where(span > 0, (t - lo[idx]) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(span))
        return f.to(torch.float32)


def azimuth_fractions(points, lengths, clockwise=True):
    """times [R] float32 for a log WITHOUT stamps (KITTI's Velodyne files), from the azimuth of every row: a sweep that starts and ends
    behind the sensor (azimuth +-180 degrees) and turns clockwise seen from above gives 0.5 (1 - atan2(y, x) / pi), KISS-ICP's rule for
    those files; clockwise=False the other way round.  Plain torch (atan2): an approximation of the firing times and OUTSIDE the
    bit-exact contract -- atan2 is not the same bits on every device.  lengths is checked against the rows only."""
    what = "azimuth_fractions"
    p = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
    if p.dim() != 2 or p.shape[1] < 3 or not p.dtype.is_floating_point:
        raise ValueError(f"{what}: points must be [R, >=3] floating point, got {p.dtype} {tuple(p.shape)}")
    lengths = drive._lengths(lengths, None, what)
    if int(lengths.sum()) != p.shape[0]:
        raise ValueError(f"{what}: {int(lengths.sum())} rows in lengths, {p.shape[0]} points")
    with torch.no_grad():
        az = torch.atan2(p[:, 1].to(torch.float64), p[:, 0].to(torch.float64)) / math.pi
        f = 0.5 * ((1.0 - az) if clockwise else (1.0 + az))
        return f.clamp(0.0, 1.0).to(torch.float32)
