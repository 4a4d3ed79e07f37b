"""LiDAR odometry on the device: the scan poses of a drive from its scans alone.

Every stage from drive.submaps_from_drive onward takes poses [S, 12]; this module makes them for a LiDAR log without an INS file, in the
KISS-ICP style: a sliding local voxel map and a constant-velocity start.  It is the hash map that scans are averaged into
(csrc/lpd_map.hip) and the trimmed point-to-plane ICP of a whole scan against it (csrc/lpd_localize.hip), run in turn scan after scan,
plus the three pieces that keep the chain on the device (csrc/lpd_odom.hip; the definition is in include/lpd_hip.h): the prediction
and the acceptance of a scan, the crop of the map around the sensor, and the surface rows of the touched cells only.

    odo = odometry.estimate_poses(points, lengths)                             # Odometry; start = identity
    odo.poses, odo.valid, odo.inliers                                          # [S, 12] float64 on the device, [S] bool, [S] float64
    sub, positions = drive.submaps_from_drive(points, lengths, odo.poses)      # ... and on into close_loops, build_map, localize_scans

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
    table, origin [3] float64 and cell with it (cells() extracts it)."""
    __slots__ = ("poses", "valid", "steps", "refused", "inliers", "rms", "lost", "capacity", "keys", "acc", "origin", "cell", "left_behind")

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


def _run(rows, offsets, lengths, start, search, cap, dev):
    """the whole drive at one capacity, nothing waited for -> (Odometry fields, the tables' counters)"""
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
    for t in range(S):
        ops.odom_predict(pose, pred, t, motion)
        scan = rows[bounds[t]:bounds[t + 1]] if lengths[t] else rows[:1]      # an empty scan: offsets (0, 0) on any row
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
                  capacity=cap, keys=keys, acc=acc, origin=origin, cell=search.cell)
    return fields, torch.stack(counters), state


def estimate_poses(points, lengths, start=None, search=OdometrySearch(), device=None):
    """The scan poses of a drive from its scans (lpd_odom_*, lpd_map_crop, lpd_map_touch with lpd_map_insert and lpd_map_localize) ->
    Odometry.  points / lengths as VoxelMap.insert takes them, each scan in its own sensor frame; start: the first scan's pose, [12] or
    [3, 4] float64, identity by default -- the map's origin is its translation.  For each scan, in order: its start from the two
    poses before it; the ICP of that scan against the local map; the decision (a lost scan keeps its prediction and is not inserted);
    its insert at the accepted pose; the surface rows it touched.  Every `refresh` scans the map is cropped to `keep` metres around the
    last pose, into the second of two tables.  Nothing waits inside the loop; ONE wait at the end reads the tables' lost-rows counters
    and the number of lost scans -- when rows were lost the capacity is doubled and the whole drive run again, at most
    mapping.MAX_DOUBLINGS times."""
    what = "estimate_poses"
    if not isinstance(search, OdometrySearch):
        raise TypeError(f"{what}: search must be an OdometrySearch, got {type(search).__name__}")
    dev = drive._device(device, what)
    rows, lengths = mapping.scan_input(what, points, lengths, dev, owner="the odometry")
    with torch.no_grad():
        S = len(lengths)
        if rows.shape[0] == 0:
            raise ValueError(f"{what}: the drive has no rows")
        with torch.cuda.device(dev):
            start = _start_pose(start, dev, what)
            offsets = drive._scan_offsets(lengths, dev)
            cap = search.capacity
            if cap is None:
                longest = int(max(lengths))
                n = int(np.sum(lengths)) if search.refresh is None else min(int(np.sum(lengths)), 2 * search.refresh * longest)
                cap = mapping.first_capacity(n)
            for _ in range(mapping.MAX_DOUBLINGS + 1):
                fields, counters, state = _run(rows, offsets, lengths, start, search, cap, dev)
                c = torch.cat((counters.sum(dim=0), (S - state.sum(dtype=torch.int64)).reshape(1))).tolist()      # the wait
                if c[2] == 0:
                    return Odometry(lost=c[5], left_behind=c[4], **fields)
                cap *= 2
                if cap > ops.MAP_MAX_CAPACITY:
                    break
    raise LpdHipError(f"{what}: rows were still lost after {mapping.MAX_DOUBLINGS} doublings of the table")
