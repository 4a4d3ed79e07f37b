"""The drive map on the device: corrected poses for every scan, and the scans averaged into one global voxel grid.

posegraph.close_loops corrects the windows' reference scans.  This module carries that correction to every scan of the drive, so that
the corrected drive goes back into drive.submaps_from_drive / accumulate, and builds the map itself: every scan under its pose, averaged
per cell of a global grid that is kept as a hash table (csrc/lpd_map.hip; the definition is in include/lpd_hip.h).  The occupied-cell
count is a quality measure of a loop closure that needs no ground truth: it falls when the laps coincide.

    sub, positions = drive.submaps_from_drive(points, lengths, poses)
    res = posegraph.close_loops(sub, poses, rf, pairs)
    fixed = mapping.correct_scan_poses(sub, poses, res)                        # [S, 12] float64 on the device
    sub2, positions2 = drive.submaps_from_drive(points, lengths, fixed)        # ... re-cut along the corrected drive
    m = mapping.build_map(points, lengths, fixed, cell=0.2)                    # VoxelMap
    m.occupied, m.cells().points, m.cells().counts                             # int, [M, 3] fp32 relative to m.origin, [M] int64
    m.insert(points2, lengths2, poses2)                                        # a second lap or drive into the same map

The sums are integers (units of 2^-16 m), so the map does not depend on the order in which threads, batches or drives arrive; it equals
the numpy restatement (tests/map_ref.py) bit for bit.  No CPU fallback.
"""
import numpy as np
import torch

from . import drive, ops, submap
from ._lib import LpdHipError

# The first capacity: the smallest power of two >= rows / 2 of the first insert -- a cell for every FOUR rows at a load of one half --
# and at least 2^16 slots (2.5 MiB).  tools/map_bench.py counted 5.4 .. 262 rows per occupied cell on the two bench drives with rows in
# scan order at cells of 0.2 m and 1 m, and 1.1 .. 14 with rows scattered uniformly (profiles/map_bench.txt); a slot is 40 bytes, so
# twice the row count would be 2 GB for a 26 M-row drive that 10 .. 320 MiB serve.  A drive with fewer rows a cell grows the table,
# which costs a re-run of the insert per doubling.
MIN_FIRST_CAPACITY = 1 << 16
ROWS_PER_CELL_GUESS = 4
MAX_DOUBLINGS = 8      # of one insert


def _plan_of(what, sub):
    plan = sub.plan if isinstance(sub, drive.DriveSubmaps) else sub
    if not isinstance(plan, drive.DrivePlan):
        raise TypeError(f"{what}: sub must be a drive.DriveSubmaps or its DrivePlan, got {type(sub).__name__}")
    return plan


def correct_scan_poses(sub, poses, result):
    """The correction of a pose graph's nodes carried to every scan -> [S, 12] float64 on the device (lpd_drive_correct).  sub: the
    drive.DriveSubmaps whose windows are the nodes, or its DrivePlan; poses: the drive's input poses as drive takes them; result: the
    posegraph.PoseGraphResult of close_loops, or a [V, 12] / [V, 3, 4] float64 tensor of one pose per window.  A scan that is a node
    gets the node's pose; a scan between two nodes gets the blend of the two rigid continuations of the input odometry, weighted by the
    distance travelled; a scan before the first or behind the last node follows its one node rigidly.  Empty windows (ref = -1) are no
    nodes.  The result goes straight back into drive.submaps_from_drive / accumulate / plan_windows.  Waits for the device once (the
    number of non-empty windows)."""
    from . import posegraph
    what = "correct_scan_poses"
    plan = _plan_of(what, sub)
    nodes = result.poses if isinstance(result, posegraph.PoseGraphResult) else result
    if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.float64:
        raise TypeError(f"{what}: result must be a posegraph.PoseGraphResult or a float64 tensor of node poses")
    if nodes.dim() == 3 and tuple(nodes.shape[1:]) == (3, 4):
        nodes = nodes.reshape(nodes.shape[0], 12)
    if nodes.dim() != 2 or nodes.shape[1] != 12 or nodes.shape[0] != len(plan):
        raise ValueError(f"{what}: one pose per window, [V, 12] or [V, 3, 4] with V = {len(plan)}, got {tuple(nodes.shape)}")
    dev = plan.ref.device
    ops._req(nodes, "result", torch.float64)
    if nodes.device != dev:
        raise ValueError(f"{what}: the node poses are on {nodes.device}, the plan on {dev}")
    p = drive._poses(poses, dev, what)
    if p.device != dev:
        raise ValueError(f"{what}: poses on {p.device}, the plan on {dev}")
    if p.shape[0] != plan.poses.shape[0]:
        raise ValueError(f"{what}: {p.shape[0]} poses, the plan was made for {plan.poses.shape[0]} scans")
    with torch.cuda.device(dev), torch.no_grad():
        keep = plan.ref >= 0
        node_scan, node_pose = plan.ref[keep].contiguous(), nodes[keep].contiguous()      # the wait: how many windows are nodes
        if node_scan.shape[0] == 0:
            raise ValueError(f"{what}: the plan has no window with a reference scan")
        D = plan.distance if p.data_ptr() == plan.poses.data_ptr() else ops.drive_distance(p)[1]
        out, _ = ops.drive_correct(p, D, node_scan, node_pose)
    return out


class MapCells:
    """What VoxelMap.cells returns, on the device, in ascending key order (z-major): points [M, 3] fp32 = the mean of every occupied
    cell's rows relative to origin; counts [M] int64; keys [M] int64; sums [M, 3] int64 = the cells' sums in units of 2^-16 m; origin [3]
    float64; cell (metres, a Python float)."""
    __slots__ = ("points", "counts", "keys", "sums", "origin", "cell")

    def __init__(self, points, counts, keys, sums, origin, cell):
        self.points, self.counts, self.keys, self.sums, self.origin, self.cell = points, counts, keys, sums, origin, cell

    def __len__(self):
        return int(self.keys.shape[0])


def extract_cells(keys, acc, origin, cell):
    """A table -> MapCells, plain torch: the occupied slots, sorted by key, row_c = (float)(((double) S_c / (double) m) * 2^-16).  Every
    step is an exactly rounded elementwise operation."""
    live = keys >= 0
    k, order = torch.sort(keys[live])
    a = acc[live][order]
    m = a[:, 3]
    pts = ((a[:, :3].to(torch.float64) / m.to(torch.float64)[:, None]) * (1.0 / ops.MAP_UNITS_PER_METRE)).to(torch.float32)
    return MapCells(pts, m, k, a[:, :3].contiguous(), origin, cell)


class VoxelMap:
    """A global voxel grid of `cell` metres (2^-10 .. 16) around `origin` ([3] float64; None: the translation of the first finite pose
    of the first insert), kept as a hash table of `capacity` slots (a power of two; None: sized from the first insert, see
    MIN_FIRST_CAPACITY) on `device`.  A cell holds the integer sums of its rows' coordinates and their number."""

    def __init__(self, cell, origin=None, capacity=None, device=None):
        what = "VoxelMap"
        self.inv_cell = ops.map_inv_cell(cell, what)
        self.cell = float(cell)
        self.device = drive._device(device, what)
        if origin is not None:
            o = origin if isinstance(origin, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(origin, dtype=np.float64))
            if o.dtype != torch.float64 or tuple(o.shape) != (3,):
                raise ValueError(f"{what}: origin must be three float64 numbers, got {o.dtype} {tuple(o.shape)}")
            origin = o.to(self.device).contiguous()
        self.origin = origin
        if capacity is not None:
            if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)):
                raise TypeError(f"{what}: capacity must be an integer, got {type(capacity).__name__}")
            capacity = int(capacity)
            if not ops.MAP_MIN_CAPACITY <= capacity <= ops.MAP_MAX_CAPACITY or capacity & (capacity - 1):
                raise ValueError(f"{what}: capacity={capacity} is not a power of two in 16 .. 2^36")
        self._first_capacity = capacity
        self.keys = self.acc = self.info = None
        self.grown = 0      # doublings so far

    @property
    def capacity(self):
        return 0 if self.keys is None else int(self.keys.shape[0])

    def _grow(self, source):
        """a table of twice the capacity holding the cells of `source` = (keys, acc, info) or nothing; doubles again while the rehash
        itself loses a cell"""
        cap = self.capacity
        for _ in range(MAX_DOUBLINGS):
            cap *= 2
            if cap > ops.MAP_MAX_CAPACITY:
                break
            keys, acc, info = ops.map_table(cap, self.device)
            if source is not None:
                ops.map_rehash(source[0], source[1], keys, acc, info)
                info[1] = source[2][1]
                if int(info[2]):
                    continue
            self.keys, self.acc, self.info = keys, acc, info
            self.grown += 1
            return
        raise LpdHipError(f"VoxelMap: the table cannot grow beyond {self.capacity} slots")

    def insert(self, points, lengths, poses, scans=None):
        """Posed scans into the map (lpd_map_insert).  points / lengths as drive.accumulate takes them (a list of [n_i, >=3] scans, or
        one concatenated tensor with host lengths; a scan may be empty), each scan in its own sensor frame; poses as drive takes them;
        scans: a (start, stop) pair or a range -- those scans only.  Incremental: further calls add to the same map, and the map does
        not depend on how the scans are split into calls.  When the table turns out too small (rows lost), it is reallocated at twice
        the capacity from a copy made before the call, and THE CALL IS RUN AGAIN -- at most 8 doublings a call; a table more than half
        full after a call is doubled for the next one.  Waits for the device once a run (the counters).  -> self"""
        what = "VoxelMap.insert"
        pts, lengths = drive._drive_input(points, lengths)
        with torch.no_grad():
            p = drive._poses(poses, self.device, what)
            lengths = drive._lengths(lengths, p.shape[0], what)
            S = p.shape[0]
            if scans is None:
                a, b = 0, S
            else:
                a, b = (scans.start, scans.stop) if isinstance(scans, range) else (int(v) for v in scans)
                if isinstance(scans, range) and scans.step != 1:
                    raise ValueError(f"{what}: scans must be a contiguous range")
                if not 0 <= a <= b <= S:
                    raise ValueError(f"{what}: scans {a} .. {b} outside 0 .. {S}")
            rows = submap._device_rows(pts, self.device)
            if rows.device != self.device or p.device != self.device:
                raise ValueError(f"{what}: points on {rows.device}, poses on {p.device}, the map on {self.device}")
            n = int(lengths[a:b].sum())
            with torch.cuda.device(self.device):
                if self.origin is None:
                    finite = torch.isfinite(p).all(dim=1)
                    self.origin = p[torch.argmax(finite.to(torch.int32))][[3, 7, 11]].contiguous()      # the first finite pose; no wait
                if n == 0:
                    return self
                offsets = drive._scan_offsets(lengths, self.device)
                if self.keys is None:
                    cap = self._first_capacity
                    if cap is None:
                        cap = MIN_FIRST_CAPACITY
                        while cap < 2 * (n // ROWS_PER_CELL_GUESS) and cap < ops.MAP_MAX_CAPACITY:
                            cap *= 2
                    self.keys, self.acc, self.info = ops.map_table(cap, self.device)
                    before = None
                else:
                    before = (self.keys.clone(), self.acc.clone(), self.info.clone())
                for _ in range(MAX_DOUBLINGS + 1):
                    ops.map_insert(rows, offsets, p, self.origin, self.inv_cell, self.keys, self.acc, self.info, a, b)
                    counters = self.info.tolist()      # the wait
                    if counters[2] == 0:
                        break
                    self._grow(before)
                else:
                    raise LpdHipError(f"{what}: rows were still lost after {MAX_DOUBLINGS} doublings of the table")
                if 2 * counters[3] > self.capacity and 2 * self.capacity <= ops.MAP_MAX_CAPACITY:
                    self._grow((self.keys, self.acc, self.info))
        return self

    def _counter(self, k):
        return 0 if self.info is None else int(self.info[k])

    @property
    def occupied(self):
        """the number of occupied cells (a Python int: one read-back)"""
        return self._counter(3)

    @property
    def inserted(self):
        return self._counter(0)

    @property
    def dropped(self):
        """rows that got no cell: a coordinate that is not finite, or a cell more than 2^20 cells from the origin"""
        return self._counter(1)

    def cells(self):
        """-> MapCells, in ascending key order (plain torch: a mask, a sort, a gather, three elementwise operations)"""
        if self.keys is None:
            raise ValueError("VoxelMap.cells: nothing was inserted")
        with torch.no_grad():
            return extract_cells(self.keys, self.acc, self.origin, self.cell)


def build_map(points, lengths, poses, cell=0.2, origin=None, capacity=None, device=None):
    """A drive -> its VoxelMap in one call: VoxelMap(cell, origin, capacity, device).insert(points, lengths, poses).  origin=None takes
    the translation of the first finite pose."""
    return VoxelMap(cell, origin, capacity, device).insert(points, lengths, poses)
