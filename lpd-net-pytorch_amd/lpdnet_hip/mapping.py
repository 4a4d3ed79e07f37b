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

The map is what a second lap or session is localised against (csrc/lpd_localize.hip): lap one closed, corrected and mapped as above;
lap two's odometry poses in; localised poses out; lap two inserted into the same map.

    loc = mapping.localize_scans(m, points2, lengths2, odometry2)              # Localization: trimmed point-to-plane ICP against the cells
    loc.poses, loc.inliers, loc.rms                                            # [S2, 12] float64, share of rows with a cell, metres
    m.insert(points2, lengths2, loc.poses)                                     # ... and drive.submaps_from_drive(points2, lengths2, loc.poses)

Every sum of the ICP is an integer as well, and the lookup of a cell does not depend on the slot it landed in: the localised poses are
the same bits in every launch and at every table size, and equal tests/loc_ref.py bit for bit.

Every stage above assumes a static world.  What moved through the scene is found from the rays themselves (csrc/lpd_carve.hip): every
row is a ray from its scan's sensor position, and a cell that later rays pass straight through was not a wall.

    points2, lengths2, res = mapping.remove_moving(points, lengths, poses, cell=0.5)   # the scans without the rows of moving cells
    res.moving, res.rows_removed, res.map, res.source                          # [rows] bool, int, the carved VoxelMap, the full one
    m.pierce(points, lengths, poses); clean = m.carved(); mask = mapping.moving_rows(m, points, lengths, poses)    # ... step by step

A cell holds ONE centroid, so rows of an object that share a cell with the ground cannot be told from it: give the grid an origin
whose z lies a little (0.1 m) above the ground, so that a cell wall separates the ground from what stands on it.  The
walk of a ray is in integers and a count belongs to a cell's key: the same bits at every table size, batching and stream, equal to
tests/carve_ref.py.
"""
import numpy as np
import torch

from . import drive, ops, submap
from ._lib import LpdHipError
from .verify import _Frozen

# The first capacity: the smallest power of two >= rows / 2 of the first insert -- a cell for every FOUR rows at a load of one half --
# and at least 2^16 slots (2.5 MiB).  tools/map_bench.py counted 5.4 .. 262 rows per occupied cell on the two bench drives with rows in
# scan order at cells of 0.2 m and 1 m, and 1.1 .. 14 with rows scattered uniformly (profiles/map_bench.txt); a slot is 40 bytes, so
# twice the row count would be 2 GB for a 26 M-row drive that 10 .. 320 MiB serve.  A drive with fewer rows a cell grows the table,
# which costs a re-run of the insert per doubling.
MIN_FIRST_CAPACITY = 1 << 16
ROWS_PER_CELL_GUESS = 4
MAX_DOUBLINGS = 8      # of one insert


def first_capacity(rows):
    """the slots of a table that is sized from the `rows` it is about to take (see above)"""
    cap = MIN_FIRST_CAPACITY
    while cap < 2 * (rows // ROWS_PER_CELL_GUESS) and cap < ops.MAP_MAX_CAPACITY:
        cap *= 2
    return cap


def _scan_range(what, scans, S):
    """scans: None, a (start, stop) pair or a contiguous range -> (a, b) with 0 <= a <= b <= S"""
    if scans is None:
        return 0, S
    a, b = (scans.start, scans.stop) if isinstance(scans, range) else (int(v) for v in scans)
    if isinstance(scans, range) and scans.step != 1:
        raise ValueError(f"{what}: scans must be a contiguous range")
    if not 0 <= a <= b <= S:
        raise ValueError(f"{what}: scans {a} .. {b} outside 0 .. {S}")
    return a, b


def scan_input(what, points, lengths, device, S=None, owner="the map"):
    """points / lengths as drive.accumulate takes them -> (rows on `device`, host lengths); S: the scans they must hold (None: 1 .. 2^22)"""
    pts, lengths = drive._drive_input(points, lengths)
    if S is None:
        S = len(lengths)
        if not 1 <= S <= ops.DRIVE_MAX_SCANS:
            raise ValueError(f"{what}: {S} scans; 1 .. 2^22")
    with torch.no_grad():
        lengths = drive._lengths(lengths, S, what)
        rows = submap._device_rows(pts, device)
    if rows.device != device:
        raise ValueError(f"{what}: points on {rows.device}, {owner} on {device}")
    return rows, lengths


def _posed_input(what, points, lengths, poses, scans, device):
    """what VoxelMap.insert and localize_scans take -> (rows, lengths, poses [S, 12] float64 on `device`, the scans a .. b-1)"""
    with torch.no_grad():
        p = drive._poses(poses, device, what)
    rows, lengths = scan_input(what, points, lengths, device, p.shape[0])
    if p.device != device:
        raise ValueError(f"{what}: points on {rows.device}, poses on {p.device}, the map on {device}")
    return (rows, lengths, p) + _scan_range(what, scans, p.shape[0])


def fit_quality(matched, lengths, m, ss):
    """a last pass's inliers = matched / the scan's length (0 for an empty scan) and rms = sqrt(ss / m) / 1024 m (0 where m = 0)"""
    m, n_rows = m.to(torch.float64), torch.from_numpy(np.asarray(lengths, dtype=np.float64)).to(m.device)
    inliers = torch.where(n_rows > 0, matched.to(torch.float64) / n_rows.clamp(min=1.0), torch.zeros_like(n_rows))
    rms = torch.where(m > 0, torch.sqrt(ss.to(torch.float64) / m.clamp(min=1.0)) / 1024.0, torch.zeros_like(m))
    return inliers, rms


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
            if not ops.map_capacity_ok(capacity):
                raise ValueError(f"{what}: capacity={capacity} is not a power of two in 16 .. 2^36")
        self._first_capacity = capacity
        self.keys = self.acc = self.info = None
        self._surface = None      # (reach, min_cells, surf, info): slot-indexed, so every insert and every growth drops it
        self.pierced = None       # [capacity] int32 of pierce(): slot-indexed, so a growth drops it
        self._pierce_state = None      # (the Carve counted with, info[0] at that time on the device, rows counted so far)
        self.pierce_info = None   # [6] int64 of pierce()
        self.left_behind = None   # [1] int64 on the device: the cells that carved() left behind, on the map it returned
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
            self._surface = None
            self.pierced = self._pierce_state = self.pierce_info = None
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
        rows, lengths, p, a, b = _posed_input(what, points, lengths, poses, scans, self.device)
        with torch.no_grad():
            n = int(lengths[a:b].sum())
            with torch.cuda.device(self.device):
                if self.origin is None:
                    finite = torch.isfinite(p).all(dim=1)
                    self.origin = p[torch.argmax(finite.to(torch.int32))][[3, 7, 11]].contiguous()      # the first finite pose; no wait
                if n == 0:
                    return self
                self._surface = None
                offsets = drive._scan_offsets(lengths, self.device)
                if self.keys is None:
                    cap = first_capacity(n) if self._first_capacity is None else self._first_capacity
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

    def surface(self, reach=1, min_cells=5):
        """The read side of the table (lpd_map_surface) -> surf [capacity, 8] fp32 on the device, one row a SLOT: (cx, cy, cz, nx, ny,
        nz, flatness, cells used), all zeros for an empty slot.  The normal of a cell comes from the centroids of the present cells among
        the (2 reach + 1)^3 around it (reach 1 or 2), (0, 0, 0) with fewer than min_cells of them.  Made once and kept; every insert and
        every growth of the table drops it, because it is indexed by slot.  Nothing is read back."""
        what = "VoxelMap.surface"
        reach, min_cells = ops.map_surface_params(what, reach, min_cells)
        if self.keys is None:
            raise ValueError(f"{what}: nothing was inserted")
        if self._surface is None or self._surface[:2] != (reach, min_cells):
            with torch.cuda.device(self.device), torch.no_grad():
                self._surface = (reach, min_cells) + ops.map_surface(self.keys, self.acc, reach, min_cells)
        return self._surface[2]

    def surface_cells(self, reach=1, min_cells=5):
        """-> SurfaceCells in ascending key order, the order of cells(): normals [M, 3] fp32, flatness [M] fp32, used [M] int64 (plain
        torch: a mask, a sort, a gather)"""
        surf = self.surface(reach, min_cells)
        with torch.no_grad():
            live = self.keys >= 0
            k, order = torch.sort(self.keys[live])
            s = surf[live][order]
            return SurfaceCells(s[:, 3:6].contiguous(), s[:, 6].contiguous(), s[:, 7].to(torch.int64), k, s[:, :3].contiguous())

    def pierce(self, points, lengths, poses, carve=None, scans=None):
        """Counts, per occupied cell, the rays of posed scans that pass through its content (lpd_map_pierce) and keeps the counts in
        self.pierced ([capacity] int32, one a SLOT) and self.pierce_info ([6] int64).  points / lengths / poses / scans as insert takes
        them -- usually the very scans that were inserted; the surface is made if needed.  Further calls with the same Carve add to the
        same counts (one read-back: the inserted-rows counter must not have moved), and the counts per cell do not depend on how the
        scans are split into calls; another Carve, or an insert since the counts were begun, starts over.  A growth of the table drops
        the counts, because slots move.  PIERCE AFTER THE LAST INSERT: counts taken before a later insert into the
        same table miss that insert's cells and rays; carved() and moving_rows() refuse them (the inserted-rows counter has moved).
        At most 2^31 - 1 rows are counted against one table.  A first call does not wait for the device.  -> self"""
        what = "VoxelMap.pierce"
        carve = Carve() if carve is None else carve
        if not isinstance(carve, Carve):
            raise TypeError(f"{what}: carve must be a Carve, got {type(carve).__name__}")
        if self.keys is None:
            raise ValueError(f"{what}: nothing was inserted")
        rows, lengths, p, a, b = _posed_input(what, points, lengths, poses, scans, self.device)
        with torch.no_grad(), torch.cuda.device(self.device):
            n = int(lengths[a:b].sum())
            fresh = self.pierced is None or self._pierce_state[0] != carve
            if not fresh:      # counts to add to: only while nothing was inserted since they were begun (one read-back)
                then, now = torch.cat((self._pierce_state[1], self.info[0:1])).tolist()
                fresh = then != now
            counted = n if fresh else self._pierce_state[2] + n
            if counted > ops.CARVE_MAX_ROWS:
                raise ValueError(f"{what}: {counted} rows counted against one table; at most 2^31 - 1 (the counts are int32)")
            if fresh:
                self.pierced = torch.zeros((self.capacity,), dtype=torch.int32, device=self.device)
                self.pierce_info = torch.zeros((6,), dtype=torch.int64, device=self.device)
            self._pierce_state = (carve, self.info[0:1].clone(), counted)
            if n == 0 or rows.shape[0] == 0:
                return self
            surf = self.surface(carve.reach, carve.min_cells)
            ops.map_pierce(rows, drive._scan_offsets(lengths, self.device), p, self.origin, self.inv_cell, self.keys, surf,
                           carve.clearance * self.cell, carve.radius * self.cell, carve.skip_end, carve.skip_start, carve.max_steps, carve.max_flat,
                           self.pierced, self.pierce_info, a, b)
        return self

    def _pierce_counts(self, what, carve):
        """the counts of pierce() for the rule of `carve` (None: the Carve they were counted with) -> (pierced, carve); one read-back"""
        if self.pierced is None:
            raise ValueError(f"{what}: no pierce counts; call pierce() after the last insert (a growth of the table drops them)")
        carve = self._pierce_state[0] if carve is None else carve
        if not isinstance(carve, Carve):
            raise TypeError(f"{what}: carve must be a Carve, got {type(carve).__name__}")
        then, now = torch.cat((self._pierce_state[1], self.info[0:1])).tolist()      # the wait
        if then != now:
            raise ValueError(f"{what}: {now - then} rows were inserted after pierce(); count again after the last insert")
        return self.pierced, carve

    def carved(self, carve=None):
        """-> a NEW VoxelMap of the same grid and capacity without the MOVING cells (lpd_map_carve): those with at least
        carve.min_pierce pierces and carve.ratio pierces a row.  carve: None = the Carve that pierce() counted with; another one
        applies its min_pierce and ratio to the same counts.  Its `left_behind` is the [1] int64 count of the cells that stayed
        behind, on the device.  Waits for the device once (see pierce)."""
        what = "VoxelMap.carved"
        pierced, carve = self._pierce_counts(what, carve)
        with torch.no_grad(), torch.cuda.device(self.device):
            out = VoxelMap(self.cell, self.origin, self.capacity, self.device)
            cap = self.capacity
            for _ in range(MAX_DOUBLINGS + 1):
                out.keys, out.acc, out.info, info5 = ops.map_crop_table(cap, self.device)
                ops.map_carve(self.keys, self.acc, pierced, carve.min_pierce, carve.ratio_q, out.keys, out.acc, info5)
                if int(info5[2]) == 0:      # a second wait; a table that held the cells before holds fewer of them now
                    break
                cap *= 2
                if cap > ops.MAP_MAX_CAPACITY:
                    raise LpdHipError(f"{what}: the table cannot grow beyond {self.capacity} slots")
            else:
                raise LpdHipError(f"{what}: cells were still lost after {MAX_DOUBLINGS} doublings of the table")
            out.info[1] = self.info[1]
            out.left_behind = info5[4:5]
        return out


class SurfaceCells:
    """What VoxelMap.surface_cells returns, on the device, in ascending key order: normals [M, 3] fp32 (unit, or (0, 0, 0)), flatness [M]
    fp32 = l3 / l2 of the centroids' covariance, used [M] int64 = the cells the normal was made from, keys [M] int64, points [M, 3] fp32."""
    __slots__ = ("normals", "flatness", "used", "keys", "points")

    def __init__(self, normals, flatness, used, keys, points):
        self.normals, self.flatness, self.used, self.keys, self.points = normals, flatness, used, keys, points

    def __len__(self):
        return int(self.keys.shape[0])


class LocalizeSearch(_Frozen):
    """The search of localize_scans, validated and frozen.  iters: steps (0 .. 64); dmax: the trimming distance in metres -- None:
    min(cell, 16) for the first iters // 2 + 1 passes and half of that afterwards, so that no nearer centroid lies outside the 27 cells
    searched; one number; or a sequence of iters + 1 numbers, one a pass; min_inliers: a step with fewer correspondences is refused
    (>= 6); max_flat: a cell whose centroids' l3 / l2 exceeds it gives no correspondence, in (0, 1]; reach, min_cells: VoxelMap.surface's."""
    __slots__ = ("iters", "dmax", "min_inliers", "max_flat", "reach", "min_cells")

    def __init__(self, iters=8, dmax=None, min_inliers=50, max_flat=0.3, reach=1, min_cells=5):
        what = "LocalizeSearch"
        self._set("iters", self._whole(iters, "iters", 0, ops.LOC_MAX_ITERS))
        self._set("min_inliers", self._whole(min_inliers, "min_inliers", ops.LOC_MIN_INLIERS, (1 << 31) - 1))
        if isinstance(max_flat, bool) or not isinstance(max_flat, (int, float, np.integer, np.floating)) or not 0.0 < float(max_flat) <= 1.0:
            raise ValueError(f"{what}: max_flat={max_flat!r} outside (0, 1]")
        self._set("max_flat", float(max_flat))
        try:
            reach, min_cells = ops.map_surface_params(what, reach, min_cells)
        except TypeError as e:
            raise ValueError(str(e)) from None
        self._set("reach", reach)
        self._set("min_cells", min_cells)
        if dmax is not None:
            if not isinstance(dmax, (list, tuple, np.ndarray)):
                dmax = (dmax,) * (self.iters + 1)
            if len(dmax) != self.iters + 1:
                raise ValueError(f"{what}: dmax holds {len(dmax)} entries; iters + 1 = {self.iters + 1}")
            for i, v in enumerate(dmax):
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                    raise ValueError(f"{what}: dmax[{i}]={v!r} (a number)")
            dmax = tuple(float(v) for v in dmax)
            ops.map_localize_dmax(what, dmax)
        self._set("dmax", dmax)

    def schedule(self, cell):
        """the iters + 1 distances of lpd_map_localize on a map of `cell` metres"""
        if self.dmax is not None:
            return self.dmax
        wide = min(float(cell), ops.LOC_MAX_DMAX)
        n_wide = min(self.iters // 2 + 1, self.iters + 1)
        return (wide,) * n_wide + (0.5 * wide,) * (self.iters + 1 - n_wide)


class Localization:
    """What localize_scans returns, on the device, one entry a scan: poses [S, 12] float64 (scans that were not asked for, and invalid
    ones, keep their input pose bit for bit); valid [S] bool (False: not asked for, a pose that is not finite, more than 2^20 rows);
    steps, refused [S] int32 = the steps applied and refused; inliers [S] float64 = the last pass's correspondences over the scan's
    length (0 for an empty scan); rms [S] float64 metres = sqrt(sum ri^2 / m) / 1024 of the last pass, 0 where m = 0; sums
    [iters + 1, S, 32] int64 = every pass's sums; cells [rows] int64 or None = the last pass's cell key of every row, -1 without a
    correspondence."""
    __slots__ = ("poses", "valid", "steps", "refused", "inliers", "rms", "sums", "cells")

    def __init__(self, poses, valid, steps, refused, inliers, rms, sums, cells):
        self.poses, self.valid, self.steps, self.refused, self.inliers, self.rms, self.sums, self.cells = (poses, valid, steps, refused, inliers,
                                                                                                         rms, sums, cells)

    def __len__(self):
        return int(self.poses.shape[0])


def localize_scans(vmap, points, lengths, poses, search=LocalizeSearch(), scans=None, want_cells=False):
    """Posed scans localised against a VoxelMap: trimmed point-to-plane ICP of every scan, as a whole, against the centroids and normals
    of the map's cells (lpd_map_localize) -> Localization.  points / lengths / poses / scans as VoxelMap.insert takes them, each scan in
    its own sensor frame and `poses` the start -- odometry, or the last fix carried forward; a start within about a cell and a few
    degrees converges.  The result's poses go straight into drive.submaps_from_drive, VoxelMap.insert and
    correct_scan_poses.  Judge a scan by `inliers`: a scan at the right place keeps a third or more of its rows, one that is lost a few
    per cent.  Nothing waits for the device."""
    what = "localize_scans"
    if not isinstance(vmap, VoxelMap):
        raise TypeError(f"{what}: vmap must be a VoxelMap, got {type(vmap).__name__}")
    if not isinstance(search, LocalizeSearch):
        raise TypeError(f"{what}: search must be a LocalizeSearch, got {type(search).__name__}")
    if vmap.keys is None:
        raise ValueError(f"{what}: nothing was inserted into the map")
    rows, lengths, p, a, b = _posed_input(what, points, lengths, poses, scans, vmap.device)
    with torch.no_grad():
        S, dev = p.shape[0], vmap.device
        with torch.cuda.device(dev):
            n = int(lengths[a:b].sum())
            if n == 0 or rows.shape[0] == 0:      # nothing to read: every scan keeps its pose
                zero = torch.zeros((S,), dtype=torch.int32, device=dev)
                return Localization(p.clone(), torch.zeros((S,), dtype=torch.bool, device=dev), zero, zero.clone(),
                                    torch.zeros((S,), dtype=torch.float64, device=dev), torch.zeros((S,), dtype=torch.float64, device=dev),
                                    torch.zeros((search.iters + 1, S, ops.LOC_SUMS), dtype=torch.int64, device=dev),
                                    torch.full((rows.shape[0],), -1, dtype=torch.int64, device=dev) if want_cells else None)
            offsets = drive._scan_offsets(lengths, dev)
            surf = vmap.surface(search.reach, search.min_cells)
            pose, info, sums, cells = ops.map_localize(rows, offsets, p, vmap.origin, vmap.inv_cell, vmap.keys, surf, search.schedule(vmap.cell),
                                                       search.min_inliers, search.max_flat, a, b, want_cells)
            inliers, rms = fit_quality(info[:, 3], lengths, sums[-1, :, 0], sums[-1, :, 28])
    return Localization(pose, info[:, 0] == 1, info[:, 1].contiguous(), info[:, 2].contiguous(), inliers, rms, sums, cells)


def build_map(points, lengths, poses, cell=0.2, origin=None, capacity=None, device=None):
    """A drive -> its VoxelMap in one call: VoxelMap(cell, origin, capacity, device).insert(points, lengths, poses).  origin=None takes
    the translation of the first finite pose."""
    return VoxelMap(cell, origin, capacity, device).insert(points, lengths, poses)


class Carve(_Frozen):
    """How moving objects are found in a VoxelMap, validated and frozen (lpd_map_pierce, lpd_map_carve).  skip_end,
    skip_start: cells of a ray next to its endpoint's / the sensor's cell (Chebyshev) that are stepped into but not looked up, 0 .. 16;
    max_steps: cells of one ray that are stepped into, 1 .. 8192; max_flat: a cell whose centroids' l3 / l2 exceeds it has no trustworthy
    normal, in (0, 1]; clearance: how far, in CELLS, a pierced cell must lie from the plane the ray ended on, and the two ends of the ray
    from the cell's own plane; radius: in CELLS, how near a ray must pass the centroid of a cell without a trustworthy normal; min_pierce
    (>= 1) and ratio (pierces a row, 0 .. 1024): a cell is moving with at least min_pierce pierces and ratio pierces for every row in
    it; reach, min_cells: VoxelMap.surface's."""
    __slots__ = ("skip_end", "skip_start", "max_steps", "max_flat", "clearance", "radius", "min_pierce", "ratio", "reach", "min_cells")

    def __init__(self, skip_end=2, skip_start=0, max_steps=ops.CARVE_MAX_STEPS, max_flat=0.15, clearance=0.3, radius=0.4, min_pierce=3, ratio=0.5,
                 reach=1, min_cells=5):
        what = "Carve"
        try:
            prm = ops.carve_ray_params(what, skip_end, skip_start, max_steps, max_flat, clearance, radius)
            reach, min_cells = ops.map_surface_params(what, reach, min_cells)
        except TypeError as e:
            raise ValueError(str(e)) from None
        for name, v in zip(("skip_end", "skip_start", "max_steps"), prm):
            self._set(name, v)
        self._set("max_flat", float(max_flat))
        self._set("clearance", prm[4])
        self._set("radius", prm[5])
        self._set("min_pierce", self._whole(min_pierce, "min_pierce", 1, (1 << 31) - 1))
        ops.carve_ratio_q(ratio, what)
        self._set("ratio", float(ratio))
        self._set("reach", reach)
        self._set("min_cells", min_cells)

    @property
    def ratio_q(self):
        """rint(ratio * 1024): what lpd_map_carve and lpd_scan_moving compare in integers"""
        return ops.carve_ratio_q(self.ratio, "Carve")


class Carving:
    """What remove_moving returns beside the filtered scans: moving [rows] bool on the device, True for an input row that lay in a
    moving cell (False for a row that got no cell); source = the VoxelMap of all input rows with its pierce counts; map = the carved
    VoxelMap; rows_removed, a Python int; pierce_info [6] int64 on the device (rays traversed, rows dropped, rays cut, cells stepped
    into, cells found, pierces counted); cells_removed: a Python int, one read-back when asked for."""
    __slots__ = ("moving", "source", "map", "rows_removed", "pierce_info")

    def __init__(self, moving, source, carved, rows_removed, pierce_info):
        self.moving, self.source, self.map, self.rows_removed, self.pierce_info = moving, source, carved, rows_removed, pierce_info

    @property
    def cells_removed(self):
        return 0 if self.map.left_behind is None else int(self.map.left_behind)


def moving_rows(vmap, points, lengths, poses, carve=None, scans=None):
    """Which rows of posed scans lie in a MOVING cell of `vmap` (lpd_scan_moving) -> [rows] bool on the device, one entry per row of the
    concatenated input; rows of scans outside `scans`, and rows that get no cell, are False.  vmap holds the counts of VoxelMap.pierce;
    carve: None = the Carve they were counted with.  Waits for the device once (see VoxelMap.pierce)."""
    what = "moving_rows"
    if not isinstance(vmap, VoxelMap):
        raise TypeError(f"{what}: vmap must be a VoxelMap, got {type(vmap).__name__}")
    pierced, carve = vmap._pierce_counts(what, carve)
    rows, lengths, p, a, b = _posed_input(what, points, lengths, poses, scans, vmap.device)
    with torch.no_grad(), torch.cuda.device(vmap.device):
        if int(lengths[a:b].sum()) == 0 or rows.shape[0] == 0:
            return torch.zeros((rows.shape[0],), dtype=torch.bool, device=vmap.device)
        flags, _ = ops.scan_moving(rows, drive._scan_offsets(lengths, vmap.device), p, vmap.origin, vmap.inv_cell, vmap.keys, vmap.acc, pierced,
                                   carve.min_pierce, carve.ratio_q, scan0=a, scan1=b)
        return flags != 0


def remove_moving(points, lengths, poses, cell=0.5, carve=None, origin=None, capacity=None, device=None):
    """A drive without what moved through it: the map of all scans (build_map), its surface, the rays that pierce every cell
    (VoxelMap.pierce), the rows that lie in a pierced cell (moving_rows), and the scans without those rows -> (points, lengths,
    Carving).  points / lengths / poses as build_map takes them; the returned points are one concatenated tensor on the device with
    host lengths, and go straight into drive.submaps_from_drive, build_map or odometry.estimate_poses with the same poses.  The
    compaction is submap.filter_scans, with its one read-back."""
    what = "remove_moving"
    carve = Carve() if carve is None else carve
    if not isinstance(carve, Carve):
        raise TypeError(f"{what}: carve must be a Carve, got {type(carve).__name__}")
    vmap = VoxelMap(cell, origin, capacity, device)
    rows, lengths = scan_input(what, points, lengths, vmap.device)
    vmap.insert(rows, lengths, poses)
    if vmap.keys is None:      # no row at all
        return rows, [int(n) for n in lengths], Carving(torch.zeros((rows.shape[0],), dtype=torch.bool, device=vmap.device), vmap, vmap, 0,
                                                          torch.zeros((6,), dtype=torch.int64, device=vmap.device))
    vmap.pierce(rows, lengths, poses, carve)
    moving = moving_rows(vmap, rows, lengths, poses, carve)
    kept, new_lengths = submap.filter_scans(rows, lengths, ~moving)
    removed = int(sum(int(n) for n in lengths)) - int(sum(new_lengths))
    return kept, new_lengths, Carving(moving, vmap, vmap.carved(carve), removed, vmap.pierce_info)
