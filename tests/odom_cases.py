"""Cases and bounds that tests/test_odometry_cpu.py and tests/test_odometry_gpu.py share.  The bounds are measured on the restatement
alone (tests/odom_ref.py on the CPU; test_odometry_cpu.py prints the MEASURE lines and checks the factor) and are written into DESIGN.md
13q; no number here comes from a kernel."""
import math

import numpy as np

import align_ref
import icp_ref
import loc_cases as C
import map_ref as M
import odom_ref as O

f32, f64, i64 = np.float32, np.float64, np.int64

SEEDS = (1, 2, 3, 4)
CELLS = (1.0, 0.5)
# The quality drives: street_drive(seed, S = 12, step = 1 m, rows = 6000, turn = 0.5 degrees a scan; roll and pitch drawn afresh within a
# degree for every scan), scan 0 at its true pose, every later scan started from the constant-velocity prediction, the default eight
# steps, a crop to KEEP_M after scan 5 (REFRESH = 6).  At 1 m cells scan 1 starts at pose 0, a full metre off.  At 0.5 m cells that
# start is two cells off and does NOT always converge (seed 1 ended 1.9 m off, with an inlier share of 0.07 at scan 1): those drives
# get FIRST_MOTION, one nominal step straight ahead -- a speed prior, not the truth.  Measured on the restatement, the worst over the
# four seeds and the eleven estimated scans of each:
#   1 m cells    0.2065 degrees, 0.0392 m; inlier shares 0.3933 .. 0.5893
#   0.5 m cells  0.2388 degrees, 0.0291 m; inlier shares 0.2177 .. 0.6222
# The bounds are 1.5 x the measured values; the margin covers seeds that were not measured.  Every scan was accepted.
DRIVE_S, DRIVE_STEP, DRIVE_ROWS, DRIVE_TURN_DEG = 12, 1.0, 6000, 0.5
REFRESH, KEEP_M = 6, 20.0
NOMINAL_MOTION = np.array([1.0, 0.0, 0.0, DRIVE_STEP, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
FIRST_MOTION = {1.0: None, 0.5: NOMINAL_MOTION}
MEASURED_ROT_DEG = {1.0: 0.2065, 0.5: 0.2388}
MEASURED_TRANS_M = {1.0: 0.0392, 0.5: 0.0291}
WORST_ROT_DEG = {c: 1.5 * v for c, v in MEASURED_ROT_DEG.items()}
WORST_TRANS_M = {c: 1.5 * v for c, v in MEASURED_TRANS_M.items()}
# The lost scans: scan LOST_AT of the same drives replaced by lost_scan -- the walls of ANOTHER scene seen from the same pose, without
# a ground.  Accepted or not, the localiser runs on them; the largest inlier share it ends with, over the four seeds: 0.1683 at 1 m
# cells, 0.1697 at 0.5 m cells.  The smallest share of a true scan above: 0.2177.  The default min_share is the geometric mean of the
# largest lost and the smallest true share, sqrt(0.1697 * 0.2177) = 0.1922 -> 0.19.
LOST_AT = 7
LOST_SHARE_MAX = 0.1697
TRUE_SHARE_MIN = 0.2177
MIN_SHARE = 0.19
# The end-to-end measure: the occupied 1 m cells of the drive's rows at the estimated poses (1 m odometry cells) over those at the true
# poses, the worst of the four seeds: 3100 / 3092 = 1.0026.  The bound is 1 + 1.5 x (ratio - 1).
OCCUPIED_RATIO = 1.0026
OCCUPIED_BOUND = 1.0 + 1.5 * (OCCUPIED_RATIO - 1.0)


def street_drive(seed, S=DRIVE_S, step=DRIVE_STEP, rows=DRIVE_ROWS, turn_deg=DRIVE_TURN_DEG):
    """-> dict(points [S rows, 3] fp32, lengths [S], truth [S, 12], scene, seed): S scans of `rows` rows `step` metres apart along a
    street of align_ref.scene(seed), the heading turning by turn_deg a scan, roll and pitch within a degree, each scan drawn afresh by
    loc_cases.sensor_scan in its own TRUE sensor frame."""
    sc = align_ref.scene(seed)
    g = np.random.default_rng(7000 + seed)
    head = g.uniform(0.0, 2.0 * np.pi)
    pos = g.uniform(-15.0, 15.0, 2)
    truth, pts = [], []
    for k in range(S):
        R = icp_ref.rot_xyz(math.radians(g.uniform(-1.0, 1.0)), math.radians(g.uniform(-1.0, 1.0)), head)
        t = np.concatenate((pos, [C.SENSOR_HEIGHT + g.normal(0.0, 0.02)]))
        truth.append(C.pose12(R, t))
        pts.append(C.sensor_scan(sc, R, t, 1000 * seed + k, rows))
        pos = pos + step * np.array([math.cos(head), math.sin(head)])
        head += math.radians(turn_deg)
    return dict(points=np.concatenate(pts), lengths=np.full(S, rows, dtype=i64), truth=np.array(truth), scene=sc, seed=seed)


def lost_scan(drive, k):
    """what replaces scan k of a drive: as many rows of the walls of ANOTHER scene seen from the same pose, no ground -> [rows, 3] fp32"""
    P = drive["truth"][k].reshape(3, 4)
    rows = int(drive["lengths"][k])
    walls = align_ref.submap(align_ref.scene(100 + drive["seed"]), P[:2, 3], 0.0, 9000 + drive["seed"], n=rows, radius=C.RADIUS).astype(f64)
    walls[:, 2] -= P[2, 3]
    return (walls @ P[:, :3]).astype(f32)


def with_lost_scan(drive, k=LOST_AT):
    """the drive with scan k replaced by lost_scan -> (points, lengths)"""
    pts = drive["points"].copy()
    off = M.offsets_of(drive["lengths"])
    pts[off[k]:off[k + 1]] = lost_scan(drive, k)
    return pts, drive["lengths"]


def without_scan(drive, k=LOST_AT):
    """the scans 0 .. k of the drive with scan k emptied (no rows, length 0) -> (points, lengths)"""
    off = M.offsets_of(drive["lengths"])
    lengths = drive["lengths"][:k + 1].copy()
    lengths[k] = 0
    return drive["points"][:off[k]], lengths


def estimate(drive, cell, points=None, lengths=None, **kw):
    """odom_ref.estimate of a drive from its true first pose, with the quality drives' crop and first motion"""
    kw = dict(dict(refresh=REFRESH, keep_m=KEEP_M, min_share=MIN_SHARE, first_motion=FIRST_MOTION[cell]), **kw)
    return O.estimate(drive["points"] if points is None else points, drive["lengths"] if lengths is None else lengths, drive["truth"][0], cell, **kw)


def errors(poses, truth):
    """-> [(degrees, metres)] of every pose against its truth"""
    return C.errors(poses, truth)


def hand_drive(n=6, step=(0.5, 0.25, 0.0)):
    """a straight constant-velocity drive whose arithmetic is exact: identity rotation, translations k * step in binary fractions"""
    P = np.tile(O.IDENTITY, (n, 1))
    P[:, M.TRA] = np.arange(n)[:, None] * np.asarray(step, dtype=f64)[None, :]
    return P


# ---- the cases that the GPU file runs on the device as well ------------------------------------------------------------------------------------
def predict_cases():
    """-> [(name, poses [4, 12], t, first_motion or None)]"""
    rng = np.random.default_rng(11)
    out = []
    straight = hand_drive(4)
    for t in (0, 1, 2, 3):
        out.append((f"straight t={t}", straight, t, None))
    quarter = np.array([C.pose12(icp_ref.rot_xyz(0.0, 0.0, k * math.pi / 2), [math.cos(k * math.pi / 2), math.sin(k * math.pi / 2), 0.0]) for k in range(4)])
    out += [("quarter turn t=2", quarter, 2, None), ("quarter turn t=3", quarter, 3, None)]
    utm = np.array([C.pose12(icp_ref.rot_xyz(0.01 * k, -0.02, 0.3 + 0.05 * k), [500000.0 + 1.3 * k, 5.7e6 + 0.7 * k * k, 120.0 + 0.01 * k]) for k in range(4)])
    out += [("UTM t=2", utm, 2, None), ("UTM t=3", utm, 3, None)]
    for k in range(6):
        P = np.array([C.pose12(icp_ref.rot_xyz(*rng.uniform(-0.3, 0.3, 3)), rng.uniform(-50.0, 50.0, 3)) for _ in range(4)])
        out.append((f"random {k}", P, 2 + k % 2, None))
    nan2, nan1 = utm.copy(), utm.copy()
    nan2[1, 5] = np.nan
    nan1[2, 11] = np.inf
    out += [("NaN at t-2", nan2, 3, None), ("inf at t-1", nan1, 3, None), ("NaN at t-1 of t=2", nan2, 2, None)]
    motion = C.pose12(icp_ref.rot_xyz(0.0, 0.01, 0.02), [1.0, 0.05, 0.0])
    out += [("t=0 with a first_motion", utm, 0, motion), ("t=1 with a first_motion", utm, 1, motion), ("t=1 without", utm, 1, None),
            ("t=2 with a first_motion", utm, 2, motion)]
    return out


def accept_cases():
    """-> [(name, pred [12], pose [12], info [4], len, t, share_q, max_jump, accepted)]"""
    pred = C.pose12(icp_ref.rot_xyz(0.0, 0.0, 0.2), [3.0, 4.0, 1.0])
    pose = C.pose12(icp_ref.rot_xyz(0.01, 0.0, 0.21), [3.0 + 0.3, 4.0 + 0.4, 1.0])      # 0.5 m from pred, up to rounding
    d = pose[M.TRA] - pred[M.TRA]
    jump = float(np.sqrt(M.dot3(d[0], d[1], d[2], d[0], d[1], d[2])))
    while not jump * jump >= M.dot3(d[0], d[1], d[2], d[0], d[1], d[2]):      # the smallest max_jump whose square reaches the squared distance
        jump = float(np.nextafter(jump, np.inf))
    while float(np.nextafter(jump, 0.0)) ** 2 >= M.dot3(d[0], d[1], d[2], d[0], d[1], d[2]):
        jump = float(np.nextafter(jump, 0.0))
    out = []
    # corr * 1024 == share_q * len: 300 * 1024 == 100 * 3072
    for corr, want in ((300, 1), (299, 0), (301, 1)):
        out.append((f"share equality, corr={corr}", pred, pose, (1, 3, 5, corr), 3072, 4, 100, 5.0, want))
    out.append(("share equality, one row more", pred, pose, (1, 3, 5, 300), 3073, 4, 100, 5.0, 0))
    out.append(("share equality, one row fewer", pred, pose, (1, 3, 5, 300), 3071, 4, 100, 5.0, 1))
    out.append(("products beyond int32", pred, pose, (1, 8, 0, 1 << 22), 1 << 22, 4, 1024, 5.0, 1))
    out.append(("products beyond int32, one short", pred, pose, (1, 8, 0, (1 << 22) - 1), 1 << 22, 4, 1024, 5.0, 0))
    out.append(("max_jump at equality", pred, pose, (1, 8, 0, 2000), 3000, 2, 100, jump, 1))
    out.append(("max_jump one ulp below", pred, pose, (1, 8, 0, 2000), 3000, 2, 100, float(np.nextafter(jump, 0.0)), 0))
    out.append(("max_jump one ulp above", pred, pose, (1, 8, 0, 2000), 3000, 2, 100, float(np.nextafter(jump, np.inf)), 1))
    out.append(("max_jump 0, pose == pred", pred, pred, (1, 8, 0, 2000), 3000, 2, 100, 0.0, 1))
    out.append(("zero steps applied", pred, pose, (1, 0, 8, 2000), 3000, 2, 100, 5.0, 0))
    out.append(("an empty scan", pred, pose, (1, 1, 7, 0), 0, 2, 0, 5.0, 0))
    out.append(("an invalid scan", pred, pose, (-1, 0, 0, 0), 3000, 2, 100, 5.0, 0))
    bad = pose.copy()
    bad[3] = np.nan
    out.append(("a NaN translation", pred, bad, (1, 8, 0, 2000), 3000, 2, 100, 5.0, 0))
    out.append(("scan 0 with rows", pred, pose, (0, 0, 0, 0), 10, 0, 100, 0.0, 1))
    out.append(("scan 0 without rows", pred, pose, (0, 0, 0, 0), 0, 0, 100, 5.0, 0))
    out.append(("scan 0 with a NaN pose", pred, bad, (0, 0, 0, 0), 10, 0, 100, 5.0, 0))
    return out


def keep_cases():
    """-> [(centre [12], origin [3], cell, keep_cells, q [n, 3])]"""
    out = []
    origin = np.array([100.0, -50.0, 2.0])
    centre = C.pose12(icp_ref.rot_xyz(0.0, 0.0, 0.4), origin + np.array([10.5, -3.5, 0.5]))      # cell (10, -4, 0) at 1 m
    for keep in (0, 1, 3):
        q = np.array([[10 + dx, -4 + dy, dz] for dx in (-keep - 1, -keep, 0, keep, keep + 1) for dy in (-keep - 1, -keep, 0, keep, keep + 1)
                      for dz in (-keep - 1, -keep, 0, keep, keep + 1)])
        out.append((centre, origin, 1.0, keep, q))
    lim = M.QLIM
    edge = np.array([[-lim, 0, 0], [lim - 1, 0, 0], [0, -lim, lim - 1], [lim - 1, lim - 1, lim - 1], [-lim, -lim, -lim], [lim - 6, 3, 0], [lim - 7, 3, 0]])
    far = C.pose12(np.eye(3), origin + np.array([(lim - 3) * 0.5 + 0.25, 1.75, 0.25]))      # cell (2^20 - 3, 3, 0) at 0.5 m
    out.append((far, origin, 0.5, 3, edge))
    out.append((far, origin, 0.5, 2 * lim, edge))
    nan = centre.copy()
    nan[0] = np.nan
    out.append((nan, origin, 1.0, 0, edge))
    nocell = C.pose12(np.eye(3), origin + np.array([4.0e6, 0.0, 0.0]))      # finite, but beyond the 2^20 cells of 1 m
    out.append((nocell, origin, 1.0, 0, edge))
    return out
