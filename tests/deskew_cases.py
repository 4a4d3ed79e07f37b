"""Cases and bounds that tests/test_deskew_cpu.py and tests/test_deskew_gpu.py share: drives whose sweeps are skewed by the motion of
the sensor, and the rows at the edges of the definition.  The bounds are measured on the restatement alone (tests/deskew_ref.py on the
CPU; test_deskew_cpu.py prints the MEASURE lines and checks the factor) and are written into DESIGN.md 13q.1; no number here comes from
a kernel."""
import math

import numpy as np

import align_ref
import icp_ref
import loc_cases as LC
import map_ref as M
import odom_cases as OC

f32, f64, i64 = np.float32, np.float64, np.int64

SEEDS = (1, 2, 3, 4)
# The skewed drives: (step in metres, turn in degrees) a scan.  12 scans of 6000 rows, 1 m cells, a crop after scan 5, first_motion =
# one nominal step with the nominal turn.
DRIVES = {"1m2deg": (1.0, 2.0), "1.5m2.5deg": (1.5, 2.5), "2m3deg": (2.0, 3.0)}
DRIVE_S, DRIVE_ROWS, REFRESH, KEEP_M, CELL, REF = 12, 6000, 6, 20.0, 1.0, 0.5
# Condition 1, the residual with the TRUE motion: the largest distance of a deskewed row from its clean row over the largest skew of
# the drive (the largest distance of a skewed row from its clean row: 0.92 .. 0.93 m, 1.28 .. 1.29 m and 1.63 .. 1.65 m), measured on
# the restatement, per drive the seeds 1 .. 4.  What is left is the chord that the blend takes for the arc, and grows with the turn.
# The bound is the design's: 0.05.
RESIDUAL_RATIO = {"1m2deg": (0.01415, 0.01419, 0.01416, 0.01422), "1.5m2.5deg": (0.01927, 0.01904, 0.01929, 0.01934),
                  "2m3deg": (0.02419, 0.02403, 0.02396, 0.02398)}
RESIDUAL_BOUND = 0.05
# Condition 2, the odometry: the worst rotation (degrees) and translation (metres) error over the four seeds and the eleven estimated
# scans of each, measured on the restatement: the clean rows, the skewed rows as they are, the skewed rows with times.  The deskewed
# errors must be at most FACTOR of the skewed ones; the absolute bounds on the deskewed errors are 1.5 x the measured values.
#                 clean                skewed, as they are    skewed, with times     with times over as they are
#   1.5m2.5deg    0.1179 deg 0.0503 m  0.4854 deg 0.1988 m    0.1144 deg 0.0539 m    0.24 and 0.27
#   2m3deg        0.1509 deg 0.0533 m  0.4270 deg 0.2325 m    0.1429 deg 0.0578 m    0.33 and 0.25
# A FINDING ABOUT THE SLOWEST DRIVE: at 1 m and 2 degrees a scan the restatement does NOT hold the factor on these drives -- clean
# 0.1555 deg 0.0708 m, as they are 0.2439 deg 0.0961 m, with times 0.1538 deg 0.0679 m: 0.63 and 0.71.  Deskewing takes the errors back
# to those of the clean rows there as well, but seed 2's clean rows alone end 0.1555 deg and 0.0708 m off, more than half of what the
# skew of so slow a drive adds, so no deskewing can halve them.  Condition 2 is therefore checked at 1.5 m with 2.5 degrees and at 2 m
# with 3 degrees a scan, where the restatement holds it; condition 1 is checked on all three.
ODOMETRY_DRIVES = ("1.5m2.5deg", "2m3deg")
CLEAN = {"1.5m2.5deg": (0.1179, 0.0503), "2m3deg": (0.1509, 0.0533)}
SKEWED = {"1.5m2.5deg": (0.4854, 0.1988), "2m3deg": (0.4270, 0.2325)}
DESKEWED = {"1.5m2.5deg": (0.1144, 0.0539), "2m3deg": (0.1429, 0.0578)}
FACTOR = 0.5
WORST_ROT_DEG = {k: 1.5 * v[0] for k, v in DESKEWED.items()}
WORST_TRANS_M = {k: 1.5 * v[1] for k, v in DESKEWED.items()}


# ---- rigid motions along a constant twist ----------------------------------------------------------------------------------------------------
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def twist_of(R, t):
    """the twist (w [3], v [3]) with exp(twist) = (R | t)"""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = math.acos(c)
    if th < 1e-12:
        return np.zeros(3), np.asarray(t, dtype=f64).copy()
    w = th / (2.0 * math.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    K = _hat(w)
    V = np.eye(3) + (1.0 - math.cos(th)) / th ** 2 * K + (th - math.sin(th)) / th ** 3 * (K @ K)
    return w, np.linalg.solve(V, t)


def along_twist(w, v, s):
    """exp(s twist) for every s [n] -> (R [n, 3, 3], t [n, 3])"""
    s = np.asarray(s, dtype=f64)
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.tile(np.eye(3), (len(s), 1, 1)), s[:, None] * v[None, :]
    K = _hat(w / th)
    a = s * th
    R = np.eye(3)[None] + np.sin(a)[:, None, None] * K[None] + (1.0 - np.cos(a))[:, None, None] * (K @ K)[None]
    V = s[:, None, None] * np.eye(3)[None] + ((1.0 - np.cos(a)) / th)[:, None, None] * K[None] + ((a - np.sin(a)) / th)[:, None, None] * (K @ K)[None]
    return R, V @ v


def skewed_drive(seed, step, turn_deg, S=DRIVE_S, rows=DRIVE_ROWS, ref=REF):
    """-> dict(clean [S rows, 3] fp32, points = the skewed rows [S rows, 3] fp32, times [S rows] fp32, lengths [S], truth [S, 12],
    motions [S, 12], skew = the largest distance of a skewed row from its clean row, scene, seed).  A street drive as
    odom_cases.street_drive with roll and pitch fixed for the drive; pose k is the sensor's at the START of sweep k, and during the
    sweep the sensor moves along the constant twist from pose k to pose k + 1 (motions[k] = pose_k^-1 pose_k+1, the TRUE motion).  The
    clean rows of scan k are loc_cases.sensor_scan from the pose at the time `ref` of the sweep -- truth[k]; every row gets a time
    drawn uniformly from 0 .. 1 and is re-expressed in the frame the sensor has at that time: that is the skewed row."""
    sc = align_ref.scene(seed)
    g = np.random.default_rng(8000 + seed)
    head = g.uniform(0.0, 2.0 * np.pi)
    pos = g.uniform(-15.0, 15.0, 2)
    roll, pitch = math.radians(g.uniform(-1.0, 1.0)), math.radians(g.uniform(-1.0, 1.0))
    starts = []
    for k in range(S + 1):
        starts.append((icp_ref.rot_xyz(roll, pitch, head), np.concatenate((pos, [LC.SENSOR_HEIGHT]))))
        pos = pos + step * np.array([math.cos(head), math.sin(head)])
        head += math.radians(turn_deg)
    clean, skewed, times, truth, motions = [], [], [], [], []
    skew = 0.0
    for k in range(S):
        (R0, t0), (R1, t1) = starts[k], starts[k + 1]
        Rm, tm = R0.T @ R1, R0.T @ (t1 - t0)
        w, v = twist_of(Rm, tm)
        Rr, tr = along_twist(w, v, [ref])
        Rref, tref = R0 @ Rr[0], R0 @ tr[0] + t0      # the sensor at the time ref
        c = LC.sensor_scan(sc, Rref, tref, 2000 * seed + k, rows)
        s = g.random(rows).astype(f32)
        Rs, ts = along_twist(w, v, s.astype(f64) - ref)      # the sensor at the row's time, in the frame of the time ref (one twist)
        p = np.einsum("nji,nj->ni", Rs, c.astype(f64) - ts).astype(f32)      # R_s^T (c - t_s)
        skew = max(skew, float(np.linalg.norm(p.astype(f64) - c.astype(f64), axis=1).max()))
        clean.append(c)
        skewed.append(p)
        times.append(s)
        truth.append(LC.pose12(Rref, tref))
        motions.append(LC.pose12(Rm, tm))
    return dict(clean=np.concatenate(clean), points=np.concatenate(skewed), times=np.concatenate(times), lengths=np.full(S, rows, dtype=i64),
                truth=np.array(truth), motions=np.array(motions), skew=skew, scene=sc, seed=seed)


def nominal_motion(step, turn_deg):
    """one nominal step straight ahead with the nominal turn: a speed prior, not the truth"""
    return LC.pose12(icp_ref.rot_xyz(0.0, 0.0, math.radians(turn_deg)), [step, 0.0, 0.0])


def estimate_kw(step, turn_deg):
    return dict(cell=CELL, refresh=REFRESH, keep_m=KEEP_M, min_share=OC.MIN_SHARE, first_motion=nominal_motion(step, turn_deg))


def errors(poses, truth):
    return LC.errors(poses, truth)


# ---- the rows at the edges of the definition -------------------------------------------------------------------------------------------------
def boundary_times():
    """times at 0, 1, their neighbours on both sides, NaN, +-inf and -0.0 -> [n] fp32"""
    one, zero = f32(1.0), f32(0.0)
    return np.array([0.0, 1.0, np.nextafter(zero, one), np.nextafter(zero, -one), np.nextafter(one, zero), np.nextafter(one, f32(2.0)), np.nan, np.inf,
                     -np.inf, -0.0, 0.5, 0.25], dtype=f32)


def boundary_motions():
    """-> [(name, motion [12])]: the identity, a half turn less a degree about a tilted axis, a general one and one with a NaN"""
    ax = np.array([0.3, -0.2, 0.9])
    ax /= np.linalg.norm(ax)
    R179, _ = along_twist(ax * math.radians(179.0), np.zeros(3), [1.0])
    nan = LC.pose12(icp_ref.rot_xyz(0.01, -0.02, 0.05), [1.5, 0.1, -0.02])
    nan[6] = np.nan
    inf = LC.pose12(np.eye(3), [np.inf, 0.0, 0.0])
    return [("identity", np.array([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])),
            ("179 degrees", LC.pose12(R179[0], [0.5, -0.25, 0.125])),
            ("general", LC.pose12(icp_ref.rot_xyz(0.01, -0.02, 0.05), [1.5, 0.1, -0.02])),
            ("a NaN", nan), ("an inf translation", inf)]


def boundary_table(seed=3):
    """one scan a boundary motion, every boundary time in each, random rows out to 100 m -> (points [n, 3] fp32, lengths, times [n]
    fp32, motions [S, 12])"""
    g = np.random.default_rng(seed)
    tm, mo = boundary_times(), boundary_motions()
    reps = 3
    n = len(tm) * reps
    pts = g.uniform(-100.0, 100.0, (len(mo) * n, 3)).astype(f32)
    pts[0] = (-0.0, 0.0, -0.0)
    return pts, np.full(len(mo), n, dtype=i64), np.tile(np.repeat(tm, reps), len(mo)), np.array([m for _, m in mo])


def random_table(seed, lengths, reach=100.0, step=3.0, turn_deg=10.0):
    """random rows out to `reach` metres with random times, a random motion a scan of up to `step` metres and `turn_deg` degrees ->
    (points [n, 3] fp32, lengths, times [n] fp32, motions [S, 12])"""
    g = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=i64)
    n = int(lengths.sum())
    pts = g.uniform(-reach, reach, (max(n, 1), 3)).astype(f32)
    tm = g.random(max(n, 1)).astype(f32)
    mo = np.array([LC.pose12(icp_ref.rot_xyz(*(math.radians(a) for a in g.uniform(-turn_deg, turn_deg, 3))), g.uniform(-step, step, 3)) for _ in lengths])
    return pts, lengths, tm, mo
