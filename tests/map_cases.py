"""Cases and bounds that tests/test_map_cpu.py and tests/test_map_gpu.py share.  The bounds are measured on the restatements alone
(tests/map_ref.py against its own np.longdouble version; test_map_cpu.py prints the MEASURE lines and checks the factor of two) and
are written into DESIGN.md 13m; no number here comes from a kernel."""
import numpy as np

import drive_ref

# lpd_drive_correct with nodes that did not move (node_pose == poses[node_scan]) on unmoved_case(): the output against the input pose.
# Measured (the larger of |float64 - extended| and |extended - input|): rotation entries 3.3e-16 -- the float64 rounding of
# R_s (R_s^T R_i) and of the normalised quaternion; translation 1.3e-24 of the largest coordinate (5.7e6 m), i.e. 7e-18 m -- the
# candidate's translation R_s (R_s^T (t_i - t_s)) + t_s departs from t_i by 1e-15 of a step of metres, and the last addition rounds
# that away at the ulp of a UTM northing.  Twice the measured values, rounded up:
CORRECT_ROT_BOUND = 7.0e-16
CORRECT_TRANS_BOUND = 2.5e-24      # relative to the largest |coordinate| of the drive
# lpd_map_insert's fp32 world rows against extended precision on utm_case() (points within 60 m of the sensor, the origin on the drive,
# poses at UTM scale).  Measured 1.17e-5 m -- four fp32 roundings at up to 150 m; twice that, rounded up:
ROWS_BOUND = 2.4e-5


def unmoved_case():
    """-> (poses [S, 12], D [S], node_scan [V]): a 300-scan drive at UTM scale with nodes every 7 .. 23 scans"""
    rng = np.random.default_rng(77)
    _, poses = drive_ref.make_drive(rng, np.ones(300, dtype=np.int64), step=0.7, heading_noise=0.05, origin=(5.7e6, 6.2e5, 120.0))
    D = drive_ref.distance(drive_ref.steps(poses))
    ns = np.cumsum(rng.integers(7, 24, 16)).astype(np.int32)
    return poses, D, ns[ns < 300]


def utm_case():
    """-> (points [rows, 3] fp32, lengths [S], poses [S, 12], origin [3]): 40 scans of 50 .. 300 rows at a UTM origin"""
    rng = np.random.default_rng(78)
    lengths = rng.integers(50, 300, 40).astype(np.int64)
    points, poses = drive_ref.make_drive(rng, lengths, step=1.5, origin=(5.7e6, 6.2e5, 120.0), point_scale=60.0)
    return points, lengths, poses, poses[0, [3, 7, 11]].copy()


def lap_case(seed, V=48, per_node=3, n_points=8000):
    """The end-to-end scene: pgo_ref.two_laps(seed, V) with per_node scans to a node.  The true pose of a scan between two nodes is
    the blend of the nodes' true poses; the drifted drive keeps the true odometry rigid around each drifted node.
    -> dict(graph, node_scan [V], gt [S, 12], start [S, 12], points, lengths)"""
    import map_ref as M
    import pgo_ref as R
    g = R.two_laps(seed, V)
    gt, start = [], []
    for k in range(V):
        for j in range(per_node if k < V - 1 else 1):
            t = gt_k = g["gt"][k]
            if j:
                t = M.blend(g["gt"][[k]], g["gt"][[k + 1]], np.array([j / per_node]))[0]
            gt.append(t)
            start.append(R.mul12(g["start"][k], R.mul12(R.inv12(gt_k), t)))
    gt, start = np.array(gt), np.array(start)
    points, lengths = M.facade_scene(seed, gt, n_points=n_points)
    return dict(graph=g, node_scan=(np.arange(V) * per_node).astype(np.int32), gt=gt, start=start, points=points, lengths=lengths)
