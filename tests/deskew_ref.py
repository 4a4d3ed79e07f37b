"""Numpy restatement of the motion compensation of LiDAR sweeps (include/lpd_hip.h, "Motion compensation"; arithmetic in
csrc/lpd_deskew_math.h), composed from map_ref, loc_ref and odom_ref: the two motion rules, the per-scan part of the blend, the transform
of the rows of a scan table, and the odometry chain with times.  Used by tests/test_deskew_cpu.py (against csrc/lpd_deskew_math.h
compiled for the host) and tests/test_deskew_gpu.py (against the kernels, exact equality)."""
import math

import numpy as np

import loc_ref as L
import map_ref as M
import odom_ref as O

f32, f64, i64 = np.float32, np.float64, np.int64
IDENTITY = O.IDENTITY


def between(X, Y):
    """lpd_deskew_between: X, Y [n, 12] -> X^-1 Y packed as poses [n, 12]"""
    X, Y = np.asarray(X, dtype=f64).reshape(-1, 12), np.asarray(Y, dtype=f64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        R, t = M.between(X, Y)
    out = np.empty_like(X)
    out[:, M.ROT], out[:, M.TRA] = R, t
    return out


def drive_motions(poses):
    """lpd_drive_motions: poses [S, 12] -> motion [S, 12]"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    S = P.shape[0]
    if S == 1:
        return IDENTITY[None, :].copy()
    a = np.minimum(np.arange(S), S - 2)
    return between(P[a], P[a + 1])


def odom_motion(poses, t, first_motion=None):
    """lpd_deskew_odom_motion -> [12]"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    if t >= 2:
        return between(P[t - 2:t - 1], P[t - 1:t])[0]
    return IDENTITY.copy() if first_motion is None else np.asarray(first_motion, dtype=f64).reshape(12).copy()


def scan_part(motion):
    """lpd_deskew_scan for motions [n, 12] -> (dq [n, 4], dt [n, 3], ok [n] bool)"""
    m = np.asarray(motion, dtype=f64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        qa = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (m.shape[0], 1))
        qb = M.quat_any(np.ascontiguousarray(m[:, M.ROT]))
        d = (((qa[:, 0] * qb[:, 0]) + (qa[:, 1] * qb[:, 1])) + (qa[:, 2] * qb[:, 2])) + (qa[:, 3] * qb[:, 3])
        qb = np.where((d < 0)[:, None], -qb, qb)
        return qb - qa, m[:, M.TRA] - 0.0, np.isfinite(m).all(axis=1)


def row_pose(motion, a):
    """lpd_deskew_pose: the blended pose of every row, motion [n, 12] and a [n] -> [n, 12].  Written as lpd_map_blend(identity, motion, a)
    -- the definition -- through map_ref.blend; the header's split into a scan's and a row's part is held to it bit for bit by
    tests/test_deskew_cpu.py."""
    m = np.asarray(motion, dtype=f64).reshape(-1, 12)
    return M.blend(np.tile(IDENTITY, (m.shape[0], 1)), m, np.asarray(a, dtype=f64))


def row_ok(motion, times):
    """lpd_deskew_row_ok -> [n] bool"""
    tm = np.asarray(times, dtype=f32)
    with np.errstate(all="ignore"):
        return np.isfinite(np.asarray(motion, dtype=f64).reshape(-1, 12)).all(axis=1) & (tm >= f32(0.0)) & (tm <= f32(1.0))


def rows(xyz, times, motion, ref=0.5):
    """lpd_deskew_row for rows [n, 3] fp32 with their times [n] and the motions of their scans [n, 12] -> (out [n, 3] fp32, done [n])"""
    xyz, tm = np.asarray(xyz, dtype=f32), np.asarray(times, dtype=f32)
    ok = row_ok(motion, tm)
    out = xyz.copy()
    if ok.any():
        with np.errstate(all="ignore"):
            P = row_pose(np.asarray(motion, dtype=f64).reshape(-1, 12)[ok], tm[ok].astype(f64) - f64(ref))
            x, y, z = (xyz[ok, c].astype(f64) for c in range(3))
            for c in range(3):
                out[ok, c] = ((((P[:, 4 * c] * x) + (P[:, 4 * c + 1] * y)) + (P[:, 4 * c + 2] * z)) + P[:, 4 * c + 3]).astype(f32)
    return out, ok


def deskew(points, offsets, times, motion, ref=0.5, scan0=0, scan1=None, out=None):
    """lpd_scan_deskew -> (out [rows, 3] fp32, info [2] int64 = rows transformed, rows passed through).  out: what the rows that the
    call does not write keep (zeros when None)"""
    pts = np.asarray(points, dtype=f32)
    m = np.asarray(motion, dtype=f64).reshape(-1, 12)
    scan1 = m.shape[0] if scan1 is None else scan1
    out = np.zeros((pts.shape[0], 3), dtype=f32) if out is None else np.array(out, dtype=f32)
    got = M.row_scans(offsets, scan0, scan1, pts.shape[0])
    if got is None:
        return out, np.zeros(2, dtype=i64)
    g, scan, _ = got
    o, ok = rows(pts[g, :3], np.asarray(times, dtype=f32)[g], m[scan], ref)
    out[g] = o
    return out, np.array([int(ok.sum()), int((~ok).sum())], dtype=i64)


def deskew_drive(points, lengths, times, poses=None, motions=None, ref=0.5):
    """odometry.deskew_scans of a whole drive"""
    m = drive_motions(poses) if motions is None else motions
    return deskew(points, M.offsets_of(lengths), times, m, ref)


def scan_fractions(stamps, lengths):
    """odometry.scan_fractions -> [R] fp32"""
    t = np.asarray(stamps, dtype=f64)
    out = np.zeros(len(t), dtype=f32)
    off = M.offsets_of(lengths)
    for a, b in zip(off[:-1], off[1:]):
        if b > a and t[a:b].max() > t[a:b].min():
            out[a:b] = ((t[a:b] - t[a:b].min()) / (t[a:b].max() - t[a:b].min())).astype(f32)
    return out


def estimate(points, lengths, times, start=None, cell=1.0, keep_m=60.0, refresh=10, iters=8, dmax=None, min_inliers=50, max_flat=0.3, reach=1,
             min_cells=5, min_share=0.19, max_jump=5.0, first_motion=None, ref=0.5, on_map=None):
    """odometry.estimate_poses with times: odom_ref.estimate's loop with every scan deskewed under its predicted motion before it is
    localised -> odom_ref.estimate's dict and points [R, 3] = the deskewed rows, motions [S, 12], passed = the rows passed through"""
    pts = np.asarray(points, dtype=f32)[:, :3].copy()
    tm = np.asarray(times, dtype=f32)
    lengths = np.asarray(lengths, dtype=i64)
    S = len(lengths)
    off = M.offsets_of(lengths)
    P = np.zeros((S, 12), dtype=f64)
    P[0] = IDENTITY if start is None else np.asarray(start, dtype=f64).reshape(12)
    origin = P[0, M.TRA].copy()
    pred, insert_pose, motions = np.zeros((S, 12), dtype=f64), np.zeros((S, 12), dtype=f64), np.zeros((S, 12), dtype=f64)
    info = np.zeros((S, 4), dtype=np.int32)
    state = np.zeros(S, dtype=np.int32)
    dm = L.schedule(cell, iters) if dmax is None else tuple(dmax)
    keep_cells, sq = int(math.ceil(keep_m / cell)), O.share_q(min_share)
    cells, left, passed = O.empty_cells(), [], 0
    desk = np.zeros_like(pts)
    for t in range(S):
        P[t] = pred[t] = O.predict(P, t, first_motion)
        motions[t] = odom_motion(P, t, first_motion)
        a, b = int(off[t]), int(off[t + 1])
        desk[a:b], ok = rows(pts[a:b], tm[a:b], np.tile(motions[t], (b - a, 1)), ref)
        passed += int((~ok).sum())
        if t > 0 and len(cells.keys) == 0:      # an empty map: no correspondence, every step of a valid scan refused
            good = bool(L.scan_valid(P[t:t + 1], off[t:t + 2], len(desk), 0, 1)[0])
            info[t] = (1, 0, len(dm) - 1, 0) if good else (-1, 0, 0, 0)
        elif t > 0:
            r = L.localize(L.surface(cells, reach, min_cells), desk, off[t:t + 2], P[t:t + 1], origin, cell, dm, min_inliers, max_flat)
            P[t], info[t] = r["pose"][0], r["info"][0]
        state[t], P[t], insert_pose[t] = O.accept(pred[t], P[t], info[t], int(lengths[t]), t, sq, max_jump)
        cells = M.insert(desk, off, insert_pose, origin, cell, t, t + 1, into=cells)
        if refresh is not None and (t + 1) % refresh == 0 and t + 1 < S:
            cells, n = O.crop(cells, P[t], origin, cell, keep_cells)
            left.append(n)
        if on_map is not None:
            on_map(t, cells)
    n_rows = lengths.astype(f64)
    inliers = np.where(n_rows > 0, info[:, 3].astype(f64) / np.maximum(n_rows, 1.0), 0.0)
    return dict(poses=P, pred=pred, valid=state == 1, info=info, inliers=inliers, cells=cells, left=left, insert_pose=insert_pose, points=desk,
                motions=motions, passed=passed)
