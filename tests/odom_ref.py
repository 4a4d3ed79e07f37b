"""Numpy restatement of LiDAR odometry (include/lpd_hip.h, "LiDAR odometry"; arithmetic in csrc/lpd_odom_math.h), composed from
map_ref and loc_ref: the constant-velocity start of a scan, the decision on a localised scan, the crop of a map around a centre, the set
of cells an insert touches, and the whole chain.  The table is map_ref.Cells in key order -- no hash table, so slot independence is
built in.  Used by tests/test_odometry_cpu.py (against csrc/lpd_odom_math.h compiled for the host) and tests/test_odometry_gpu.py
(against the kernels, exact equality)."""
import math

import numpy as np

import loc_ref as L
import map_ref as M

f32, f64, i64 = np.float32, np.float64, np.int64
SHARE_UNITS = 1024
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def share_q(min_share):
    return int(round(float(min_share) * SHARE_UNITS))


def predict(poses, t, first_motion=None):
    """lpd_odom_predict_pose -> [12] float64"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        if t <= 1:
            if t == 1 and first_motion is not None:
                m = np.asarray(first_motion, dtype=f64).reshape(1, 12)
                return M.compose(P[0:1], np.ascontiguousarray(m[:, M.ROT]), np.ascontiguousarray(m[:, M.TRA]))[0]
            return P[0].copy()
        P1, P2 = P[t - 1:t], P[t - 2:t - 1]
        if not (np.isfinite(P1).all() and np.isfinite(P2).all()):
            return P1[0].copy()
        c = M.candidate(P2, P1, P1)
        return M.blend(c, c, np.zeros(1))[0]


def accepted(pred, pose, info, length, t, sq, max_jump):
    """lpd_odom_accepted"""
    pred, pose = np.asarray(pred, dtype=f64).reshape(12), np.asarray(pose, dtype=f64).reshape(12)
    if t == 0:
        return bool(np.isfinite(pose).all() and length > 0)
    if not (int(info[0]) == 1 and int(info[1]) >= 1 and length > 0):
        return False
    if not int(info[3]) * SHARE_UNITS >= int(sq) * int(length):
        return False
    with np.errstate(all="ignore"):
        d = pose[M.TRA] - pred[M.TRA]
        return bool(M.dot3(d[0], d[1], d[2], d[0], d[1], d[2]) <= f64(max_jump) * f64(max_jump))


def accept(pred, pose, info, length, t, sq, max_jump):
    """lpd_odom_accept_pose -> (state, pose [12], insert_pose [12])"""
    ok = accepted(pred, pose, info, length, t, sq, max_jump)
    pose = np.asarray(pose, dtype=f64).reshape(12)
    return (1, pose.copy(), pose.copy()) if ok else (0, np.asarray(pred, dtype=f64).reshape(12).copy(), np.full(12, np.nan))


def centre_cell(centre, origin, cell):
    """lpd_odom_centre_cell -> (has, qc [3] int64)"""
    centre = np.asarray(centre, dtype=f64).reshape(1, 12)
    if not np.isfinite(centre).all():
        return False, np.zeros(3, dtype=i64)
    _, u = M.rel(centre, origin)
    q, ok = M.index(u[0], M.inv_cell(cell))
    return bool(ok.all()), q


def keep(keys, has, qc, keep_cells):
    """lpd_odom_keep for every key -> [n] bool"""
    keys = np.asarray(keys, dtype=i64)
    if not has:
        return np.ones(len(keys), dtype=bool)
    return (np.abs(M.unkey(keys) - np.asarray(qc, dtype=i64)[None, :]) <= int(keep_cells)).all(axis=1)


def crop(cells, centre, origin, cell, keep_cells):
    """lpd_map_crop on Cells -> (Cells of the kept cells, the number left behind)"""
    has, qc = centre_cell(centre, origin, cell)
    k = keep(cells.keys, has, qc, keep_cells)
    return M.Cells(cells.keys[k], cells.sums[k], cells.counts[k], 0), int((~k).sum())


def row_keys(points, offsets, poses, origin, cell, scan0=0, scan1=None):
    """the keys of the rows that lpd_map_insert gives a cell (one a row, repeated)"""
    w, _, _ = M.rows_of(points, offsets, poses, origin, scan0, scan1)
    return M.keyed(w, M.inv_cell(cell))[0]


def touched(keys, rkeys, reach):
    """lpd_map_touch on a map with the ascending `keys`: the cells within `reach` of a row's cell -> [len(keys)] bool"""
    keys = np.asarray(keys, dtype=i64)
    mark = np.zeros(len(keys), dtype=bool)
    q = M.unkey(np.unique(np.asarray(rkeys, dtype=i64)))
    for d in L.offsets_of(reach):
        j = L.lookup(keys, *L.neighbour(q, d))
        mark[j[j >= 0]] = True
    return mark


def empty_cells():
    return M.Cells(np.zeros(0, dtype=i64), np.zeros((0, 3), dtype=i64), np.zeros(0, dtype=i64), 0)


def estimate(points, lengths, start=None, cell=1.0, keep_m=60.0, refresh=10, iters=8, dmax=None, min_inliers=50, max_flat=0.3, reach=1,
             min_cells=5, min_share=0.19, max_jump=5.0, first_motion=None, on_map=None):
    """odometry.estimate_poses -> dict(poses [S, 12], pred [S, 12], valid [S] bool, info [S, 4] int32, inliers [S], cells = the final
    Cells, left = the cells every crop left behind).  on_map(t, cells): called with the map after scan t's insert (and crop)."""
    pts = np.asarray(points, dtype=f32)
    lengths = np.asarray(lengths, dtype=i64)
    S = len(lengths)
    off = M.offsets_of(lengths)
    P = np.zeros((S, 12), dtype=f64)
    P[0] = IDENTITY if start is None else np.asarray(start, dtype=f64).reshape(12)
    origin = P[0, M.TRA].copy()
    pred, insert_pose = np.zeros((S, 12), dtype=f64), np.zeros((S, 12), dtype=f64)
    info = np.zeros((S, 4), dtype=np.int32)
    state = np.zeros(S, dtype=np.int32)
    dm = L.schedule(cell, iters) if dmax is None else tuple(dmax)
    keep_cells, sq = int(math.ceil(keep_m / cell)), share_q(min_share)
    cells, surf, left = empty_cells(), None, []
    for t in range(S):
        P[t] = pred[t] = predict(P, t, first_motion)
        if t > 0 and len(cells.keys) == 0:      # an empty map: no correspondence, every step of a valid scan refused
            ok = bool(L.scan_valid(P[t:t + 1], off[t:t + 2], len(pts), 0, 1)[0])
            info[t] = (1, 0, len(dm) - 1, 0) if ok else (-1, 0, 0, 0)
        elif t > 0:
            if surf is None:
                surf = L.surface(cells, reach, min_cells)
            r = L.localize(surf, pts, off[t:t + 2], P[t:t + 1], origin, cell, dm, min_inliers, max_flat)
            P[t], info[t] = r["pose"][0], r["info"][0]
        state[t], P[t], insert_pose[t] = accept(pred[t], P[t], info[t], int(lengths[t]), t, sq, max_jump)
        cells = M.insert(pts, off, insert_pose, origin, cell, t, t + 1, into=cells)
        if refresh is not None and (t + 1) % refresh == 0 and t + 1 < S:
            cells, n = crop(cells, P[t], origin, cell, keep_cells)
            left.append(n)
        surf = None
        if on_map is not None:
            on_map(t, cells)
    n_rows = lengths.astype(f64)
    inliers = np.where(n_rows > 0, info[:, 3].astype(f64) / np.maximum(n_rows, 1.0), 0.0)
    return dict(poses=P, pred=pred, valid=state == 1, info=info, inliers=inliers, cells=cells, left=left, insert_pose=insert_pose)
