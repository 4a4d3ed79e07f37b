"""Numpy restatement of localisation against the drive map (include/lpd_hip.h, "Localisation against the drive map"; arithmetic in
csrc/lpd_loc_math.h), written from the definition: the lookup of a cell, the surf row of a cell (centroid, normal, flatness, cells used)
and the trimmed point-to-plane ICP of posed scans against those rows.  It works on map_ref.insert's cells -- sorted keys and a binary
search, no hash table, so slot independence is built in.  fp32 and float64 operations stand where the header has them, one numpy
operation each; sums are int64; the step is icp_ref's Python-float LDL^T and update.  Used by tests/test_localize_cpu.py (against
csrc/lpd_loc_math.h compiled for the host) and tests/test_localize_gpu.py (against the kernels, exact equality)."""
import numpy as np

import icp_ref as I
import map_ref as M

f32, f64, i64 = np.float32, np.float64, np.int64
QLIM = M.QLIM
MAX_SCAN_ROWS = 1 << 20
RANGE = f32(512.0)
OFFSETS27 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]      # ascending key


def offsets_of(reach):
    r = range(-reach, reach + 1)
    return [(dx, dy, dz) for dz in r for dy in r for dx in r]


def neighbour(q, d):
    """q [n, 3] int64, d = (dx, dy, dz) -> (key [n] int64, inside [n]): a cell with an index outside [-2^20, 2^20) is absent"""
    nq = np.asarray(q, dtype=i64) + np.asarray(d, dtype=i64)[None, :]
    inside = ((nq >= -QLIM) & (nq < QLIM)).all(axis=1)
    return M.key(np.where(inside[:, None], nq, 0)), inside


def lookup(keys, k, inside=None):
    """keys [M] ascending, k [n] -> the index of every k in keys, -1 for an absent one"""
    k = np.asarray(k, dtype=i64)
    if len(keys) == 0:
        return np.full(k.shape, -1, dtype=i64)
    j = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
    hit = keys[j] == k
    if inside is not None:
        hit &= inside
    return np.where(hit, j, -1).astype(i64)


class Surface:
    """keys [M] int64 ascending, points [M, 3] fp32, normals [M, 3] fp32, flatness [M] fp32, used [M] int64"""

    def __init__(self, keys, points, normals, flatness, used):
        self.keys, self.points, self.normals, self.flatness, self.used = keys, points, normals, flatness, used

    def rows(self):
        """[M, 8] fp32 = the surf rows in key order"""
        return np.concatenate((self.points, self.normals, self.flatness[:, None], self.used.astype(f32)[:, None]), axis=1).astype(f32)


def surface_of(keys, points, reach=1, min_cells=5):
    """lpd_map_surface on cells given by their ascending keys and centroids (every count positive)"""
    keys, c = np.asarray(keys, dtype=i64), np.asarray(points, dtype=f32)
    n = len(keys)
    q = M.unkey(keys)
    s = {name: np.zeros(n, dtype=f32) for name in ("sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz")}
    k = np.zeros(n, dtype=i64)
    with np.errstate(all="ignore"):
        for d in offsets_of(reach):
            j = lookup(keys, *neighbour(q, d))
            pres = j >= 0
            e = c[np.maximum(j, 0)] - c
            dx, dy, dz = e[:, 0], e[:, 1], e[:, 2]
            for name, v in (("sx", dx), ("sy", dy), ("sz", dz), ("sxx", dx * dx), ("sxy", dx * dy), ("sxz", dx * dz), ("syy", dy * dy),
                            ("syz", dy * dz), ("szz", dz * dz)):
                s[name] = np.where(pres, s[name] + v, s[name])
            k += pres
        nrm, flat = I.normal_from_moments(s, np.maximum(k, 1))
    few = k < min_cells
    nrm = np.where(few[:, None], f32(0.0), nrm).astype(f32)
    flat = np.where(few, f32(0.0), flat).astype(f32)
    return Surface(keys, c, nrm, flat, k)


def surface(cells, reach=1, min_cells=5):
    """map_ref.Cells -> Surface"""
    return surface_of(cells.keys, cells.points, reach, min_cells)


# ---- one scan ------------------------------------------------------------------------------------------------------------------------------
def scan_valid(poses, offsets, rows, scan0, scan1):
    """[S] bool: False outside scan0 .. scan1-1"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    off = np.asarray(offsets, dtype=i64)
    v = np.zeros(len(P), dtype=bool)
    o0, o1 = off[scan0:scan1], off[scan0 + 1:scan1 + 1]
    v[scan0:scan1] = np.isfinite(P[scan0:scan1]).all(axis=1) & (o0 >= 0) & (o0 <= o1) & (o1 <= rows) & (o1 - o0 <= MAX_SCAN_ROWS)
    return v


def centre(poses, origin):
    """-> (g [S, 3] float64 = t - origin, g32 its fp32 rounding)"""
    with np.errstate(all="ignore"):
        g = np.asarray(poses, dtype=f64).reshape(-1, 12)[:, M.TRA] - np.asarray(origin, dtype=f64)[None, :]
        return g, g.astype(f32)


def centred(w, g32):
    """p = w - g32 -> (p fp32, ok: every |p_c| <= 512)"""
    with np.errstate(all="ignore"):
        p = (np.asarray(w, dtype=f32) - np.asarray(g32, dtype=f32)).astype(f32)
        return p, (np.abs(p) <= RANGE).all(axis=1)


def d2(c, w):
    with np.errstate(all="ignore"):
        dx, dy, dz = c[:, 0] - w[:, 0], c[:, 1] - w[:, 1], c[:, 2] - w[:, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def nearest(surf, q, w, live):
    """the nearest centroid among the 27 cells around q, in ascending key order, strictly nearer wins -> (index into surf or -1, d2)"""
    n = len(w)
    best = np.full(n, np.inf, dtype=f32)
    at = np.full(n, -1, dtype=i64)
    for d in OFFSETS27:
        k, inside = neighbour(q, d)
        j = lookup(surf.keys, k, inside & live)
        pres = j >= 0
        dd = d2(surf.points[np.maximum(j, 0)], w)
        with np.errstate(all="ignore"):
            win = pres & (dd < best)
        best = np.where(win, dd, best).astype(f32)
        at = np.where(win, j, at)
    return at, best


def accept(surf, at, best, dmax, max_flat):
    a = np.maximum(at, 0)
    n = surf.normals[a]
    with np.errstate(all="ignore"):
        return (at >= 0) & I.within(best, dmax) & ~((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == 0)) & (surf.flatness[a] <= f32(max_flat))


def terms(p, c, n, g32):
    """the 32 terms of every correspondence [m, 32] int64: q = c - g32, then lpd_icp_row and lpd_icp_terms"""
    with np.errstate(all="ignore"):
        q = (c - g32).astype(f32)
    Ji, ri = I.rows(p, q, n)
    T = np.zeros((len(ri), I.SUMS), dtype=i64)
    T[:, I.SUM_M] = 1
    e = I.SUM_H
    for a in range(6):
        for b in range(a, 6):
            T[:, e] = Ji[:, a] * Ji[:, b]
            e += 1
    for a in range(6):
        T[:, I.SUM_G + a] = Ji[:, a] * ri
    T[:, I.SUM_RR] = ri * ri
    return T


def step(sums, min_inliers, pose, origin, g):
    """lpd_loc_step -> (applied, pose [12] float64): a refused step returns the pose's own values"""
    pose = [float(v) for v in np.asarray(pose, dtype=f64).reshape(12)]
    origin, g = [float(v) for v in origin], [float(v) for v in g]
    same = np.array(pose)
    with np.errstate(all="ignore"):
        if int(sums[I.SUM_M]) < int(min_inliers):
            return False, same
        try:
            x = I.ldl(sums)
            if x is None or not all(I._finite(v) for v in x):
                return False, same
            moved = list(pose)
            for c in range(3):
                moved[4 * c + 3] = (pose[4 * c + 3] - origin[c]) - g[c]
            new = I.update(x, moved)
            for c in range(3):
                new[4 * c + 3] = (new[4 * c + 3] + g[c]) + origin[c]
        except (OverflowError, ZeroDivisionError):      # Python raises where IEEE gives inf or NaN: a refusal either way
            return False, same
        if not all(I._finite(v) for v in new):
            return False, same
    return True, np.array(new)


def one_pass(surf, pts, grow, gscan, poses, origin, g32, inv, dmax, max_flat, S):
    """-> (sums [S, 32] int64, has [n], at [n]) over the rows grow of the scans gscan at `poses`"""
    Mx, u = M.rel(poses, origin)
    w = M.world(Mx[gscan], u[gscan], pts[grow, :3])
    q, ok = M.index(w, inv)
    p, near = centred(w, g32[gscan])
    live = ok.all(axis=1) & near
    at, best = nearest(surf, q, w, live)
    has = live & accept(surf, at, best, dmax, max_flat)
    T = terms(p[has], surf.points[at[has]], surf.normals[at[has]], g32[gscan[has]])
    sums = np.zeros((S, I.SUMS), dtype=i64)
    np.add.at(sums, gscan[has], T)
    return sums, has, at


def localize(surf, points, offsets, poses, origin, cell, dmax, min_inliers=50, max_flat=0.3, scan0=0, scan1=None):
    """lpd_map_localize -> dict(pose [S, 12] float64, info [S, 4] int32, sums [iters + 1, S, 32] int64, cell [rows] int64)"""
    pts = np.asarray(points, dtype=f32)
    P = np.array(poses, dtype=f64).reshape(-1, 12)
    S, rows, iters = len(P), len(pts), len(dmax) - 1
    scan1 = S if scan1 is None else scan1
    origin = np.asarray(origin, dtype=f64)
    inv = M.inv_cell(cell)
    info = np.zeros((S, 4), dtype=np.int32)
    sums = np.zeros((iters + 1, S, I.SUMS), dtype=i64)
    cells = np.full(rows, -1, dtype=i64)
    valid = scan_valid(P, offsets, rows, scan0, scan1)
    info[scan0:scan1, 0] = np.where(valid[scan0:scan1], 1, -1)
    g, g32 = centre(P, origin)
    got = M.row_scans(offsets, scan0, scan1, rows)
    if got is None:
        grow = gscan = np.zeros(0, dtype=i64)
    else:
        keep = valid[got[1]]
        grow, gscan = got[0][keep], got[1][keep]
    for s in range(iters + 1):
        sums[s], has, at = one_pass(surf, pts, grow, gscan, P, origin, g32, inv, f32(dmax[s]), max_flat, S)
        if s == iters:
            cells[grow] = np.where(has, surf.keys[np.maximum(at, 0)] if len(surf.keys) else -1, -1)
            break
        for i in np.flatnonzero(valid):
            ok, P[i] = step(sums[s, i], min_inliers, P[i], origin, g[i])
            info[i, 1 if ok else 2] += 1
    info[valid, 3] = sums[iters, valid, I.SUM_M]
    return dict(pose=P, info=info, sums=sums, cell=cells)


def schedule(cell, iters=8):
    """LocalizeSearch's default distances: min(cell, 16) for the first iters // 2 + 1 passes, half of that afterwards"""
    wide = min(float(cell), 16.0)
    n_wide = min(iters // 2 + 1, iters + 1)
    return (wide,) * n_wide + (0.5 * wide,) * (iters + 1 - n_wide)


def step_float64(surf, pts, pose, origin, cell, dmax, max_flat):
    """The yardstick of one step: the same correspondences, rows formed in float64 from the float64 pose without quantisation, solved
    by numpy -> x [6] (rotation vector, translation) about the scan's centre"""
    P = np.asarray(pose, dtype=f64).reshape(1, 12)
    g, g32 = centre(P, origin)
    n = len(pts)
    _, has, at = one_pass(surf, np.asarray(pts, dtype=f32), np.arange(n), np.zeros(n, dtype=i64), P, origin, g32, M.inv_cell(cell), f32(dmax),
                          max_flat, 1)
    R, t = P[0].reshape(3, 4)[:, :3], P[0].reshape(3, 4)[:, 3]
    p = np.asarray(pts, dtype=f64)[has, :3] @ R.T + (t - np.asarray(origin, dtype=f64)) - g[0]
    q = surf.points[at[has]].astype(f64) - g[0]
    nn = surf.normals[at[has]].astype(f64)
    J = np.concatenate((np.cross(p, nn), nn), axis=1)
    r = np.einsum("ij,ij->i", q - p, nn)
    return np.linalg.solve(J.T @ J, J.T @ r), int(has.sum())
