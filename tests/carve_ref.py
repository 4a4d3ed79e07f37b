"""Numpy restatement of the moving-object stage of the drive map (include/lpd_hip.h, "Moving objects out of the drive map"; arithmetic in
csrc/lpd_carve_math.h), written from the definition: the record of a scan, the integer walk of a ray, which cells are looked up, the
pierce rule, the MOVING predicate, the carved map and the flagged rows.  It works on map_ref.insert's cells and loc_ref's Surface --
sorted keys and a binary search, no hash table, so a count belongs to a key by construction.  fp32 and float64 operations stand where
the header has them, one numpy operation each; the walk is in int64.  Two forms of the walk: walk_one, one ray in Python integers as the
definition words it, and the batched one inside pierce(), which steps all rays of a call together.  Used by tests/test_carve_cpu.py
(against csrc/lpd_carve_math.h compiled for the host) and tests/test_carve_gpu.py (against the kernels, exact equality)."""
import numpy as np

import loc_ref as L
import map_ref as M

f32, f64, i64 = np.float32, np.float64, np.int64
SUB = 512
MAX_SKIP, MAX_STEPS, RATIO_UNITS, MAX_RATIO_Q = 16, 8192, 1024, 1 << 20


class Params:
    """the host parameters of lpd_map_pierce (clearance and radius in METRES) and the rule of lpd_map_carve; no defaults here:
    carve_cases.params makes one from mapping.Carve's"""

    def __init__(self, skip_end, skip_start, max_steps, max_flat, clearance, radius, min_pierce, ratio_q):
        self.skip_end, self.skip_start, self.max_steps, self.max_flat = int(skip_end), int(skip_start), int(max_steps), f32(max_flat)
        self.clearance, self.radius, self.min_pierce, self.ratio_q = float(clearance), float(radius), int(min_pierce), int(ratio_q)


def ratio_q(ratio):
    return int(round(float(ratio) * RATIO_UNITS))


# ---- one scan ------------------------------------------------------------------------------------------------------------------------------
def scans(poses, origin, inv):
    """-> (Mm [S, 3, 3] fp32, u [S, 3] fp32 = the sensor, e [S, 3] fp32 = u * inv_cell, ok [S]: the pose is finite and u has a cell)"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    Mm, u = M.rel(P, origin)
    with np.errstate(all="ignore"):
        e = (u * f32(inv)).astype(f32)
    _, has = M.index(u, inv)
    return Mm, u, e, np.isfinite(P).all(axis=1) & has.all(axis=1)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------
def sub(f):
    """a coordinate in cells (fp32) -> units of 1/512 cell, always odd"""
    return 2 * np.floor(np.asarray(f, dtype=f32).astype(f64) * 256.0).astype(i64) + 1


def ray_of(f, e):
    """f, e [n, 3] fp32 (the endpoint and the sensor in cells) -> dict of int64 arrays: D = |A - B|, s, N, qa, qb, n"""
    A, B = sub(f), sub(e)
    qa, qb = A >> 9, B >> 9
    D = A - B
    s = np.sign(D)
    W = SUB * (qb + (s > 0))
    return dict(D=np.abs(D), s=s, N=np.abs(W - B), qa=qa, qb=qb, n=np.abs(qa - qb).sum(axis=1))


def visits(n, max_steps):
    return np.clip(np.asarray(n, dtype=i64) - 1, 0, max_steps)


def best_axis(N, D):
    """[n, 3] int64 each -> the axis of the next step: the smallest N_c / D_c by cross-multiplication, ties to the lowest axis, an axis
    with D_c == 0 never (-1 when all are)"""
    b = np.full(len(N), -1, dtype=i64)
    rows = np.arange(len(N))
    for c in range(3):
        bb = np.maximum(b, 0)
        take = (D[:, c] != 0) & ((b < 0) | (N[:, c] * D[rows, bb] < N[rows, bb] * D[:, c]))
        b = np.where(take, c, b)
    return b


def walk_one(f, e, max_steps=MAX_STEPS):
    """ONE ray in Python integers, as the definition words it -> (the cells stepped into [(x, y, z)], n, cut)"""
    A = [2 * int(np.floor(float(f32(v)) * 256.0)) + 1 for v in f]
    B = [2 * int(np.floor(float(f32(v)) * 256.0)) + 1 for v in e]
    qa, q = [a >> 9 for a in A], [b >> 9 for b in B]
    D = [a - b for a, b in zip(A, B)]
    s = [(d > 0) - (d < 0) for d in D]
    N = [abs(SUB * (q[c] + (s[c] > 0)) - B[c]) for c in range(3)]
    D = [abs(d) for d in D]
    n = sum(abs(a - b) for a, b in zip(qa, q))
    out = []
    for _ in range(min(max(n - 1, 0), max_steps)):
        b = -1
        for c in range(3):
            if D[c] != 0 and (b < 0 or N[c] * D[b] < N[b] * D[c]):
                b = c
        q[b] += s[b]
        N[b] += SUB
        out.append(tuple(q))
    return out, n, n - 1 > max_steps


def cheb(a, b):
    return np.abs(np.asarray(a, dtype=i64) - np.asarray(b, dtype=i64)).max(axis=-1)


def looked(q, qa, qb, skip_end, skip_start):
    return (cheb(q, qa) >= skip_end) & (cheb(q, qb) >= skip_start)


# ---- the pierce rule -----------------------------------------------------------------------------------------------------------------------
def reliable(n, flat, max_flat):
    n = np.asarray(n, dtype=f32)
    with np.errstate(all="ignore"):
        return ~((n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)) & (np.asarray(flat, dtype=f32) <= f32(max_flat))


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def off(n, a, b):
    """n . (a - b) in float64 on fp32 values"""
    return _dot(np.asarray(n, dtype=f32).astype(f64), np.asarray(a, dtype=f32).astype(f64) - np.asarray(b, dtype=f32).astype(f64))


def pierced(o, w, c, n, flat, has_e, ne, flate, prm):
    """rays o -> w [k, 3] fp32 at found cells (c, n [k, 3], flat [k]); the endpoint's own row (ne, flate) where has_e -> [k] bool"""
    with np.errstate(all="ignore"):
        part1 = ~(has_e & reliable(ne, flate, prm.max_flat)) | (np.abs(off(ne, c, w)) > prm.clearance)
        g, h = off(n, o, c), off(n, w, c)
        plane = ((g > prm.clearance) & (h < -prm.clearance)) | ((g < -prm.clearance) & (h > prm.clearance))
        o64, w64, c64 = (np.asarray(v, dtype=f32).astype(f64) for v in (o, w, c))
        v, a = w64 - o64, c64 - o64
        aa, vv, av = _dot(a, a), _dot(v, v), _dot(a, v)
        near = ((aa * vv) - (av * av)) < ((prm.radius * prm.radius) * vv)
        return part1 & np.where(reliable(n, flat, prm.max_flat), plane, near)


# ---- lpd_map_pierce ------------------------------------------------------------------------------------------------------------------------
def pierce(surf, points, offsets, poses, origin, cell, prm, scan0=0, scan1=None, counts=None, info=None, plane_test=True):
    """surf: loc_ref.Surface of the map -> (counts [M] int64 per key in surf.keys' order, info [6] int64); a given counts / info is added
    to.  plane_test=False is the NAIVE rule the quality tests are held against: every found cell that is looked up counts."""
    pts = np.asarray(points, dtype=f32)
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    scan1 = len(P) if scan1 is None else scan1
    counts = np.zeros(len(surf.keys), dtype=i64) if counts is None else counts
    info = np.zeros(6, dtype=i64) if info is None else info
    got = M.row_scans(offsets, scan0, scan1, pts.shape[0])
    if got is None:
        return counts, info
    g, scan, not_read = got
    inv = M.inv_cell(cell)
    Mm, u, e, ok_scan = scans(P, origin, inv)
    w = M.world(Mm[scan], u[scan], pts[g, :3])
    _, has = M.index(w, inv)
    live = has.all(axis=1) & ok_scan[scan]
    info[1] += not_read + int((~live).sum())
    w, o, scan = w[live], u[scan][live], scan[live]
    with np.errstate(all="ignore"):
        f = (w * f32(inv)).astype(f32)
    r = ray_of(f, e[scan])
    vis = visits(r["n"], prm.max_steps)
    info[0] += len(w)
    info[2] += int((r["n"] - 1 > prm.max_steps).sum())
    info[3] += int(vis.sum())
    at_e = L.lookup(surf.keys, M.key(r["qa"]))
    q, N = r["qb"].copy(), r["N"].copy()
    act = np.flatnonzero(vis > 0)
    step = 0
    while len(act):
        b = best_axis(N[act], r["D"][act])
        q[act, b] += r["s"][act, b]
        N[act, b] += SUB
        see = act[looked(q[act], r["qa"][act], r["qb"][act], prm.skip_end, prm.skip_start)]
        j = L.lookup(surf.keys, M.key(q[see]))
        see, j = see[j >= 0], j[j >= 0]
        info[4] += len(see)
        if len(see):
            if plane_test:
                ae = at_e[see]
                hit = pierced(o[see], w[see], surf.points[j], surf.normals[j], surf.flatness[j], ae >= 0, surf.normals[np.maximum(ae, 0)],
                              surf.flatness[np.maximum(ae, 0)], prm)
            else:
                hit = np.ones(len(see), dtype=bool)
            np.add.at(counts, j[hit], 1)
            info[5] += int(hit.sum())
        step += 1
        act = act[vis[act] > step]
    return counts, info


# ---- lpd_map_carve / lpd_scan_moving ---------------------------------------------------------------------------------------------------------
def moving_exact(m, p, min_pierce, ratio_q):
    """the definition in Python integers"""
    return int(m) > 0 and int(p) >= int(min_pierce) and int(p) * RATIO_UNITS >= int(ratio_q) * int(m)


def moving(m, p, min_pierce, ratio_q):
    """arrays; the header's order: p * 1024 < 2^41, so an m >= 2^42 fails for every ratio_q >= 1 before the product is made"""
    m, p = np.asarray(m, dtype=i64), np.asarray(p, dtype=i64)
    base = (m > 0) & (p >= min_pierce)
    if ratio_q == 0:
        return base
    small = m < (1 << 42)
    return base & small & (p * RATIO_UNITS >= ratio_q * np.where(small, m, 0))


def carve(cells, counts, prm):
    """map_ref.Cells and their pierce counts -> (the Cells that stay, info5 = rows, 0, 0, cells created, cells left behind)"""
    mv = moving(cells.counts, counts, prm.min_pierce, prm.ratio_q)
    keep = ~mv
    out = M.Cells(cells.keys[keep], cells.sums[keep], cells.counts[keep], int(cells.info[1]))
    return out, np.array([int(cells.counts[keep].sum()), 0, 0, int(keep.sum()), int(mv.sum())], dtype=i64)


def scan_moving(cells, counts, points, offsets, poses, origin, cell, prm, scan0=0, scan1=None, flags=None):
    """-> (flags [rows] uint8: written for the rows of the call only; info [2] = rows flagged, rows not flagged)"""
    pts = np.asarray(points, dtype=f32)
    P = np.asarray(poses, dtype=f64).reshape(-1, 12)
    scan1 = len(P) if scan1 is None else scan1
    flags = np.zeros(pts.shape[0], dtype=np.uint8) if flags is None else flags
    off_ = np.asarray(offsets, dtype=i64)
    lo, hi = int(off_[scan0]), int(off_[scan1])
    if not 0 <= lo <= hi <= pts.shape[0]:
        return flags, np.zeros(2, dtype=i64)
    flags[lo:hi] = 0
    g, scan, _ = M.row_scans(offsets, scan0, scan1, pts.shape[0])
    Mm, u = M.rel(P, origin)
    w = M.world(Mm[scan], u[scan], pts[g, :3])
    q, has = M.index(w, M.inv_cell(cell))
    has = has.all(axis=1)
    j = L.lookup(cells.keys, M.key(np.where(has[:, None], q, 0)), has)
    mv = moving(cells.counts, counts, prm.min_pierce, prm.ratio_q)
    f = (j >= 0) & mv[np.maximum(j, 0)] if len(mv) else np.zeros(len(j), dtype=bool)
    flags[g] = f.astype(np.uint8)
    n = int(f.sum())
    return flags, np.array([n, (hi - lo) - n], dtype=i64)
