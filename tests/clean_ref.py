"""numpy restatement of lpd_road_planes / lpd_clean_count / lpd_clean_fill (definitions: include/lpd_hip.h and
csrc/lpd_clean_math.h), shared by tests/test_clean_cpu.py and tests/test_clean_gpu.py: float32 / int64 / float64 operations exactly
as stated, one rounding each; Philox from tests/tuples_ref.py.  And seeded scenes with labels (road / wall / clutter), flat or tilted.
"""
import functools

import numpy as np

import tuples_ref as T

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
CHUNK, MAX_H, MAX_POINTS, QSCALE, QMAX = 1024, 1024, 1 << 20, f32(1024.0), f32(1048576.0)
DEFAULTS = dict(r_min=0.0, r_max=512.0, z_lo=-np.inf, z_hi=np.inf, seed_z_lo=-np.inf, seed_z_hi=np.inf, H=256, tau=0.15, min_det=4.0,
                max_slope=0.27, min_inliers=16, refine=1, clearance=0.3, seed=0)
FLOATS = ("r_min", "r_max", "z_lo", "z_hi", "seed_z_lo", "seed_z_hi", "tau", "min_det", "max_slope", "clearance")


def params(**kw):
    """the parameter block with the floats rounded to fp32, as the C struct holds them"""
    assert set(kw) <= set(DEFAULTS), set(kw) - set(DEFAULTS)
    p = dict(DEFAULTS, **kw)
    for k in FLOATS:
        p[k] = f32(p[k])
    return p


def sq(r):
    return f32(f32(r) * f32(r))


def finite(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v) <= FLT_MAX


def live(x, y, z, rmin2, rmax2, z_lo, z_hi):
    x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
    with np.errstate(all="ignore"):
        d = (x * x) + (y * y)
        assert d.dtype == np.float32
        return finite(x) & finite(y) & finite(z) & (d >= rmin2) & (d <= rmax2) & (z >= z_lo) & (z <= z_hi)


def live_rows(p, P):
    return live(p[:, 0], p[:, 1], p[:, 2], sq(P["r_min"]), sq(P["r_max"]), P["z_lo"], P["z_hi"])


def row_number(r, n):
    """((uint64) r * n) >> 32 on arrays of 32-bit draws"""
    return ((np.asarray(r, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def draw(h, b, n, seed):
    """rows [len(h), 3] of the hypotheses h of scan b"""
    r = T.philox(np.asarray(h, dtype=np.uint64), b, 0, 0, seed & T.M32, (seed >> 32) & T.M32)
    return np.stack([row_number(r[j], n) for j in range(3)], axis=-1)


def slope_ok(a, b, slope2):
    with np.errstate(all="ignore"):
        return ((a * a) + (b * b)) <= slope2


def triple(p0, p1, p2, ok, min_det, slope2):
    """planes through p0, p1, p2 ([..., 3] float32 each) -> (a, b, c, valid)"""
    p0, p1, p2 = (np.asarray(v, dtype=np.float32) for v in (p0, p1, p2))
    with np.errstate(all="ignore"):
        ux, uy, uz = p1[..., 0] - p0[..., 0], p1[..., 1] - p0[..., 1], p1[..., 2] - p0[..., 2]
        vx, vy, vz = p2[..., 0] - p0[..., 0], p2[..., 1] - p0[..., 1], p2[..., 2] - p0[..., 2]
        det = (ux * vy) - (uy * vx)
        a = ((uz * vy) - (vz * uy)) / det
        b = ((ux * vz) - (vx * uz)) / det
        c = p0[..., 2] - ((a * p0[..., 0]) + (b * p0[..., 1]))
        assert a.dtype == b.dtype == c.dtype == np.float32
        valid = np.asarray(ok, dtype=bool) & (np.abs(det) >= f32(min_det)) & slope_ok(a, b, slope2) & finite(c)
    return a, b, c, valid


def residual(x, y, z, a, b, c):
    a, b, c = f32(a), f32(b), f32(c)
    with np.errstate(all="ignore"):
        e = z - (((a * x) + (b * y)) + c)
    assert np.asarray(e).dtype == np.float32
    return e


def inlier(e, tau):
    with np.errstate(invalid="ignore"):
        return np.abs(e) <= f32(tau)


def removed(e, clearance):
    with np.errstate(invalid="ignore"):
        return e <= f32(clearance)


def quant(x, o):
    with np.errstate(all="ignore"):
        q = np.rint((np.asarray(x, dtype=np.float32) - f32(o)) * QSCALE)
        assert q.dtype == np.float32
        return np.minimum(np.maximum(q, -QMAX), QMAX).astype(np.int64)


def sums(X, Y, Z):
    """the nine integer sums as Python integers"""
    X, Y, Z = (v.astype(object) for v in (X, Y, Z))
    return [len(X), int(X.sum()), int(Y.sum()), int(Z.sum()), int((X * X).sum()), int((X * Y).sum()), int((Y * Y).sum()), int((X * Z).sum()),
            int((Y * Z).sum())]


def solve(S, ox, oy, oz, slope2):
    """lpd_clean_solve: Python floats are IEEE float64, one rounding per operation, the header's order -> (a, b, c) fp32 or None"""
    if S[0] < 3:
        return None
    m, sx, sy, sz, sxx, sxy, syy, sxz, syz = (float(v) for v in S)
    cxx = sxx - ((sx * sx) / m)
    cxy = sxy - ((sx * sy) / m)
    cyy = syy - ((sy * sy) / m)
    cxz = sxz - ((sx * sz) / m)
    cyz = syz - ((sy * sz) / m)
    D = (cxx * cyy) - (cxy * cxy)
    if not (D > 0.0 and D <= np.finfo(np.float64).max):
        return None
    a = ((cxz * cyy) - (cyz * cxy)) / D
    b = ((cyz * cxx) - (cxz * cxy)) / D
    cq = ((sz - (a * sx)) - (b * sy)) / m
    c = ((float(oz) + (cq / 1024.0)) - (a * float(ox))) - (b * float(oy))
    with np.errstate(all="ignore"):
        af, bf, cf = f32(a), f32(b), f32(c)
    if not (bool(slope_ok(af, bf, slope2)) and bool(finite(cf))):
        return None
    return af, bf, cf


def hypotheses(p, b, P, lv=None):
    """-> (a, b, c, valid, rows) arrays over h = 0 .. H-1 for scan b"""
    n, H = p.shape[0], P["H"]
    lv = live_rows(p, P) if lv is None else lv
    rows = draw(np.arange(H), b, n, P["seed"]).reshape(H, 3)
    with np.errstate(invalid="ignore"):
        band = (p[:, 2] >= P["seed_z_lo"]) & (p[:, 2] <= P["seed_z_hi"])
    ok = (lv & band)[rows].all(axis=1)
    q = p[:, :3]
    a, bb, c, valid = triple(q[rows[:, 0]], q[rows[:, 1]], q[rows[:, 2]], ok, P["min_det"], sq(P["max_slope"]))
    return a, bb, c, valid, rows


def road_plane(p, b, P):
    """one scan [n, >=3] float32 -> (plane (a, b, c, 0) float32, info (n_live, h* or -1, S, inliers of the final plane), live)"""
    p = np.asarray(p, dtype=np.float32)
    lv = live_rows(p, P)
    n_live = int(lv.sum())
    none = np.zeros(4, dtype=np.float32)
    if P["H"] == 0:
        return none, [n_live, -1, 0, 0], lv
    x, y, z = p[lv, 0], p[lv, 1], p[lv, 2]
    a, bb, c, valid, rows = hypotheses(p, b, P, lv)
    best_S, best_h = -1, -1
    for h in np.flatnonzero(valid):
        S = int(inlier(residual(x, y, z, a[h], bb[h], c[h]), P["tau"]).sum())
        if S > best_S:      # ascending h: a tie keeps the lower one
            best_S, best_h = S, int(h)
    if best_h < 0:
        return none, [n_live, -1, 0, 0], lv
    if best_S < P["min_inliers"]:
        return none, [n_live, -1, best_S, 0], lv
    pa, pb, pc = a[best_h], bb[best_h], c[best_h]
    final = best_S
    if P["refine"]:
        o = p[rows[best_h, 0], :3]
        inl = inlier(residual(x, y, z, pa, pb, pc), P["tau"])
        S9 = sums(quant(x[inl], o[0]), quant(y[inl], o[1]), quant(z[inl], o[2]))
        got = solve(S9, o[0], o[1], o[2], sq(P["max_slope"]))
        if got is not None:
            pa, pb, pc = got
            final = int(inlier(residual(x, y, z, pa, pb, pc), P["tau"]).sum())
    return np.array([pa, pb, pc, 0.0], dtype=np.float32), [n_live, best_h, best_S, final], lv


def keep_mask(p, plane, info, lv, P):
    """5. which rows of the scan are kept, for a given plane"""
    if info[1] < 0:
        return lv.copy()
    e = residual(p[:, 0], p[:, 1], p[:, 2], plane[0], plane[1], plane[2])
    return lv & ~removed(e, P["clearance"])


def clean_batch(points, offsets, P, max_len=None):
    """The three entry points on a ragged batch: points [rows, >=3] float32, offsets [B+1] (any integers)
    -> dict(out [total, 3], out_offsets [B+1] int32, plane [B, 4], info [B, 4] int32, mask [rows] uint8)"""
    points = np.asarray(points, dtype=np.float32)
    rows, B = points.shape[0], len(offsets) - 1
    max_len = MAX_POINTS if max_len is None else max_len
    plane, info = np.zeros((B, 4), dtype=np.float32), np.zeros((B, 4), dtype=np.int32)
    mask, kept, out_off = np.zeros(rows, dtype=np.uint8), [], [0]
    for b in range(B):
        a, e = int(offsets[b]), int(offsets[b + 1])
        if a < 0 or e - a < 1 or e - a > max_len or e > rows:
            info[b] = (-1, -1, 0, 0)
            out_off.append(out_off[-1])
            continue
        p = points[a:e]
        plane[b], info[b], lv = road_plane(p, b, P)
        k = keep_mask(p, plane[b], info[b], lv, P)
        mask[a:e] = k
        kept.append(p[k, :3])
        out_off.append(out_off[-1] + int(k.sum()))
    out = np.concatenate(kept, 0) if kept else np.zeros((0, 3), dtype=np.float32)
    return dict(out=np.ascontiguousarray(out), out_offsets=np.array(out_off, dtype=np.int32), plane=plane, info=info, mask=mask)


# ---- scenes with labels: 0 road, 1 wall, 2 clutter (the layout of tests/submap_ref.py's scan: a road disc to 50 m, a wall, 24 blobs)
ROAD_Z = -1.7


@functools.lru_cache(maxsize=None)
def _scene(n, seed, ta, tb):
    rng = np.random.default_rng(seed)
    ng, nw = n // 2, n // 4
    nc = n - ng - nw
    r, ang = 50.0 * np.sqrt(rng.random(ng)), 2 * np.pi * rng.random(ng)
    ground = np.stack((r * np.cos(ang), r * np.sin(ang), ROAD_Z + 0.03 * rng.standard_normal(ng)), axis=1)
    wall = np.stack((-40 + 80 * rng.random(nw), 12.0 + 0.05 * rng.standard_normal(nw), ROAD_Z + 8 * rng.random(nw)), axis=1)
    centres = rng.uniform((-45, -45, -1.5), (45, 45, 2.0), size=(24, 3))
    clutter = centres[rng.integers(0, 24, nc)] + rng.standard_normal((nc, 3)) * (0.8, 0.8, 0.5)
    pts = np.concatenate((ground, wall, clutter), 0)
    pts[:, 2] += ta * pts[:, 0] + tb * pts[:, 1]      # the whole scene stands on the tilted road
    label = np.concatenate((np.zeros(ng, np.int8), np.ones(nw, np.int8), np.full(nc, 2, np.int8)))
    order = rng.permutation(n)
    pts = np.ascontiguousarray(pts[order], dtype=np.float32)
    label = label[order]
    pts.setflags(write=False)
    label.setflags(write=False)
    return pts, label


def scene(n, seed=0, tilt=(0.0, 0.0)):
    """-> (points [n, 3] float32, labels [n] int8); the road is z = tilt[0] x + tilt[1] y + ROAD_Z (+ 3 cm of noise).  Read-only."""
    return _scene(int(n), int(seed), float(tilt[0]), float(tilt[1]))


def height_above_road(p, tilt=(0.0, 0.0)):
    return p[:, 2].astype(np.float64) - (tilt[0] * p[:, 0].astype(np.float64) + tilt[1] * p[:, 1].astype(np.float64) + ROAD_Z)
