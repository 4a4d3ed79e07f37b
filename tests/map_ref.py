"""Numpy restatement of the drive map (include/lpd_hip.h, "The drive map"), written from the definition: the corrected pose of every
scan (lpd_drive_correct), the world rows, cells, keys and fixed-point sums of lpd_map_insert, and the extraction of
lpdnet_hip/mapping.py.  Every float64 / fp32 operation is one numpy operation on arrays of that dtype, so each is rounded once and
nothing is contracted; sums are int64.  The `_ext` functions compute the same quantities in extended precision (np.longdouble) from the
same inputs: the yardstick of the fp32 / float64 error.  Used by tests/test_map_cpu.py (against csrc/lpd_map_math.h compiled for the
host) and tests/test_map_gpu.py (against the kernels, exact equality)."""
import numpy as np

import pgo_ref

f32, f64, i64, u64 = np.float32, np.float64, np.int64, np.uint64
QLIM = 1 << 20
UNITS = 65536.0
CHUNK = 1024
MAX_PROBES = 128


def inv_cell(cell):
    """the fp32 1.0f / cell"""
    return f32(1.0) / f32(cell)


# ---- lpd_map_insert ---------------------------------------------------------------------------------------------------------------------
def rel(poses, origin):
    """poses [n, 12] float64, origin [3] float64 -> (M [n, 3, 3] fp32, u [n, 3] fp32): M = R_i, u = t_i - origin in float64, rounded once"""
    P = np.asarray(poses, dtype=f64).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        return P[:, :, :3].astype(f32), (P[:, :, 3] - np.asarray(origin, dtype=f64)[None, :]).astype(f32)


def world(M, u, xyz):
    """rows [n, 3] fp32 by per-row (M [n, 3, 3], u [n, 3]) fp32 -> w [n, 3] fp32: (((M_c0*x) + (M_c1*y)) + (M_c2*z)) + u_c"""
    x, y, z = (np.ascontiguousarray(xyz[:, c], dtype=f32) for c in range(3))
    out = np.empty((len(x), 3), dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            out[:, c] = (((M[:, c, 0] * x) + (M[:, c, 1] * y)) + (M[:, c, 2] * z)) + u[:, c]
    return out


def index(w, inv):
    """w fp32 (any shape) -> (q int64, ok bool): q = (int) floorf(w * inv_cell) where that lies in [-2^20, 2^20)"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(w, dtype=f32) * f32(inv))
        ok = (f >= f32(-QLIM)) & (f < f32(QLIM))
    return np.where(ok, f, f32(0)).astype(i64), ok


def key(q):
    """q [n, 3] int64 -> key [n] int64"""
    q = np.asarray(q, dtype=i64)
    return (q[:, 0] + QLIM) | ((q[:, 1] + QLIM) << 21) | ((q[:, 2] + QLIM) << 42)


def unkey(k):
    k = np.asarray(k, dtype=i64)
    mask = (1 << 21) - 1
    return np.stack(((k & mask) - QLIM, ((k >> 21) & mask) - QLIM, ((k >> 42) & mask) - QLIM), axis=1)


def fixed(w):
    """rint (half to even) of the exact product w * 2^16 -> int64 (finite w)"""
    return np.rint(np.asarray(w, dtype=f32).astype(f64) * UNITS).astype(i64)


def mix(k):
    """the finaliser of splitmix64 on the key's 64 bits -> uint64"""
    x = np.asarray(k, dtype=i64).astype(u64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> u64(30))
        x = x * u64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> u64(27))
        x = x * u64(0x94d049bb133111eb)
        x = x ^ (x >> u64(31))
    return x


def slot(k, capacity):
    return (mix(k) & u64(capacity - 1)).astype(i64)


def probes(capacity):
    return min(int(capacity), MAX_PROBES)


def scan_of(offsets, lo, hi, g):
    """lpd_drive_scan_of, the binary search as it is written (offsets may hold anything): the result lies in [lo, hi - 1]"""
    a, b = lo + 1, hi
    while a < b:
        mid = (a + b) >> 1
        if int(offsets[mid]) > g:
            b = mid
        else:
            a = mid + 1
    return a - 1


def row_scans(offsets, scan0, scan1, rows):
    """-> (g [n] the rows of the call that are read, scan [n] their scans, not_read = the rows of chunks that are not read), or None
    when the call reads nothing (not 0 <= offsets[scan0] <= offsets[scan1] <= rows)"""
    off = np.asarray(offsets, dtype=i64)
    lo, hi = int(off[scan0]), int(off[scan1])
    if not 0 <= lo <= hi <= rows:
        return None
    part = off[scan0:scan1 + 1]
    if np.all(part[1:] >= part[:-1]):      # a table that is one: every chunk is read
        g = np.arange(lo, hi, dtype=i64)
        return g, scan0 + np.searchsorted(part[:-1], g, side="right") - 1, 0
    gs, ss, not_read = [], [], 0
    for c0 in range((lo // CHUNK) * CHUNK, hi, CHUNK):
        g0, g1 = max(c0, lo), min(c0 + CHUNK, hi)
        if g0 >= g1:
            continue
        i_lo, i_hi = scan_of(off, scan0, scan1, g0), scan_of(off, scan0, scan1, g1 - 1)
        sub = off[i_lo:i_hi + 2]
        if not (i_lo <= i_hi and sub[0] <= g0 and g1 - 1 < sub[-1] and np.all(sub[1:] >= sub[:-1])):
            not_read += g1 - g0
            continue
        g = np.arange(g0, g1, dtype=i64)
        gs.append(g)
        ss.append(i_lo + np.searchsorted(sub[:-1], g, side="right") - 1)
    if not gs:
        return np.zeros(0, dtype=i64), np.zeros(0, dtype=i64), not_read
    return np.concatenate(gs), np.concatenate(ss), not_read


class Cells:
    """the map of one or more inserts: keys [M] int64 ascending, sums [M, 3] int64, counts [M] int64, points [M, 3] fp32; info [4] =
    (rows inserted, rows dropped, 0, cells)"""

    def __init__(self, keys, sums, counts, dropped):
        self.keys, self.sums, self.counts = keys, sums, counts
        self.points = extract(sums, counts)
        self.info = np.array([int(counts.sum()), int(dropped), 0, len(keys)], dtype=i64)


def extract(sums, counts):
    """row_c = (float)(((double) S_c / (double) m) * 2^-16)"""
    return ((np.asarray(sums, dtype=i64).astype(f64) / np.asarray(counts, dtype=i64).astype(f64)[:, None]) * (1.0 / UNITS)).astype(f32)


def rows_of(points, offsets, poses, origin, scan0=0, scan1=None):
    """the world rows of the rows that are read -> (w [n, 3] fp32, g [n], not_read)"""
    pts = np.asarray(points, dtype=f32)
    S = np.asarray(poses).reshape(-1, 12).shape[0]
    scan1 = S if scan1 is None else scan1
    got = row_scans(offsets, scan0, scan1, pts.shape[0])
    if got is None:
        return np.zeros((0, 3), dtype=f32), np.zeros(0, dtype=i64), 0
    g, scan, not_read = got
    M, u = rel(np.asarray(poses, dtype=f64).reshape(-1, 12), origin)
    return world(M[scan], u[scan], pts[g, :3]), g, not_read


def keyed(w, inv):
    """world rows -> (key [n'] int64, U [n', 3] int64, dropped) of the rows that get a cell"""
    q, ok = index(w, inv)
    ok = ok.all(axis=1)
    return key(q[ok]), fixed(w[ok]), int((~ok).sum())


def merge(parts):
    """[(key, U, m)] -> (keys ascending, sums, counts): integer sums per key"""
    k = np.concatenate([p[0] for p in parts])
    U = np.concatenate([p[1] for p in parts])
    m = np.concatenate([p[2] for p in parts])
    keys, inv = np.unique(k, return_inverse=True)
    sums = np.zeros((len(keys), 3), dtype=i64)
    counts = np.zeros(len(keys), dtype=i64)
    for c in range(3):
        np.add.at(sums[:, c], inv, U[:, c])
    np.add.at(counts, inv, m)
    return keys, sums, counts


def insert(points, offsets, poses, origin, cell, scan0=0, scan1=None, into=None):
    """lpd_map_insert + the extraction -> Cells; into: the Cells of earlier inserts to add to"""
    w, _, not_read = rows_of(points, offsets, poses, origin, scan0, scan1)
    k, U, dropped = keyed(w, inv_cell(cell))
    parts = [(k, U, np.ones(len(k), dtype=i64))]
    if into is not None:
        parts.append((into.keys, into.sums, into.counts))
        dropped += int(into.info[1])
    keys, sums, counts = merge(parts)
    return Cells(keys, sums, counts, dropped + not_read)


def occupied(points, offsets, poses, origin, cell):
    """the number of occupied cells alone (the quality measure): no sums"""
    w, _, _ = rows_of(points, offsets, poses, origin)
    k, _, _ = keyed(w, inv_cell(cell))
    return int(len(np.unique(k)))


def rows_ext(points, offsets, poses, origin):
    """the world rows in extended precision from the float64 poses and the fp32 points (a table that is one)"""
    ld = np.longdouble
    pts = np.asarray(points, dtype=f32)
    off = np.asarray(offsets, dtype=i64)
    P = np.asarray(poses, dtype=f64).reshape(-1, 3, 4).astype(ld)
    g = np.arange(int(off[0]), int(off[-1]), dtype=i64)
    scan = np.searchsorted(off[:-1], g, side="right") - 1
    u = P[:, :, 3] - np.asarray(origin, dtype=f64).astype(ld)[None, :]
    return np.einsum("nck,nk->nc", P[scan][:, :, :3], pts[g, :3].astype(ld)) + u[scan]


# ---- lpd_drive_correct ------------------------------------------------------------------------------------------------------------------
def bracket(node_scan, i):
    """lpd_map_bracket as it is written, for every i of an array -> a (the last node with node_scan[a] <= i, -1 when there is none)"""
    ns = np.asarray(node_scan, dtype=i64)
    i = np.asarray(i, dtype=i64)
    lo, hi = np.zeros(i.shape, dtype=i64), np.full(i.shape, len(ns), dtype=i64)
    while True:
        act = lo < hi
        if not act.any():
            return lo - 1
        mid = (lo + hi) >> 1
        le = ns[np.minimum(mid, len(ns) - 1)] <= i
        lo = np.where(act & le, mid + 1, lo)
        hi = np.where(act & ~le, mid, hi)


def dot3(a0, a1, a2, b0, b1, b2):
    return ((a0 * b0) + (a1 * b1)) + (a2 * b2)


def between(X, Y):
    """X, Y [n, 12] -> (R [n, 9], t [n, 3]) of X^-1 Y, the difference first; any float dtype"""
    d0, d1, d2 = Y[:, 3] - X[:, 3], Y[:, 7] - X[:, 7], Y[:, 11] - X[:, 11]
    R = np.empty((X.shape[0], 9), dtype=X.dtype)
    t = np.empty((X.shape[0], 3), dtype=X.dtype)
    for r in range(3):
        for c in range(3):
            R[:, 3 * r + c] = dot3(X[:, r], X[:, 4 + r], X[:, 8 + r], Y[:, c], Y[:, 4 + c], Y[:, 8 + c])
        t[:, r] = dot3(X[:, r], X[:, 4 + r], X[:, 8 + r], d0, d1, d2)
    return R, t


def compose(X, R, t):
    """the pose X [n, 12] composed with (R [n, 9], t [n, 3]) -> [n, 12]"""
    out = np.empty_like(X)
    for r in range(3):
        x0, x1, x2 = X[:, 4 * r], X[:, 4 * r + 1], X[:, 4 * r + 2]
        for c in range(3):
            out[:, 4 * r + c] = dot3(x0, x1, x2, R[:, c], R[:, 3 + c], R[:, 6 + c])
        out[:, 4 * r + 3] = dot3(x0, x1, x2, t[:, 0], t[:, 1], t[:, 2]) + X[:, 4 * r + 3]
    return out


def candidate(Pn, Xn, Pi):
    R, t = between(Pn, Pi)
    return compose(Xn, R, t)


def quat_any(R):
    """pgo_ref.quat in the dtype of R (float64: pgo_ref.quat itself)"""
    if R.dtype == f64:
        return pgo_ref.quat(R)[0]
    one, two, quarter = R.dtype.type(1), R.dtype.type(2), R.dtype.type(0.25)
    tr = (R[:, 0] + R[:, 4]) + R[:, 8]
    c = np.stack((tr, R[:, 0], R[:, 4], R[:, 8]), axis=1)
    m = np.zeros(R.shape[0], dtype=i64)
    best = c[:, 0].copy()
    with np.errstate(all="ignore"):
        for a in range(1, 4):
            win = c[:, a] > best
            best = np.where(win, c[:, a], best)
            m = np.where(win, a, m)
        s0 = np.sqrt(one + tr) * two
        s1 = np.sqrt(((one + R[:, 0]) - R[:, 4]) - R[:, 8]) * two
        s2 = np.sqrt(((one + R[:, 4]) - R[:, 0]) - R[:, 8]) * two
        s3 = np.sqrt(((one + R[:, 8]) - R[:, 0]) - R[:, 4]) * two
        q0 = np.stack((s0 * quarter, (R[:, 7] - R[:, 5]) / s0, (R[:, 2] - R[:, 6]) / s0, (R[:, 3] - R[:, 1]) / s0), axis=1)
        q1 = np.stack(((R[:, 7] - R[:, 5]) / s1, s1 * quarter, (R[:, 1] + R[:, 3]) / s1, (R[:, 2] + R[:, 6]) / s1), axis=1)
        q2 = np.stack(((R[:, 2] - R[:, 6]) / s2, (R[:, 1] + R[:, 3]) / s2, s2 * quarter, (R[:, 5] + R[:, 7]) / s2), axis=1)
        q3 = np.stack(((R[:, 3] - R[:, 1]) / s3, (R[:, 2] + R[:, 6]) / s3, (R[:, 5] + R[:, 7]) / s3, s3 * quarter), axis=1)
    return np.where((m == 0)[:, None], q0, np.where((m == 1)[:, None], q1, np.where((m == 2)[:, None], q2, q3)))


ROT = [0, 1, 2, 4, 5, 6, 8, 9, 10]
TRA = [3, 7, 11]


def blend(A, B, alpha):
    """A, B [n, 12], alpha [n] -> [n, 12]"""
    one, two = A.dtype.type(1), A.dtype.type(2)
    with np.errstate(all="ignore"):
        qa, qb = quat_any(np.ascontiguousarray(A[:, ROT])), quat_any(np.ascontiguousarray(B[:, ROT]))
        d = (((qa[:, 0] * qb[:, 0]) + (qa[:, 1] * qb[:, 1])) + (qa[:, 2] * qb[:, 2])) + (qa[:, 3] * qb[:, 3])
        qb = np.where((d < 0)[:, None], -qb, qb)
        q = qa + (alpha[:, None] * (qb - qa))
        n = np.sqrt((((q[:, 0] * q[:, 0]) + (q[:, 1] * q[:, 1])) + (q[:, 2] * q[:, 2])) + (q[:, 3] * q[:, 3]))
        w, x, y, z = q[:, 0] / n, q[:, 1] / n, q[:, 2] / n, q[:, 3] / n
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        out = np.empty_like(A)
        out[:, 0] = one - (two * (yy + zz))
        out[:, 1] = two * (xy - wz)
        out[:, 2] = two * (xz + wy)
        out[:, 4] = two * (xy + wz)
        out[:, 5] = one - (two * (xx + zz))
        out[:, 6] = two * (yz - wx)
        out[:, 8] = two * (xz - wy)
        out[:, 9] = two * (yz + wx)
        out[:, 10] = one - (two * (xx + yy))
        for c in TRA:
            out[:, c] = A[:, c] + (alpha * (B[:, c] - A[:, c]))
    return out


def alpha_of(Di, Da, Db):
    with np.errstate(all="ignore"):
        num, den = (Di - Da).astype(i64), (Db - Da).astype(i64)
        return np.where(den == 0, 0.0, num.astype(f64) / np.where(den == 0, 1, den).astype(f64))


def finite12(P):
    return np.isfinite(P).all(axis=1)


def correct(poses, D, node_scan, node_pose, dtype=f64):
    """lpd_drive_correct -> (out [S, 12], info [2] int32).  dtype=np.longdouble: the same definition in extended precision from the
    same float64 inputs (the blend weight is the float64 one)."""
    P64 = np.ascontiguousarray(poses, dtype=f64).reshape(-1, 12)
    X64 = np.ascontiguousarray(node_pose, dtype=f64).reshape(-1, 12)
    D = np.asarray(D, dtype=i64)
    ns = np.asarray(node_scan, dtype=i64)
    S, V = P64.shape[0], len(ns)
    i = np.arange(S, dtype=i64)
    a = bracket(ns, i)
    b = a + 1
    ha, hb = a >= 0, b < V
    ac, bc = np.clip(a, 0, V - 1), np.clip(b, 0, V - 1)
    sa, sb = np.where(ha, ns[ac], 0), np.where(hb, ns[bc], 0)
    ok = (~ha | ((sa >= 0) & (sa <= i))) & (~hb | ((sb > i) & (sb < S))) & (ha | hb) & finite12(P64)
    sac, sbc = np.clip(sa, 0, S - 1), np.clip(sb, 0, S - 1)
    Xa, Xb = X64[ac], X64[bc]
    exact = ok & ha & (sa == i)
    copy = exact & finite12(Xa)
    rest = ok & ~exact
    rest &= ~ha | (finite12(P64[sac]) & finite12(Xa))
    rest &= ~hb | (finite12(P64[sbc]) & finite12(Xb))
    P, Xa_t, Xb_t = P64.astype(dtype), Xa.astype(dtype), Xb.astype(dtype)
    with np.errstate(all="ignore"):
        A = candidate(P[sac], Xa_t, P)
        B = candidate(P[sbc], Xb_t, P)
        mixed = blend(A, B, alpha_of(D[i], D[sac], D[sbc]).astype(dtype))
    out = P.copy()
    out[copy] = Xa_t[copy]
    both = rest & ha & hb
    out[both] = mixed[both]
    out[rest & ha & ~hb] = A[rest & ha & ~hb]
    out[rest & hb & ~ha] = B[rest & hb & ~ha]
    made = int(copy.sum() + rest.sum())
    return out, np.array([made, S - made], dtype=np.int32)


# ---- the scene of the quality condition ---------------------------------------------------------------------------------------------------
def facade_scene(seed, poses_true, n_points=40000, reach=25.0):
    """Static world points on circular facades (radii rounded to whole metres in 36 .. 40 m and 60 .. 64 m, heights 0 .. 6 m) seen from
    the true poses: each scan holds the points within `reach` of its sensor, in its TRUE sensor frame as fp32.
    -> (points [rows, 3] fp32, lengths [S])"""
    rng = np.random.default_rng(seed)
    inner = rng.random(n_points) < 0.5
    r = np.rint(np.where(inner, rng.uniform(36.0, 40.0, n_points), rng.uniform(60.0, 64.0, n_points)))
    phi = rng.uniform(0.0, 2.0 * np.pi, n_points)
    world_pts = np.stack((r * np.cos(phi), r * np.sin(phi), rng.uniform(0.0, 6.0, n_points)), axis=1)
    P = np.asarray(poses_true, dtype=f64).reshape(-1, 3, 4)
    scans, lengths = [], []
    for R, t in zip(P[:, :, :3], P[:, :, 3]):
        d = world_pts - t
        near = np.einsum("ij,ij->i", d, d) <= reach * reach
        scans.append((d[near] @ R).astype(f32))      # R^T (p - t)
        lengths.append(int(near.sum()))
    return np.concatenate(scans), np.array(lengths, dtype=i64)


def offsets_of(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=i64)))).astype(np.int32)


def quality(points, lengths, gt, start, solved, cell=1.0):
    """-> (M_true, M_start, M_solved, share): the occupied cells under the three sets of poses, origin = the first pose's translation"""
    off = offsets_of(lengths)
    m = [occupied(points, off, p, np.asarray(p, dtype=f64).reshape(-1, 12)[0, TRA], cell) for p in (gt, start, solved)]
    return m[0], m[1], m[2], (m[1] - m[2]) / (m[1] - m[0])
