"""The numpy restatement of lpd_point_normals and lpd_icp_pairs (include/lpd_hip.h, csrc/lpd_icp_math.h) and of
lpdnet_hip/verify.py's refine_pairs: fp32 arrays, one operation per step, Python integers for the sums, Python floats (IEEE float64,
one rounding an operation) for the step.  No GPU, no scipy.  Also the perturbed starts of the quality tests (fixed seeds)."""
import math

import numpy as np

f32 = np.float32
Q, CLAMP, RANGE, SUMS, SWEEPS = f32(1024.0), f32(1048576.0), f32(512.0), 32, 6
SUM_M, SUM_H, SUM_G, SUM_RR = 0, 1, 22, 28
FLT_MAX, DBL_MAX = f32(3.402823466e+38), 1.7976931348623157e308


# ---- normals -----------------------------------------------------------------------------------------------------------------------
def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """lpd_feat_rotate over arrays; vp, vq [3, n] = the entries of the three rows of V -> the updated seven"""
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (f32(2.0) * apq)
        tt = np.copysign(f32(1.0), theta) / (np.abs(theta) + np.sqrt(theta * theta + f32(1.0)))
        t = np.where(apq == 0, f32(0.0), tt).astype(f32)
        c = f32(1.0) / np.sqrt(t * t + f32(1.0))
        s = t * c
        app2 = app - t * apq
        aqq2 = aqq + t * apq
        rp = c * arp - s * arq
        rq = s * arp + c * arq
        wp = c * vp - s * vq
        wq = s * vp + c * vq
    return app2, aqq2, np.zeros_like(apq), rp, rq, wp, wq


def moments(xyz, idx):
    """xyz [N, 3] fp32, idx [N, K] -> the nine sums of lpd_feat_add over the list, in list order, centred on the query point.  An
    index outside the cloud reads the cloud's last point."""
    xyz = np.asarray(xyz, dtype=f32)
    N = len(xyz)
    idx = np.minimum(np.asarray(idx).astype(np.int64) & 0xFFFFFFFF, N - 1)      # the unsigned minimum of the kernel
    s = {k: np.zeros(N, dtype=f32) for k in ("sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz")}
    with np.errstate(all="ignore"):
        for j in range(idx.shape[1]):
            d = xyz[idx[:, j]] - xyz
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            s["sx"] = s["sx"] + dx
            s["sy"] = s["sy"] + dy
            s["sz"] = s["sz"] + dz
            s["sxx"] = s["sxx"] + dx * dx
            s["sxy"] = s["sxy"] + dx * dy
            s["sxz"] = s["sxz"] + dx * dz
            s["syy"] = s["syy"] + dy * dy
            s["syz"] = s["syz"] + dy * dz
            s["szz"] = s["szz"] + dz * dz
    return s


def normal_from_moments(s, k):
    """lpd_icp_normal over arrays: -> (normals [n, 3] fp32, flatness [n] fp32)"""
    kf = f32(k)
    with np.errstate(all="ignore"):
        mx, my, mz = s["sx"] / kf, s["sy"] / kf, s["sz"] / kf
        a0 = s["sxx"] / kf - mx * mx
        a1 = s["syy"] / kf - my * my
        a2 = s["szz"] / kf - mz * mz
        a01 = s["sxy"] / kf - mx * my
        a02 = s["sxz"] / kf - mx * mz
        a12 = s["syz"] / kf - my * mz
        n = len(a0)
        one, zero = np.ones(n, dtype=f32), np.zeros(n, dtype=f32)
        c0, c1, c2 = np.stack((one, zero, zero)), np.stack((zero, one, zero)), np.stack((zero, zero, one))      # columns of V, [row, n]
        for _ in range(SWEEPS):
            a0, a1, a01, a02, a12, c0, c1 = _rotate(a0, a1, a01, a02, a12, c0, c1)
            a0, a2, a02, a01, a12, c0, c2 = _rotate(a0, a2, a02, a01, a12, c0, c2)
            a1, a2, a12, a01, a02, c1, c2 = _rotate(a1, a2, a12, a01, a02, c1, c2)
        l1 = np.fmax(np.fmax(a0, np.fmax(a1, a2)), f32(0.0))
        l3 = np.fmax(np.fmin(a0, np.fmin(a1, a2)), f32(0.0))
        l2 = np.fmax(np.fmax(np.fmin(a0, a1), np.fmin(np.fmax(a0, a1), a2)), f32(0.0))
        first, second = (a0 <= a1) & (a0 <= a2), a1 <= a2
        v = np.where(first, c0, np.where(second, c1, c2))
        x, y, z = v[0], v[1], v[2]
        ln = np.sqrt(((x * x) + (y * y)) + (z * z))
        fin = np.ones(n, dtype=bool)
        for val in s.values():
            fin &= np.abs(val) <= FLT_MAX
        ok = fin & (l1 > 0) & (ln > 0) & (np.abs(ln) <= FLT_MAX)
        nrm = np.where(ok, np.stack((x / ln, y / ln, z / ln)), f32(0.0)).astype(f32).T
        flat = np.where(ok & (l2 > 0), l3 / l2, f32(0.0)).astype(f32)
    return np.ascontiguousarray(nrm), flat


def point_normals(xyz, idx):
    """xyz [N, 3], idx [N, K] -> (normals [N, 3], flatness [N])"""
    return normal_from_moments(moments(xyz, idx), np.asarray(idx).shape[1])


def knn_lists(xyz, k, block=512):
    """[N, k] nearest-first lists by fp64 brute force (the point itself first): the lists of the CPU tests"""
    x = np.asarray(xyz, dtype=np.float64)
    out = np.empty((len(x), k), dtype=np.int32)
    sq = (x * x).sum(axis=1)
    for i0 in range(0, len(x), block):
        d = sq[i0:i0 + block, None] - 2.0 * (x[i0:i0 + block] @ x.T) + sq[None, :]
        d[np.arange(len(d)), np.arange(i0, i0 + len(d))] = -1.0
        part = np.argpartition(d, k - 1, axis=1)[:, :k]
        order = np.argsort(np.take_along_axis(d, part, axis=1), axis=1, kind="stable")
        out[i0:i0 + block] = np.take_along_axis(part, order, axis=1)
    return out


def eigh_normals(xyz, idx):
    """fp64: -> (unit normals [N, 3], gap [N] = (l2 - l3) / l1 of the fp64 eigenvalues, 0 where l1 == 0)"""
    x = np.asarray(xyz, dtype=np.float64)
    d = x[np.asarray(idx)] - x[:, None, :]
    mu = d.mean(axis=1)
    C = np.einsum("nki,nkj->nij", d, d) / d.shape[1] - mu[:, :, None] * mu[:, None, :]
    w, V = np.linalg.eigh(C)
    gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0), 0.0)
    return V[:, :, 0], gap


# ---- one pass ----------------------------------------------------------------------------------------------------------------------
def pose32(pose):
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4).astype(f32)
    return P[:, :3].copy(), P[:, 3].copy()


def transform(pose, a, sc):
    """-> (p [n, 3] fp32, live [n])"""
    M, u = pose32(pose)
    a = np.asarray(a, dtype=f32)
    sc = f32(sc)
    with np.errstate(all="ignore"):
        ax, ay, az = a[:, 0] * sc, a[:, 1] * sc, a[:, 2] * sc
        p = np.stack([(((M[c, 0] * ax) + (M[c, 1] * ay)) + (M[c, 2] * az)) + u[c] for c in range(3)], axis=1).astype(f32)
        live = (np.abs(p) <= RANGE).all(axis=1)      # false for NaN and inf
    return p, live


def d2(q, p):
    """q [m, 3], p [n, 3] -> [n, m] fp32"""
    with np.errstate(all="ignore"):
        dx = q[None, :, 0] - p[:, None, 0]
        dy = q[None, :, 1] - p[:, None, 1]
        dz = q[None, :, 2] - p[:, None, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def within(dd, dmax):
    with np.errstate(all="ignore"):
        return dd <= f32(dmax) * f32(dmax)


def nearest(q, p, block=256):
    """-> (j [n] int64: the nearest q, the lowest index at a tie, -1 when no distance is below +inf; dbest [n] fp32)"""
    n = len(p)
    j = np.full(n, -1, dtype=np.int64)
    best = np.full(n, np.inf, dtype=f32)
    for i0 in range(0, n, block):
        dd = d2(q, p[i0:i0 + block])
        dd = np.where(np.isnan(dd), f32(np.inf), dd)
        jj = np.argmin(dd, axis=1)      # the first minimum
        mn = dd[np.arange(len(jj)), jj]
        hit = mn < np.inf
        j[i0:i0 + block] = np.where(hit, jj, -1)
        best[i0:i0 + block] = mn
    return j, best


def quant(v):
    """(int64) rint(v * 1024) clamped to +-2^20, half to even; NaN -> 0"""
    with np.errstate(all="ignore"):
        s = np.asarray(v, dtype=f32) * Q
        s = np.where(s > CLAMP, CLAMP, s)
        s = np.where(s < -CLAMP, -CLAMP, s)
        return np.where(np.isnan(s), 0.0, np.rint(s)).astype(np.int64)


def rows(p, q, n):
    """-> (Ji [m, 6] int64, ri [m] int64) of m correspondences"""
    with np.errstate(all="ignore"):
        e = q - p
        r = ((e[:, 0] * n[:, 0]) + (e[:, 1] * n[:, 1])) + (e[:, 2] * n[:, 2])
        cx = (p[:, 1] * n[:, 2]) - (p[:, 2] * n[:, 1])
        cy = (p[:, 2] * n[:, 0]) - (p[:, 0] * n[:, 2])
        cz = (p[:, 0] * n[:, 1]) - (p[:, 1] * n[:, 0])
    return np.stack([quant(v) for v in (cx, cy, cz, n[:, 0], n[:, 1], n[:, 2])], axis=1), quant(r)


def sums_of(Ji, ri):
    """the 32 sums as Python integers (int64 is wide enough: 2^14 terms of at most 2^40)"""
    s = [0] * SUMS
    s[SUM_M] = int(len(ri))
    e = SUM_H
    for a in range(6):
        for b in range(a, 6):
            s[e] = int((Ji[:, a] * Ji[:, b]).sum())
            e += 1
    for a in range(6):
        s[SUM_G + a] = int((Ji[:, a] * ri).sum())
    s[SUM_RR] = int((ri * ri).sum())
    return s


def one_pass(pose, a, sc_a, b, sc_b, normals_b, dmax):
    """-> (sums [32] list of int, nn [N] int32)"""
    p, live = transform(pose, a, sc_a)
    with np.errstate(all="ignore"):
        q = (np.asarray(b, dtype=f32) * f32(sc_b)).astype(f32)
    j, best = nearest(q, p)
    has = live & (j >= 0) & within(best, dmax)
    js = np.where(has, j, 0)
    nb = np.asarray(normals_b, dtype=f32)[js]
    has &= ~((nb[:, 0] == 0) & (nb[:, 1] == 0) & (nb[:, 2] == 0))
    Ji, ri = rows(p[has], q[js[has]], nb[has])
    return sums_of(Ji, ri), np.where(has, j, -1).astype(np.int32)


# ---- the step ----------------------------------------------------------------------------------------------------------------------
def _finite(v):
    return abs(v) <= DBL_MAX      # false for NaN


def ldl(sums):
    """-> x [6] list of float, or None when a pivot is not positive and finite"""
    A = [[0.0] * 6 for _ in range(6)]
    e = SUM_H
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = float(int(sums[e]))      # int -> float64: one rounding, to nearest even
            e += 1
    L = [[0.0] * 6 for _ in range(6)]
    D, v, y, x = [0.0] * 6, [0.0] * 6, [0.0] * 6, [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            v[k] = L[j][k] * D[k]
            d = d - (L[j][k] * v[k])
        if not (d > 0.0 and _finite(d)):
            return None
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - (L[i][k] * v[k])
            L[i][j] = s / d
    for i in range(6):
        s = float(int(sums[SUM_G + i]))
        for k in range(i):
            s = s - (L[i][k] * y[k])
        y[i] = s
    for i in range(6):
        y[i] = y[i] / D[i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - (L[k][i] * x[k])
        x[i] = s
    return x


def update(x, pose):
    """pose [12] list of float -> the new [12]"""
    hx, hy, hz = x[0] * 0.5, x[1] * 0.5, x[2] * 0.5
    ln = math.sqrt(((1.0 + (hx * hx)) + (hy * hy)) + (hz * hz))
    qw, qx, qy, qz = 1.0 / ln, hx / ln, hy / ln, hz / ln
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    dR = [[1.0 - (2.0 * (yy + zz)), 2.0 * (xy - wz), 2.0 * (xz + wy)],
          [2.0 * (xy + wz), 1.0 - (2.0 * (xx + zz)), 2.0 * (yz - wx)],
          [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - (2.0 * (xx + yy))]]
    out = [0.0] * 12
    for i in range(3):
        for j in range(4):
            out[4 * i + j] = ((dR[i][0] * pose[j]) + (dR[i][1] * pose[4 + j])) + (dR[i][2] * pose[8 + j])
        out[4 * i + 3] = out[4 * i + 3] + x[3 + i]
    return out


def solve(sums, min_inliers, pose):
    """-> (applied, pose [12] float64 array): a refused step returns the pose's own values"""
    pose = [float(v) for v in np.asarray(pose, dtype=np.float64).reshape(12)]
    with np.errstate(all="ignore"):
        if int(sums[SUM_M]) < int(min_inliers):
            return False, np.array(pose)
        try:
            x = ldl(sums)
            if x is None or not all(_finite(v) for v in x):
                return False, np.array(pose)
            new = update(x, pose)
        except (OverflowError, ZeroDivisionError):      # Python raises where IEEE gives inf or NaN: a refusal either way
            return False, np.array(pose)
        if not all(_finite(v) for v in new):
            return False, np.array(pose)
    return True, np.array(new)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
def icp_pair(a, b, normals_b, pose, dmax, min_inliers, sc_a=1.0, sc_b=1.0):
    """dmax: iters + 1 distances -> dict(pose [12], info [4], sums [iters + 1, 32] int64, nn [N])"""
    iters = len(dmax) - 1
    pose = np.asarray(pose, dtype=np.float64).reshape(12).copy()
    sums = np.zeros((iters + 1, SUMS), dtype=np.int64)
    applied = refused = 0
    nn = None
    for s in range(iters + 1):
        ss, nn = one_pass(pose, a, sc_a, b, sc_b, normals_b, dmax[s])
        sums[s] = ss
        if s < iters:
            ok, pose = solve(ss, min_inliers, pose)
            applied += int(ok)
            refused += int(not ok)
    return dict(pose=pose, info=np.array([1, applied, refused, int(sums[-1, 0])], dtype=np.int32), sums=sums, nn=nn)


def icp_pairs(A, B, normalsB, pairs, pose, dmax, min_inliers, scaleA=None, scaleB=None):
    """A [TA, N, 3], B [TB, N, 3], normalsB [TB, N, 3], pairs [P, 2], pose [P, 12] -> (pose [P, 12], info [P, 4] int32,
    sums [iters + 1, P, 32] int64, nn [P, N] int32); a pair outside its table is not read"""
    P, N, iters = len(pairs), A.shape[1], len(dmax) - 1
    pose = np.array(pose, dtype=np.float64).reshape(P, 12)
    info = np.zeros((P, 4), dtype=np.int32)
    sums = np.zeros((iters + 1, P, SUMS), dtype=np.int64)
    nn = np.full((P, N), -1, dtype=np.int32)
    for p, (ra, rb) in enumerate(np.asarray(pairs).tolist()):
        if not (0 <= ra < len(A) and 0 <= rb < len(B)):
            info[p, 0] = -1
            continue
        r = icp_pair(A[ra], B[rb], normalsB[rb], pose[p], dmax, min_inliers, 1.0 if scaleA is None else scaleA[ra],
                     1.0 if scaleB is None else scaleB[rb])
        pose[p], info[p], sums[:, p], nn[p] = r["pose"], r["info"], r["sums"], r["nn"]
    return pose, info, sums, nn


def rms(sums_last):
    m = int(sums_last[SUM_M])
    return math.sqrt(int(sums_last[SUM_RR]) / m) / 1024.0 if m > 0 else 0.0


# ---- poses of the quality tests ----------------------------------------------------------------------------------------------------
def rot_xyz(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_error(pose, R_true, t_true):
    """-> (rotation error in degrees, translation error in metres) of a [12] pose against the truth"""
    Pm = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    dR = Pm[:, :3] @ np.asarray(R_true).T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(Pm[:, 3] - np.asarray(t_true)))


FINE_YAW_DEG, FINE_SHIFT_M, TILT_DEG, Z_M = 0.38, 0.11, 5.0, 1.0      # the fine pass's residual; the tilt and z offset given to A


def tilted_true_pair(seed, n=4096):
    """align_ref.true_pair with A tilted: A' = T^-1 A for a seeded T of up to 5 degrees of roll and pitch and up to 1 m of z, so that
    the truth becomes p_B = R(yaw) T p_A' + t.  -> (a', b, R_true [3, 3], t_true [3], start [12]): the start is what the fine pass
    leaves -- the true yaw and planar shift off by up to its residual, no roll, pitch or z."""
    import align_ref
    a, b, yaw, t = align_ref.true_pair(seed) if n == 4096 else _true_pair_n(seed, n)
    g = np.random.default_rng(3000 + seed)
    Rt = rot_xyz(math.radians(g.uniform(-TILT_DEG, TILT_DEG)), math.radians(g.uniform(-TILT_DEG, TILT_DEG)), 0.0)
    tz = np.array([0.0, 0.0, g.uniform(-Z_M, Z_M)])
    a2 = ((a.astype(np.float64) - tz) @ Rt).astype(f32)      # rows: Rt^T (a - tz)
    Rz = rot_xyz(0.0, 0.0, yaw)
    R_true = Rz @ Rt
    t_true = Rz @ tz + np.array([t[0], t[1], 0.0])
    y0 = yaw + math.radians(g.uniform(-FINE_YAW_DEG, FINE_YAW_DEG))
    start = np.zeros((3, 4))
    start[:, :3] = rot_xyz(0.0, 0.0, y0)
    start[:2, 3] = np.asarray(t) + g.uniform(-FINE_SHIFT_M, FINE_SHIFT_M, 2)
    return a2, b, R_true, t_true, start.reshape(12)


def _true_pair_n(seed, n):
    import align_ref
    g = np.random.default_rng(1000 + seed)
    sc = align_ref.scene(seed)
    pos_b, th_b, th_a = g.uniform(-30.0, 30.0, 2), g.uniform(0, 2 * np.pi), g.uniform(0, 2 * np.pi)
    t = g.uniform(-3.0, 3.0, 2)
    cb, sb = math.cos(th_b), math.sin(th_b)
    pos_a = pos_b + np.array([cb * t[0] - sb * t[1], sb * t[0] + cb * t[1]])
    return (align_ref.submap(sc, pos_a, th_a, 2 * seed + 1, n=n), align_ref.submap(sc, pos_b, th_b, 2 * seed + 2, n=n),
            (th_a - th_b) % (2 * np.pi), t)
