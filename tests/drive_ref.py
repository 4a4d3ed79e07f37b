"""Numpy restatement of the drive step (include/lpd_hip.h, "Submaps from a drive"), written from the definition: steps, distance,
windows, plan, relative pose, rows.  Every float64 / fp32 operation is one numpy operation on arrays of that dtype, so each is
rounded once and nothing is contracted; distances are Python / int64 integers.  Used by tests/test_drive_cpu.py (against
csrc/lpd_drive_math.h compiled for the host) and tests/test_drive_gpu.py (against the kernels, exact equality)."""
import numpy as np

f32 = np.float32
UNITS = 65536
QMAX = 1 << 36


def units(metres):
    """rint(metres * 65536) as a Python integer (half to even)"""
    return int(np.rint(np.float64(metres) * np.float64(UNITS)))


def dot3(a0, a1, a2, b0, b1, b2):
    return ((a0 * b0) + (a1 * b1)) + (a2 * b2)


def quant(dl):
    """[n] float64 lengths -> int64 units: rint, clamped to [0, 2^36], 0 where the length is not finite"""
    dl = np.asarray(dl, dtype=np.float64)
    with np.errstate(all="ignore"):
        v = np.rint(dl * np.float64(UNITS))
    ok = np.isfinite(dl) & (v >= 0)
    v = np.where(ok, np.minimum(v, np.float64(QMAX)), 0.0)
    return v.astype(np.int64)


def step_lengths(poses):
    """poses [S, 12] float64 -> dl [S] float64, dl_0 = 0"""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    t = P[:, [3, 7, 11]]
    with np.errstate(all="ignore"):
        d = t[1:] - t[:-1]
        dl = np.sqrt(dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    return np.concatenate((np.zeros(1), dl))


def steps(poses):
    q = quant(step_lengths(poses))
    q[0] = 0
    return q


def distance(q):
    return np.cumsum(np.asarray(q, dtype=np.int64))


def lower_bound(D, v):
    """the first i with D[i] >= v, len(D) when there is none"""
    return int(np.searchsorted(np.asarray(D), v, side="left"))


def window_count(D_last, L, T):
    D_last, L, T = int(D_last), int(L), int(T)
    return (D_last - L) // T + 1 if D_last >= L else 0


def window(D, L, T, w):
    """-> (first, end, ref) of window w; (S, S, -1) behind the drive's last window"""
    S = len(D)
    lo = int(w) * int(T)
    if lo + L > int(D[-1]):
        return S, S, -1
    first, end = lower_bound(D, lo), lower_bound(D, lo + L)
    if first == end:
        return first, end, -1
    return first, end, min(lower_bound(D, lo + L // 2), end - 1)


def plan(D, offsets, poses, L, T, w0, W):
    """-> (plan [W, 4] int32, position [W, 3] float64)"""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    table = np.zeros((W, 4), dtype=np.int32)
    position = np.zeros((W, 3), dtype=np.float64)
    for j in range(W):
        first, end, ref = window(D, L, T, w0 + j)
        table[j] = (first, end, ref, int(offsets[end]) - int(offsets[first]))
        if ref >= 0:
            position[j] = P[ref, [3, 7, 11]]
    return table, position


def rel(Pi, Pr, frame):
    """the pose of a scan relative to the reference scan -> (M [3, 3] fp32, u [3] fp32)"""
    Pi, Pr = np.asarray(Pi, dtype=np.float64).reshape(3, 4), np.asarray(Pr, dtype=np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        d = Pi[:, 3] - Pr[:, 3]
        if frame:
            M = np.empty((3, 3), dtype=np.float64)
            u = np.empty(3, dtype=np.float64)
            for c in range(3):
                a = Pr[:, c]
                for k in range(3):
                    b = Pi[:, k]
                    M[c, k] = dot3(a[0], a[1], a[2], b[0], b[1], b[2])
                u[c] = dot3(a[0], a[1], a[2], d[0], d[1], d[2])
        else:
            M, u = Pi[:, :3].copy(), d
        return M.astype(f32), u.astype(f32)


def transform(M, u, xyz):
    """rows [n, 3] fp32 by (M, u) fp32 -> [n, 3] fp32"""
    x, y, z = (np.ascontiguousarray(xyz[:, c], dtype=f32) for c in range(3))
    out = np.empty((len(x), 3), dtype=f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            out[:, c] = (((M[c, 0] * x) + (M[c, 1] * y)) + (M[c, 2] * z)) + u[c]
    return out


def scan_of(offsets, g):
    """the last scan i with offsets[i] <= g"""
    return int(np.searchsorted(np.asarray(offsets), g, side="right")) - 1


def rows(points, offsets, poses, table, frame, max_len=None):
    """the rows of the windows of a plan table -> (out [sum rows, 3] fp32, out_off [W+1] int64, written [W] bool).  A window longer
    than max_len is not written: its rows stay NaN-free zeros here and `written` says so."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    n = table[:, 3].astype(np.int64)
    out_off = np.concatenate(([0], np.cumsum(n)))
    out = np.zeros((int(out_off[-1]), 3), dtype=f32)
    written = np.zeros(len(table), dtype=bool)
    for w, (first, end, ref, nr) in enumerate(table):
        if ref < 0 or nr == 0 or (max_len is not None and nr > max_len):
            continue
        written[w] = True
        at = int(out_off[w])
        for i in range(first, end):
            a, b = int(offsets[i]), int(offsets[i + 1])
            if b > a:
                M, u = rel(P[i], P[ref], frame)
                out[at:at + b - a] = transform(M, u, points[a:b, :3])
                at += b - a
    return out, out_off, written


def drive(points, lengths, poses, length, stride, frame):
    """the whole step for one drive -> dict(q, D, L, T, W, plan, position, out, out_off, offsets)"""
    offsets = np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64))))
    q = steps(poses)
    D = distance(q)
    L, T = units(length), units(stride)
    W = window_count(D[-1], L, T)
    table, position = plan(D, offsets, poses, L, T, 0, W)
    out, out_off, _ = rows(np.asarray(points, dtype=f32), offsets, poses, table, frame)
    return dict(q=q, D=D, L=L, T=T, W=W, plan=table, position=position, out=out, out_off=out_off, offsets=offsets)


def make_drive(g, lengths, step=1.0, heading_noise=0.02, origin=(0.0, 0.0, 0.0), point_scale=20.0):
    """A smooth random drive: S = len(lengths) poses that advance `step` metres (a scalar or [S-1]) along a slowly turning heading,
    with a small roll and pitch, and random sensor-frame points.  -> (points [sum, 3] fp32, poses [S, 12] float64)"""
    S = len(lengths)
    step = np.broadcast_to(np.asarray(step, dtype=np.float64), (max(S - 1, 0),))
    yaw = np.cumsum(g.normal(0.0, heading_noise, S))
    roll, pitch = g.normal(0.0, 0.01, S), g.normal(0.0, 0.01, S)
    t = np.zeros((S, 3))
    t[0] = origin
    for i in range(1, S):
        t[i] = t[i - 1] + step[i - 1] * np.array([np.cos(yaw[i]), np.sin(yaw[i]), 0.01 * np.sin(0.1 * i)])
    poses = np.zeros((S, 12))
    for i in range(S):
        cy, sy, cp, sp, cr, sr = np.cos(yaw[i]), np.sin(yaw[i]), np.cos(pitch[i]), np.sin(pitch[i]), np.cos(roll[i]), np.sin(roll[i])
        R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
            np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        poses[i] = np.concatenate((R, t[i][:, None]), 1).reshape(12)
    points = (g.uniform(-1.0, 1.0, (int(np.sum(lengths)), 3)) * point_scale).astype(f32)
    return points, poses


def rows_extended(points, offsets, poses, table, frame):
    """the same rows in extended precision (np.longdouble), from the float64 poses and the fp32 points: the yardstick of the fp32 error"""
    ld = np.longdouble
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3, 4).astype(ld)
    n = table[:, 3].astype(np.int64)
    out_off = np.concatenate(([0], np.cumsum(n)))
    out = np.zeros((int(out_off[-1]), 3), dtype=ld)
    for w, (first, end, ref, nr) in enumerate(table):
        if ref < 0:
            continue
        at = int(out_off[w])
        Rr, tr = P[ref, :, :3], P[ref, :, 3]
        for i in range(first, end):
            a, b = int(offsets[i]), int(offsets[i + 1])
            if b > a:
                Ri, ti = P[i, :, :3], P[i, :, 3]
                M, u = (Rr.T @ Ri, Rr.T @ (ti - tr)) if frame else (Ri, ti - tr)
                out[at:at + b - a] = points[a:b, :3].astype(ld) @ M.T + u
                at += b - a
    return out
