"""The numpy restatement of lpd_align_pairs (include/lpd_hip.h, csrc/lpd_align_math.h) and of the coarse-to-fine chain of
lpdnet_hip/verify.py: fp32 arrays, one operation per step, boolean bitmaps, slices of a zero-padded bitmap for the shifts.  No GPU.
Also the labelled street scenes of the quality tests (fixed seeds)."""
import math

import numpy as np

f32 = np.float32
GRID = 128
MAX_S, MAX_LAYERS, MAX_H, MAX_R, MAX_POINTS = 16, 4, 1024, 8192, 16384
DEFAULTS = dict(cell=0.5, shifts=8, yaw_steps=120, layers=4, z_lo=0.0, z_cell=2.0, fine=True, fine_div=8, fine_shifts=4)


def rot_table(R):
    """(cos, sin) of 2 pi m / R in float64, rounded to fp32 once: the table the caller of the kernel makes on the host"""
    ang = 2.0 * np.pi * np.arange(R, dtype=np.float64) / float(R)
    return np.stack((np.cos(ang), np.sin(ang)), axis=1).astype(f32)


def rot_index(first, h, R):
    return (int(first) + int(h)) % int(R)      # Python's remainder is the non-negative one


def cells(pts, sc, inv_cell, z0, inv_zcell, layers, cs=None, t0=None):
    """pts [n, 3] fp32 -> (ix, iy, iz, valid).  cs = (c, s) rotates (cloud A), t0 = (t0x, t0y) is then added; None: cloud B."""
    pts = np.asarray(pts, dtype=f32)
    sc, inv_cell, z0, inv_zcell = f32(sc), f32(inv_cell), f32(z0), f32(inv_zcell)
    with np.errstate(all="ignore"):
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        raw = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        px, py, pz = x * sc, y * sc, z * sc
        if cs is None:
            xr, yr = px, py
        else:
            c, s = f32(cs[0]), f32(cs[1])
            xr = (px * c) - (py * s)
            yr = (px * s) + (py * c)
            if t0 is not None:
                xr = xr + f32(t0[0])
                yr = yr + f32(t0[1])
        fx = np.floor(xr * inv_cell) + f32(64.0)
        fy = np.floor(yr * inv_cell) + f32(64.0)
        fz = np.floor((pz - z0) * inv_zcell)
        valid = raw & (fx >= 0) & (fx < 128) & (fy >= 0) & (fy < 128) & (fz >= 0) & (fz < layers)      # NaN fails every comparison
    ix = np.where(valid, fx, 0).astype(np.int64)
    iy = np.where(valid, fy, 0).astype(np.int64)
    iz = np.where(valid, fz, 0).astype(np.int64)
    return ix, iy, iz, valid


def bitmap(pts, sc, inv_cell, z0, inv_zcell, layers, cs=None, t0=None):
    """occ [layers, 128 (iy), 128 (ix)] bool"""
    ix, iy, iz, valid = cells(pts, sc, inv_cell, z0, inv_zcell, layers, cs, t0)
    occ = np.zeros((layers, GRID, GRID), dtype=bool)
    occ[iz[valid], iy[valid], ix[valid]] = True
    return occ


def score_slices(occA, occB, dy, dx):
    """score(dy, dx) = sum over layers and rows of popcount(shift(occA[l][iy], dx) & occB[l][iy + dy]), by slicing alone"""
    y0, y1 = max(0, -dy), min(GRID, GRID - dy)
    x0, x1 = max(0, -dx), min(GRID, GRID - dx)
    return int(np.count_nonzero(occA[:, y0:y1, x0:x1] & occB[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]))


def scores_all(occA_all, occB, S):
    """occA_all [H, L, 128, 128] bool -> [H, 2S+1 (dy), 2S+1 (dx)] int64.  The window of the zero-padded B at (dy, dx) is B moved by
    (-dy, -dx); the count of the AND is a dot product of 0/1 values in fp32, exact below 2^24."""
    H, L = occA_all.shape[:2]
    W = 2 * S + 1
    pad = np.zeros((L, GRID + 2 * S, GRID + 2 * S), dtype=bool)
    pad[:, S:S + GRID, S:S + GRID] = occB
    Af = occA_all.reshape(H, -1).astype(f32)
    out = np.zeros((H, W, W), dtype=np.int64)
    for dyi in range(W):
        win = np.stack([pad[:, dyi:dyi + GRID, dxi:dxi + GRID].ravel() for dxi in range(W)]).astype(f32)
        out[:, dyi, :] = np.rint(Af @ win.T).astype(np.int64)
    return out


def align_pair(a, b, rot, H, inv_cell, S, z0, inv_zcell, layers, sc_a=1.0, sc_b=1.0, first=0, t0=None):
    """-> (best [8] = (h, dy, dx, score, nA, nB, 1, 0), yaw_scores [H])"""
    R = len(rot)
    occB = bitmap(b, sc_b, inv_cell, z0, inv_zcell, layers)
    occA = np.stack([bitmap(a, sc_a, inv_cell, z0, inv_zcell, layers, rot[rot_index(first, h, R)], t0) for h in range(H)])
    sc = scores_all(occA, occB, S)
    flat = int(np.argmax(sc))      # the first maximum in C order: the smallest (h, dy + S, dx + S)
    W = 2 * S + 1
    h, dyi, dxi = flat // (W * W), (flat // W) % W, flat % W
    best = [h, dyi - S, dxi - S, int(sc[h, dyi, dxi]), int(occA[h].sum()), int(occB.sum()), 1, 0]
    return np.array(best, dtype=np.int32), sc.reshape(H, -1).max(axis=1).astype(np.int32)


def align_pairs(A, B, pairs, rot, H, inv_cell, S, z0, inv_zcell, layers, scaleA=None, scaleB=None, first=None, t0=None):
    """A [TA, N, 3], B [TB, N, 3], pairs [P, 2] -> (best [P, 8] int32, yaw_scores [P, H] int32); a pair outside its table is not read"""
    P = len(pairs)
    best = np.zeros((P, 8), dtype=np.int32)
    ys = np.zeros((P, H), dtype=np.int32)
    for p, (ra, rb) in enumerate(np.asarray(pairs).tolist()):
        if not (0 <= ra < len(A) and 0 <= rb < len(B)):
            best[p, 0] = -1
            continue
        best[p], ys[p] = align_pair(A[ra], B[rb], rot, H, inv_cell, S, z0, inv_zcell, layers,
                                    1.0 if scaleA is None else scaleA[ra], 1.0 if scaleB is None else scaleB[rb],
                                    0 if first is None else first[p], None if t0 is None else t0[p])
    return best, ys


def chain(A, B, pairs, search=None, scaleA=None, scaleB=None):
    """verify.align_pairs: the coarse pass, then (search['fine']) the fine pass around its winner.  -> dict of coarse, fine (or None),
    yaw_scores, yaw [P] float64, translation [P, 2] float64, score, cells_a, cells_b, overlap, valid"""
    s = dict(DEFAULTS)
    s.update(search or {})
    H, cell = s["yaw_steps"], s["cell"]
    inv_z = f32(1.0 / s["z_cell"])
    coarse, ys = align_pairs(A, B, pairs, rot_table(H), H, f32(1.0 / cell), s["shifts"], s["z_lo"], inv_z, s["layers"], scaleA, scaleB)
    valid = coarse[:, 6] == 1
    fine, last = None, coarse
    if s["fine"]:
        fd = s["fine_div"]
        R = H * fd
        first = np.array([(int(h) * fd - fd) % R for h in coarse[:, 0]], dtype=np.int32)
        t0 = np.stack((coarse[:, 2].astype(f32) * f32(cell), coarse[:, 1].astype(f32) * f32(cell)), axis=1)
        fine, _ = align_pairs(A, B, pairs, rot_table(R), 2 * fd + 1, f32(1.0 / (cell / 2.0)), s["fine_shifts"], s["z_lo"], inv_z, s["layers"],
                              scaleA, scaleB, first, t0)
        last = fine
        m = (first.astype(np.int64) + fine[:, 0]) % R
        yaw = m.astype(np.float64) * (2.0 * math.pi / R)
        translation = t0.astype(np.float64) + np.stack((fine[:, 2], fine[:, 1]), axis=1).astype(np.float64) * (cell / 2.0)
    else:
        yaw = coarse[:, 0].astype(np.float64) * (2.0 * math.pi / H)
        translation = np.stack((coarse[:, 2], coarse[:, 1]), axis=1).astype(np.float64) * cell
    yaw = np.where(valid, yaw, 0.0)
    translation = np.where(valid[:, None], translation, 0.0)
    least = np.minimum(last[:, 4], last[:, 5])
    overlap = np.where(least > 0, last[:, 3] / np.maximum(least, 1).astype(np.float64), 0.0)
    return dict(coarse=coarse, fine=fine, yaw_scores=ys, yaw=yaw, translation=translation, score=last[:, 3], cells_a=last[:, 4],
                cells_b=last[:, 5], overlap=overlap, valid=valid)


# ---- the 128-bit row of the kernel, as a Python integer ----
def row_int(words):
    return sum(int(w) << (32 * j) for j, w in enumerate(words))


def row_words(v):
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(4)]


def shift_int(v, dx):
    """bit ix -> ix + dx, bits leaving [0, 128) dropped"""
    return ((v << dx) if dx >= 0 else (v >> -dx)) & ((1 << 128) - 1)


# ---- labelled street scenes ----
def scene(seed, extent=70.0):
    """Walls 5-30 m long and 2-8 m high along two street directions (with a little jitter), poles, low clutter; no ground (the road
    is removed before a submap is made).  z is the height above the road."""
    g = np.random.default_rng(seed)
    n_w, n_p, n_c = 70, 60, 120
    ang = g.choice([0.0, np.pi / 2], n_w) + g.normal(0.0, 0.12, n_w)
    mid = g.uniform(-extent, extent, (n_w, 2))
    half = g.uniform(5.0, 30.0, n_w)[:, None] * 0.5 * np.stack((np.cos(ang), np.sin(ang)), axis=1)
    return dict(w0=mid - half, w1=mid + half, wh=g.uniform(2.0, 8.0, n_w),
                poles=g.uniform(-extent, extent, (n_p, 2)), ph=g.uniform(3.0, 8.0, n_p),
                clutter=g.uniform(-extent, extent, (n_c, 2)), cs=g.uniform(0.3, 1.0, n_c), ch=g.uniform(0.3, 1.0, n_c))


def submap(sc, pos, heading, seed, n=4096, radius=25.0, noise=0.02):
    """n points of the scene within `radius` of pos (plan view), drawn afresh (its own seed), with 2 cm noise, in the frame of a
    sensor at pos looking along `heading`: p_world = R(heading) p + pos.  -> [n, 3] fp32"""
    g = np.random.default_rng(seed)
    pos = np.asarray(pos, dtype=np.float64)
    parts = []
    for p0, p1, h in zip(sc["w0"], sc["w1"], sc["wh"]):
        m = int(np.linalg.norm(p1 - p0) * h * 6.0)
        u = g.random(m)[:, None]
        parts.append(np.column_stack((p0 + u * (p1 - p0), g.random(m) * h)))
    for c, h in zip(sc["poles"], sc["ph"]):
        m = 60
        a = g.uniform(0, 2 * np.pi, m)
        parts.append(np.column_stack((c[0] + 0.12 * np.cos(a), c[1] + 0.12 * np.sin(a), g.random(m) * h)))
    for c, s, h in zip(sc["clutter"], sc["cs"], sc["ch"]):
        m = 40
        parts.append(np.column_stack((c[0] + g.uniform(-s, s, m), c[1] + g.uniform(-s, s, m), g.random(m) * h)))
    w = np.concatenate(parts)
    w = w[np.hypot(w[:, 0] - pos[0], w[:, 1] - pos[1]) <= radius]
    if len(w) == 0:
        return np.full((n, 3), 1e6, dtype=f32)
    w = w[g.choice(len(w), n, replace=len(w) < n)] + g.normal(0.0, noise, (n, 3))
    c, s = math.cos(heading), math.sin(heading)
    d = w[:, :2] - pos
    return np.column_stack((c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], w[:, 2])).astype(f32)


def true_pair(seed):
    """Two submaps of one scene: B at a random position and heading, A at B's position plus an offset of up to 3 m per axis (in B's
    frame, the frame the shift window is laid out in), with an independent heading.  -> (a, b, yaw, t): p_B = R(yaw) p_A + t."""
    g = np.random.default_rng(1000 + seed)
    sc = scene(seed)
    pos_b, th_b, th_a = g.uniform(-30.0, 30.0, 2), g.uniform(0, 2 * np.pi), g.uniform(0, 2 * np.pi)
    t = g.uniform(-3.0, 3.0, 2)
    cb, sb = math.cos(th_b), math.sin(th_b)
    pos_a = pos_b + np.array([cb * t[0] - sb * t[1], sb * t[0] + cb * t[1]])
    return submap(sc, pos_a, th_a, 2 * seed + 1), submap(sc, pos_b, th_b, 2 * seed + 2), (th_a - th_b) % (2 * np.pi), t


def false_pair(seed):
    """Two submaps of one scene 40 m or more apart, with independent headings"""
    g = np.random.default_rng(2000 + seed)
    sc = scene(seed)
    pos_b = g.uniform(-40.0, 40.0, 2)
    while True:
        pos_a = g.uniform(-40.0, 40.0, 2)
        if np.linalg.norm(pos_a - pos_b) >= 40.0:
            break
    return submap(sc, pos_a, g.uniform(0, 2 * np.pi), 2 * seed + 5), submap(sc, pos_b, g.uniform(0, 2 * np.pi), 2 * seed + 6)


def yaw_error(a, b):
    d = (a - b) % (2 * np.pi)
    return min(d, 2 * np.pi - d)
