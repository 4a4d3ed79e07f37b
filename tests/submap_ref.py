"""References for lpd_make_submaps (the definition is in include/lpd_hip.h), shared by tests/test_submap_cpu.py and
tests/test_submap_gpu.py:

  (a) submap(x, N)            a numpy restatement of the definition, float32 / int64 operations exactly as stated
  (b) cell_means_fp64(...)    an independent fp64 grid average for a given rung: the fp64 mean of each cell's raw points, no
                              quantisation (cell membership is the definition's discrete part and is shared)
  seeded test clouds          scan (ground + wall + clutter to 50 m), lattice, identical, plane, two_points, translated
"""
import functools

import numpy as np

f32 = np.float32
LITERALS = np.array([f32(2.0 ** (-i / 16.0)) for i in range(16)], dtype=np.float32)
RUNGS, QBITS = 128, 20


def resolution(j):
    return f32(f32(LITERALS[j & 15] * f32(1024.0)) * f32(2.0 ** -(j >> 4)))


def scale(j, E):
    return f32(resolution(j) / f32(E)) if E > 0 else f32(0.0)


def spread10(v):
    v = v.astype(np.uint32) & np.uint32(0x3ff)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000ff)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300f00f)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030c30c3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def box(x):
    mn = x.min(axis=0).astype(np.float32)
    E = f32((x.max(axis=0).astype(np.float32) - mn).max())
    return mn, E


def keys(x, mn, s):
    t = (x - mn) * f32(s)
    assert t.dtype == np.float32
    q = np.minimum(np.maximum(t, f32(0.0)), f32(1023.0)).astype(np.uint32)
    return spread10(q[:, 0]) | (spread10(q[:, 1]) << np.uint32(1)) | (spread10(q[:, 2]) << np.uint32(2))


def quant(x, mn, E):
    fq = f32(f32(2.0 ** QBITS) / E) if E > 0 else f32(0.0)
    u = np.rint((x - mn) * fq)
    assert u.dtype == np.float32
    return u.astype(np.int64)


def fill_indices(n, fill):
    return [((2 * p + 1) * n) // (2 * fill) for p in range(fill)]


def count(x, mn, E, j):
    return int(np.unique(keys(x, mn, scale(j, E))).size)


def search(x, N):
    """-> (j*, M, {rung: count} of the rungs the bisection looked at)"""
    mn, E = box(x)
    lo, hi, seen = -1, RUNGS - 1, {}
    while hi - lo > 1:
        mid = (lo + hi) // 2
        seen[mid] = count(x, mn, E, mid)
        if seen[mid] <= N:
            hi = mid
        else:
            lo = mid
    if hi not in seen:
        seen[hi] = count(x, mn, E, hi)
    return hi, seen[hi], seen


def submap(x, N, normalize=True):
    """x [n, 3] float32 -> dict(out [N,3] f32, rows [N,3] f32 (before normalisation), info (j*, M, n, 0), xform (mean, r), counts [N]
    int32, fill [N-M] raw indices, inverse [n] row of every point)"""
    x = np.ascontiguousarray(x[:, :3], dtype=np.float32)
    n = x.shape[0]
    assert 128 <= N <= 4096 and 1 <= n <= 1 << 20
    mn, E = box(x)
    j, M, _ = search(x, N)
    uniq, inv = np.unique(keys(x, mn, scale(j, E)), return_inverse=True)
    assert uniq.size == M <= N
    u = quant(x, mn, E)
    S = np.zeros((M, 3), dtype=np.int64)
    np.add.at(S, inv, u)
    m = np.bincount(inv, minlength=M).astype(np.int32)
    qstep = f32(E * f32(2.0 ** -QBITS))
    mean_u = (S.astype(np.float64) / m.astype(np.float64)[:, None]).astype(np.float32)
    rows = np.empty((N, 3), dtype=np.float32)
    rows[:M] = mn + mean_u * qstep
    fill = fill_indices(n, N - M)
    if fill:
        rows[M:] = x[fill]
    counts = np.zeros(N, dtype=np.int32)
    counts[:M] = m
    if normalize:
        mean = (rows.astype(np.float64).sum(axis=0) / N).astype(np.float32)
        d = rows - mean
        r = f32(np.abs(d).max())
        out = d * (f32(1.0) / r) if r > 0 else np.zeros_like(d)
        xform = np.array([mean[0], mean[1], mean[2], r], dtype=np.float32)
    else:
        out, xform = rows.copy(), np.array([0, 0, 0, 1], dtype=np.float32)
    assert rows.dtype == np.float32 and out.dtype == np.float32
    return dict(out=out, rows=rows, info=(j, M, n, 0), xform=xform, counts=counts, fill=np.array(fill, dtype=np.int64), inverse=inv,
                mn=mn, E=E)


def cell_means_fp64(x, j):
    """(b): for rung j, the fp64 mean of the raw points of every occupied cell, cells in ascending key order -> [M, 3] float64"""
    x = np.ascontiguousarray(x[:, :3], dtype=np.float32)
    mn, E = box(x)
    uniq, inv = np.unique(keys(x, mn, scale(j, E)), return_inverse=True)
    out = np.zeros((uniq.size, 3), dtype=np.float64)
    np.add.at(out, inv, x.astype(np.float64))
    return out / np.bincount(inv, minlength=uniq.size)[:, None]


# ---- seeded test clouds (float32 [n, 3]) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan(n, seed):
    rng = np.random.default_rng(seed)
    ng, nw = n // 2, n // 4
    nc = n - ng - nw
    r = 50.0 * np.sqrt(rng.random(ng))                      # ground: a disc of 50 m with a little roughness
    a = 2 * np.pi * rng.random(ng)
    ground = np.stack((r * np.cos(a), r * np.sin(a), -1.7 + 0.03 * rng.standard_normal(ng)), axis=1)
    wall = np.stack((-40 + 80 * rng.random(nw), 12.0 + 0.05 * rng.standard_normal(nw), -1.7 + 8 * rng.random(nw)), axis=1)
    centres = rng.uniform((-45, -45, -1.5), (45, 45, 2.0), size=(24, 3))
    clutter = centres[rng.integers(0, 24, nc)] + rng.standard_normal((nc, 3)) * (0.8, 0.8, 0.5)
    pts = np.concatenate((ground, wall, clutter), 0)
    return np.ascontiguousarray(pts[rng.permutation(n)], dtype=np.float32)


def scan(n, seed=0):
    return _scan(int(n), int(seed)).copy()


def lattice(side=32, step=0.25):
    """side^3 points at k * step, k = 0 .. side-2 and side, per axis: E = side * step is a power of two, so at the power-of-two rungs
    (j = 16 i: R = 1024 / 2^i cells) every product (x - mn) * s is an integer and the points sit exactly ON cell boundaries -- one
    rounding more or less anywhere in the key arithmetic moves them into the neighbouring cell"""
    g = np.arange(side, dtype=np.float32)
    g[-1] = side
    g = g * f32(step)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    pts = np.stack((x.ravel(), y.ravel(), z.ravel()), axis=1)
    return np.ascontiguousarray(pts[np.random.default_rng(5).permutation(pts.shape[0])], dtype=np.float32)


def identical(n=500):
    return np.tile(np.array([[1.25, -3.5, 0.75]], dtype=np.float32), (n, 1))


def plane(n=3000, seed=2):
    p = scan(n, seed)
    p[:, 2] = 0.0
    return p


def two_points():
    return np.array([[0.0, 0.0, 0.0], [1.0, 2.0, -0.5]], dtype=np.float32)


def translated(n=3000, seed=3):
    return scan(n, seed) + np.array([10000.0, -5000.0, 200.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def cached_submap(name, n, N, normalize=True):
    """submap() of a named test cloud, computed once per session and shared (treat the result as read-only)"""
    return submap(cloud(name, n), N, normalize)


def cloud(name, n=0):
    if name == "scan":
        return scan(n)
    return {"lattice": lattice, "identical": identical, "plane": plane, "two_points": two_points, "translated": translated}[name]()
