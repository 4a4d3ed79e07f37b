"""numpy restatements for lpd_sample_items / lpd_gather_tuples (definitions: include/lpd_hip.h and csrc/lpd_tuple_math.h), shared by
tests/test_tuples_cpu.py and tests/test_tuples_gpu.py: Philox4x32-10, the uniform of a 32-bit draw, the jitter in float64, perm
(bit for bit) and both entry points."""
import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
GOLDEN = 0x9E3779B9


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words -> four uint64 arrays holding 32-bit values"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0
        p1 = np.uint64(PHILOX_M1) * c2
        n0 = (p1 >> s32) ^ c1 ^ k0
        n2 = (p0 >> s32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & m, p0 & m, n0, n2
        k0 = (k0 + np.uint64(PHILOX_W0)) & m
        k1 = (k1 + np.uint64(PHILOX_W1)) & m
    return c0, c1, c2, c3


def uniform(r):
    """((r >> 9) + 0.5) * 2^-23 in float64: the same real number the fp32 expression gives (it is exact there)"""
    return ((np.asarray(r, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(n_points, slots, seed):
    """z [len(slots), n_points, 3] float64: the three Box-Muller normals of every point, from the exact uniforms"""
    n = np.arange(n_points, dtype=np.uint64)[None, :]
    b = np.asarray(slots, dtype=np.uint64)[:, None]
    r = philox(n, b, 0, 0, seed & M32, (seed >> 32) & M32)
    u = [uniform(w) for w in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]), rb * np.cos(2 * np.pi * u[3])], axis=-1)


def jitter(n_points, slots, seed, sigma, clip):
    """delta [len(slots), n_points, 3] float64; sigma and clip are taken as the fp32 values the kernel receives"""
    s, c = float(np.float32(sigma)), float(np.float32(clip))
    return np.clip(s * normals(n_points, slots, seed), -c, c)


def mix(v):
    v = np.asarray(v, dtype=np.uint64) & np.uint64(M32)
    m = np.uint64(M32)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & m
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & m
    return v ^ (v >> np.uint64(16))


def perm_keys(seed, row):
    base = mix((seed & M32) ^ int(mix(((seed >> 32) & M32) ^ int(mix((row & M32) ^ GOLDEN)))))
    return [mix((int(base) + (i + 1) * GOLDEN) & M32) for i in range(4)]


def half_bits(c):
    h = 1
    while h < 16 and (1 << (2 * h)) < c:
        h += 1
    return h


def perm_all(c, seed, row, count=None):
    """perm(j, c, seed, row) for j = 0 .. count-1 (default all of [0, c)) -> int64 array"""
    count = c if count is None else min(count, c)
    if c <= 1:
        return np.zeros(count, dtype=np.int64)
    keys = perm_keys(seed, row)
    h = np.uint64(half_bits(c))
    mask = np.uint64((1 << int(h)) - 1)
    x = np.arange(count, dtype=np.uint64)
    todo = np.ones(count, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> h, v & mask
        for k in keys:
            L, R = R, L ^ (mix(R ^ k) & mask)
        v = (L << h) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(c)
    return x.astype(np.int64)


def perm(j, c, seed, row):
    return int(perm_all(c, seed, row, j + 1)[j]) if c > 1 else 0


def select_bit(w, r):
    """position of the r-th set bit of the 32-bit word w (r = 0: the lowest); 32 when there is none"""
    pos = [i for i in range(32) if (w >> i) & 1]
    return pos[r] if 0 <= r < len(pos) else 32


def pool(T, off, idx, lists_row, extra_row, invert):
    """ascending members of the pool of one row"""
    member = np.zeros(T, dtype=bool)
    n_lists = len(off) - 1
    for ln in lists_row:
        if 0 <= ln < n_lists:
            it = np.asarray(idx[off[ln]:off[ln + 1]], dtype=np.int64)
            member[it[(it >= 0) & (it < T)]] = True
    for it in extra_row:
        if 0 <= it < T:
            member[it] = True
    return np.nonzero(~member if invert else member)[0]


def sample_items(off, idx, T, lists, extra, m, invert, seed):
    """the definition of lpd_sample_items -> (out [R, m] int32, count [R] int32)"""
    lists = np.asarray(lists, dtype=np.int64)
    R = lists.shape[0]
    extra = np.zeros((R, 0), dtype=np.int64) if extra is None else np.asarray(extra, dtype=np.int64)
    out = np.full((R, m), -1, dtype=np.int32)
    count = np.zeros(R, dtype=np.int32)
    for r in range(R):
        z = pool(T, off, idx, lists[r], extra[r], invert)
        c = z.size
        count[r] = c
        k = min(m, c)
        if k:
            out[r, :k] = z[perm_all(c, seed, r, k)]
    return out, count


def gather_tuples(table, items, rot=None, sigma=0.0, clip=0.05, seed=0):
    """the definition of lpd_gather_tuples in float64 (the rotation products and the sum are NOT rounded to fp32 here)"""
    table = np.asarray(table)
    T, N = table.shape[:2]
    items = np.asarray(items, dtype=np.int64)
    out = np.zeros((items.size, N, 3), dtype=np.float64)
    ok = (items >= 0) & (items < T)
    out[ok] = table[items[ok]].astype(np.float64)
    if rot is not None:
        c = np.asarray(rot, dtype=np.float32).astype(np.float64)[:, 0, None]
        s = np.asarray(rot, dtype=np.float32).astype(np.float64)[:, 1, None]
        x, y = out[..., 0].copy(), out[..., 1].copy()
        out[..., 0] = x * c + y * s
        out[..., 1] = -x * s + y * c
    if sigma != 0.0:
        out += jitter(N, np.arange(items.size), seed, sigma, clip)
    out[~ok] = 0.0      # an item outside [0, T): zeros, not even jittered
    return out
