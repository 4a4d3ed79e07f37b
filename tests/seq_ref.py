"""numpy restatement of lpd_seq_match (include/lpd_hip.h; csrc/lpd_seq_math.h is the definition) and of lpdnet_hip/sequence.py.

Scalar functions restate the header one for one (tests/test_seqmatch_cpu.py compares them with the compiled header value for
value); `match` is the whole stage over a table of blocks, vectorised, and `match_slow` the same thing written as the definition
reads, with the integer comparator.  The blocks come either from the device (the GPU tests hand the device's own block back, so that
what is compared is everything behind the quantisation) or from float64 distances (`blocks_f64`)."""
import numpy as np

BAND, QBITS, TILE = 15, 14, 32
f32 = np.float32


# ---- the header, one for one ---------------------------------------------------------------------------------------------------------
def quant(d2):
    """int32 of fp32 d2: rint(min(max(d2, 0), 16) * 2^14), half to even; -1 for NaN"""
    d2 = np.asarray(d2, dtype=f32)
    with np.errstate(invalid="ignore"):
        v = np.minimum(np.maximum(d2, f32(0)), f32(16)) * f32(16384)
    return np.where(np.isnan(d2), -1, np.rint(np.where(np.isnan(v), 0, v))).astype(np.int32)


def d2q(qn, dn, dot):
    """x = (qn + dn) - (2 dot) in fp32, three operations; -1 where x is NaN, else quant(max(x, 0))"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (np.asarray(qn, dtype=f32) + np.asarray(dn, dtype=f32)) - (f32(2) * np.asarray(dot, dtype=f32))
    return np.where(np.isnan(x), -1, quant(np.where(np.isnan(x), f32(0), np.maximum(x, f32(0))))).astype(np.int32)


def hyp(v, s, S):
    return v * (2 * S + 1) + (s + S)


def hyp_v(e, S):
    return e // (2 * S + 1)


def hyp_s(e, S):
    return e % (2 * S + 1) - S


def band(row, j):
    return row - j + BAND


def run_of(off, x):
    """the largest m in [0, len(off) - 1) with off[m] <= x"""
    off = np.asarray(off)
    return np.clip(np.searchsorted(off, x, side="right") - 1, 0, len(off) - 2)


def counted(a, qlo, qhi, b, dlo, dhi, dq):
    return bool(qlo <= a < qhi and dlo <= b < dhi and dq >= 0)


def better(sum1, n1, key1, sum2, n2, key2):
    """Python integers: exact.  key < 0 is "none"."""
    if key1 < 0:
        return False
    if key2 < 0:
        return True
    l, r = int(sum1) * int(n2), int(sum2) * int(n1)
    return l < r or (l == r and key1 < key2)


def hypothesis(blk, st, h, s, i, qlo, qhi, j, dlo, dhi):
    """(sum, n) of one hypothesis over the block blk [32, 32] of candidate (i, j)"""
    total = n = 0
    for t in range(-h, h + 1):
        b = j + s + int(st[t + h])
        bp = band(b, j)
        if not 0 <= bp <= 2 * BAND:
            continue
        dq = int(blk[t + h, bp])
        if counted(i + t, qlo, qhi, b, dlo, dhi, dq):
            total += dq
            n += 1
    return total, n


def steps_table(velocities, h):
    """[V, 2h + 1] int32 by Python's round (half to even)"""
    return np.array([[round(float(v) * t) for t in range(-h, h + 1)] for v in velocities], dtype=np.int32)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------
def dq_matrix_f64(Q, D):
    """[nq, nd] int32: float64 squared distances |q|^2 + |d|^2 - 2 q.d clamped at 0, quantised the same way; -1 where NaN"""
    Q64, D64 = np.asarray(Q, dtype=np.float64), np.asarray(D, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (Q64 * Q64).sum(1)[:, None] + (D64 * D64).sum(1)[None, :] - 2.0 * (Q64 @ D64.T)
        v = np.minimum(np.maximum(x, 0.0), 16.0) * 16384.0
    return np.where(np.isnan(x), -1, np.rint(np.where(np.isnan(v), 0.0, v))).astype(np.int32)


def blocks_from_matrix(M, cand, h):
    """[nq, K, 32, 32] int32 from the matrix M [nq, nd] of quantised distances: entry [t + h][b'] = M[i + t][j - 15 + b'] for t = -h .. h
    and b' = 0 .. 30; -1 where a row is outside its table, in the other rows, in row and column 31, and for a skipped candidate"""
    nq, nd = M.shape
    cand = np.asarray(cand)
    K = cand.shape[1]
    out = np.full((nq, K, TILE, TILE), -1, dtype=np.int32)
    live = (cand >= 0) & (cand < nd)
    a = np.arange(nq)[:, None] + np.arange(-h, h + 1)[None, :]                      # [nq, L]
    b = np.where(live, cand, 0)[:, :, None] - BAND + np.arange(2 * BAND + 1)[None, None, :]      # [nq, K, 31]
    ok = ((a >= 0) & (a < nq))[:, None, :, None] & ((b >= 0) & (b < nd))[:, :, None, :] & live[:, :, None, None]
    vals = M[np.clip(a, 0, nq - 1)[:, None, :, None], np.clip(b, 0, nd - 1)[:, :, None, :]]
    out[:, :, :2 * h + 1, :2 * BAND + 1] = np.where(ok, vals, -1)
    return out


def blocks_f64(Q, D, cand, h):
    return blocks_from_matrix(dq_matrix_f64(Q, D), cand, h)


# ---- the stage ------------------------------------------------------------------------------------------------------------------------
def _offsets(off, rows):
    return np.array([0, rows], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)


def match(block, cand, steps, S, min_terms, nd, q_off=None, d_off=None, chunk=1 << 22):
    """-> (best [nq, K, 4] int32, order [nq, K] int32) from the blocks [nq, K, 32, 32].  The mean sum / n is compared as a float64
    quotient: sum < 2^23 and n <= 31, so two different means differ by at least 1 / 961 while a quotient is off by 2^-30 at most,
    and two equal means are the same real number and round to the same float64 -- the order is exactly lpd_seq_better's."""
    cand = np.asarray(cand, dtype=np.int64)
    steps = np.asarray(steps, dtype=np.int64)
    nq, K = cand.shape
    V, L = steps.shape
    h = (L - 1) // 2
    W = 2 * S + 1
    E = V * W
    q_off, d_off = _offsets(q_off, nq), _offsets(d_off, nd)
    e = np.arange(E)
    st = steps[hyp_v(e, S)]                                   # [E, L]
    s = hyp_s(e, S)                                           # [E]
    t = np.arange(-h, h + 1)
    best = np.zeros((nq, K, 4), dtype=np.int32)
    order = np.zeros((nq, K), dtype=np.int32)
    per = max(1, chunk // (K * E * L))
    for i0 in range(0, nq, per):
        i = np.arange(i0, min(i0 + per, nq))
        c = cand[i]
        live = (c >= 0) & (c < nd)
        j = np.where(live, c, 0)
        qr, dr = run_of(q_off, i), run_of(d_off, j)
        qlo, qhi, dlo, dhi = q_off[qr], q_off[qr + 1], d_off[dr], d_off[dr + 1]
        c0 = j[:, :, None] + s[None, None, :]                                                        # [n, K, E]
        centre = live[:, :, None] & (c0 >= dlo[:, :, None]) & (c0 < dhi[:, :, None])
        b = c0[..., None] + st[None, None]                                                           # [n, K, E, L]
        bp = b - j[:, :, None, None] + BAND
        a = i[:, None, None, None] + t[None, None, None, :]
        dq = block[i[:, None, None, None], np.arange(K)[None, :, None, None], (t + h)[None, None, None, :], np.clip(bp, 0, TILE - 1)].astype(np.int64)
        cnt = ((bp >= 0) & (bp <= 2 * BAND) & (a >= qlo[:, None, None, None]) & (a < qhi[:, None, None, None]) & (b >= dlo[:, :, None, None])
               & (b < dhi[:, :, None, None]) & (dq >= 0))
        total, n = (dq * cnt).sum(-1), cnt.sum(-1)
        valid = centre & (n >= min_terms)
        mean = np.where(valid, total / np.maximum(n, 1), np.inf)
        we = mean.argmin(-1)                                                                         # the first minimum: the lower e
        ok = np.take_along_axis(valid, we[..., None], -1)[..., 0]
        ws, wn = np.take_along_axis(total, we[..., None], -1)[..., 0], np.take_along_axis(n, we[..., None], -1)[..., 0]
        best[i, :, 0] = np.where(ok, we, -1)
        best[i, :, 1] = np.where(ok, ws, 0)
        best[i, :, 2] = np.where(ok, wn, 0)
        best[i, :, 3] = np.where(ok, j + s[we], -1)
        order[i] = np.argsort(np.where(ok, ws / np.maximum(wn, 1), np.inf), axis=1, kind="stable")
    return best, order


def match_slow(block, cand, steps, S, min_terms, nd, q_off=None, d_off=None):
    """the same, as the definition reads: loops and the integer comparator"""
    cand = np.asarray(cand)
    nq, K = cand.shape
    V, L = np.asarray(steps).shape
    h = (L - 1) // 2
    q_off, d_off = _offsets(q_off, nq), _offsets(d_off, nd)
    best = np.zeros((nq, K, 4), dtype=np.int32)
    order = np.zeros((nq, K), dtype=np.int32)
    for i in range(nq):
        m = int(run_of(q_off, i))
        qlo, qhi = int(q_off[m]), int(q_off[m + 1])
        for r in range(K):
            j = int(cand[i, r])
            w = (0, 0, -1)
            if 0 <= j < nd:
                m = int(run_of(d_off, j))
                dlo, dhi = int(d_off[m]), int(d_off[m + 1])
                for e in range(V * (2 * S + 1)):
                    v, s = hyp_v(e, S), hyp_s(e, S)
                    if not dlo <= j + s < dhi:
                        continue
                    total, n = hypothesis(block[i, r], steps[v], h, s, i, qlo, qhi, j, dlo, dhi)
                    if n >= min_terms and better(total, n, e, *w):
                        w = (total, n, e)
            best[i, r] = (-1, 0, 0, -1) if w[2] < 0 else (w[2], w[0], w[1], j + hyp_s(w[2], S))
        for r in range(K):
            me = best[i, r]
            before = 0
            for o in range(K):
                ot = best[i, o]
                if me[0] >= 0:
                    before += better(ot[1], ot[2], -1 if ot[0] < 0 else o, me[1], me[2], r)
                else:
                    before += bool(ot[0] >= 0 or o < r)
            order[i, before] = r
    return best, order


def chain(best, order, velocities, S, max_mean=None):
    """lpdnet_hip/sequence.py's fields from (best, order) -> dict of numpy arrays"""
    e, total, n, row = (best[..., c] for c in range(4))
    valid = e >= 0
    W = 2 * S + 1
    ec = np.maximum(e, 0)
    out = dict(hypothesis=e, valid=valid, row=row, sum=total, terms=n, order=order.astype(np.int64),
               velocity=np.where(valid, np.asarray(velocities, dtype=np.float64)[ec // W], 0.0), shift=np.where(valid, ec % W - S, 0),
               mean=np.where(valid, total / np.maximum(n, 1) / 16384.0, np.inf))
    out["accepted"] = None if max_mean is None else valid & (total.astype(np.int64) <= int(np.rint(max_mean * 16384.0)) * n.astype(np.int64))
    out["topk"] = np.take_along_axis(row, order.astype(np.int64), 1)
    return out


def self_candidates(idx, off, k, exclude):
    """idx [n, kk] = the retrieval of a table against itself -> [n, k] int32: rows of the same run within `exclude` dropped, the
    others in retrieval order, padded with -1"""
    n, kk = idx.shape
    off = _offsets(off, n)
    run = run_of(off, np.arange(n))
    out = np.full((n, k), -1, dtype=np.int32)
    for i in range(n):
        keep = [int(j) for j in idx[i] if j >= 0 and not (run[j] == run[i] and abs(int(j) - i) <= exclude)]
        out[i, :min(k, len(keep))] = keep[:k]
    return out


# ---- the synthetic drives of the quality figures --------------------------------------------------------------------------------------
QUALITY_RUNS = ((1.0, 20), (0.5, 100), (2.0, 60), (-1.0, 200))      # (velocity, first database row) of the four query runs of 40 rows


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def quality_drive(seed, noise, nd=240, dim=256, rows=40):
    """-> (Q [160, dim] fp32, D [nd, dim] fp32, truth [160] float64 database position of every query, q_off).  place[i] = the sum of
    four consecutive rows of a standard-normal base / 2 (neighbouring places share three quarters of their latent), D = unit(place +
    noise N(0, 1)); the queries walk the database at QUALITY_RUNS' velocities, their latents linearly interpolated, the same noise"""
    g = np.random.default_rng(seed)
    base = g.standard_normal((nd + 4, dim))
    place = (base[0:nd + 1] + base[1:nd + 2] + base[2:nd + 3] + base[3:nd + 4]) / 2.0      # nd + 1 places: one more, for the interpolation
    D = _unit(place[:nd] + noise * g.standard_normal((nd, dim)))
    truth = np.concatenate([start + vel * np.arange(rows) for vel, start in QUALITY_RUNS])
    lo = np.floor(truth).astype(int)
    f = (truth - lo)[:, None]
    lat = (1.0 - f) * place[lo] + f * place[lo + 1]
    Q = _unit(lat + noise * g.standard_normal(lat.shape))
    q_off = np.arange(0, len(truth) + 1, rows, dtype=np.int32)
    return Q.astype(f32), D.astype(f32), truth, q_off


def topk_f64(Q, D, k):
    """[nq, k] int32: the k nearest rows by float64 squared distance, ties to the lower row"""
    Q64, D64 = np.asarray(Q, dtype=np.float64), np.asarray(D, dtype=np.float64)
    d = (Q64 * Q64).sum(1)[:, None] + (D64 * D64).sum(1)[None, :] - 2.0 * (Q64 @ D64.T)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


def quality(cand, best, order, truth, tol=2.0):
    """-> (single-frame top-1, best sequence candidate, after the shift): the shares of queries whose row lies within tol of the truth"""
    n = np.arange(len(truth))
    first = order[:, 0]
    single = np.abs(cand[:, 0] - truth) <= tol
    seq = np.abs(cand[n, first] - truth) <= tol
    moved = (best[n, first, 0] >= 0) & (np.abs(best[n, first, 3] - truth) <= tol)
    return float(single.mean()), float(seq.mean()), float(moved.mean())
