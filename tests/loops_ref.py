"""numpy restatement of csrc/lpd_loops_math.h and of both kernels of csrc/lpd_loops.hip (lpd_loop_consistency, lpd_loop_select), in the
header's order of operations: float64 throughout, one rounding an operation.  Functions take arrays with a leading batch axis.  The
tests compare them with the header compiled by the host compiler value for value, and with the kernels bit for bit.  Also here: bit-row
helpers, an exact maximum clique (Bron-Kerbosch with pivoting) to measure the greedy selection against, and the quality cases on
pgo_ref.two_laps."""
import functools

import numpy as np

import pgo_ref as R

KEY_BITS = 12
MAX_LOOPS = 1 << KEY_BITS
MAX_SEEDS = 64
OK, NOTHING, TOO_FEW, TOO_MANY = 0, 1, 2, 3
f64 = np.float64
u64 = np.uint64


# ---- the header, function for function ------------------------------------------------------------------------------------------------
def valid(edge, V, meas, weight):
    """edge [n, 2] local, V [n] or a number -> [n] bool"""
    with np.errstate(invalid="ignore"):
        return R.edge_ok(edge, V, meas, weight) & (weight[:, 0] > 0.0) & (weight[:, 1] > 0.0)


def mul(A, B):
    """A, B [n, 12] -> A B [n, 12]"""
    out = np.empty_like(A)
    for r in range(3):
        a0, a1, a2 = A[:, 4 * r], A[:, 4 * r + 1], A[:, 4 * r + 2]
        for c in range(3):
            out[:, 4 * r + c] = R.dot3(a0, a1, a2, B[:, c], B[:, 4 + c], B[:, 8 + c])
        out[:, 4 * r + 3] = R.dot3(a0, a1, a2, B[:, 3], B[:, 7], B[:, 11]) + A[:, 4 * r + 3]
    return out


def between(X, Y):
    """X^-1 Y as poses [n, 12]"""
    Rm, t = R.between(X, Y)
    out = np.empty_like(X)
    for r in range(3):
        out[:, 4 * r:4 * r + 3] = Rm[:, 3 * r:3 * r + 3]
        out[:, 4 * r + 3] = t[:, r]
    return out


def chord2(X, Y):
    d0, d1, d2 = X[:, 3] - Y[:, 3], X[:, 7] - Y[:, 7], X[:, 11] - Y[:, 11]
    return R.dot3(d0, d1, d2, d0, d1, d2)


def cycle(Xia, Xja, Za, Xib, Xjb, Zb):
    """-> E [n, 12], the cycle through loop a (the lower number) and loop b"""
    with np.errstate(all="ignore"):
        T1 = between(Xja, Xjb)
        M1 = mul(Za, T1)
        Ab = mul(Xib, Zb)
        T2 = between(Ab, Xia)
        return mul(M1, T2)


def residual(Xia, Xja, Za, Xib, Xjb, Zb):
    """-> r [n, 6]"""
    E = cycle(Xia, Xja, Za, Xib, Xjb, Zb)
    r = np.empty((E.shape[0], 6))
    with np.errstate(all="ignore"):
        r[:, :3] = R.rot_residual(E[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])
    r[:, 3:] = E[:, [3, 7, 11]]
    return r


def stat(Xia, Xja, Za, wa, ia, ja, Xib, Xjb, Zb, wb, ib, jb, w_or, w_ot):
    with np.errstate(all="ignore"):
        r = residual(Xia, Xja, Za, Xib, Xjb, Zb)
        ni, nj = np.abs(ia.astype(np.int64) - ib).astype(f64), np.abs(ja.astype(np.int64) - jb).astype(f64)
        nn = ni + nj
        ci2, cj2 = chord2(Xia, Xib), chord2(Xja, Xjb)
        var_r = ((1.0 / wa[:, 0]) + (1.0 / wb[:, 0])) + (nn / w_or)
        var_t = (((1.0 / wa[:, 1]) + (1.0 / wb[:, 1])) + (nn / w_ot)) + (((ni * ci2) + (nj * cj2)) / w_or)
        rr = R.dot3(r[:, 0], r[:, 1], r[:, 2], r[:, 0], r[:, 1], r[:, 2])
        tt = R.dot3(r[:, 3], r[:, 4], r[:, 5], r[:, 3], r[:, 4], r[:, 5])
        return (rr / var_r) + (tt / var_t)


def consistent(s, gate):
    with np.errstate(invalid="ignore"):
        return s <= gate


def key(count, u):
    return (count << KEY_BITS) | ((MAX_LOOPS - 1) - u)


def key_loop(k):
    return (MAX_LOOPS - 1) - (k & (MAX_LOOPS - 1))


def word_mask(w, P):
    left = P - 64 * w
    return u64(0xFFFFFFFFFFFFFFFF) if left >= 64 else (u64(0) if left <= 0 else u64((1 << left) - 1))


# ---- bit rows ----------------------------------------------------------------------------------------------------------------------
def pack(M, ldw=None):
    """bool [P, Q] -> uint64 [P, ldw]: bit q & 63 of word q >> 6"""
    M = np.asarray(M, dtype=bool)
    P, Q = M.shape
    nw = -(-Q // 64) if Q else 0
    ldw = max(nw, 1) if ldw is None else ldw
    pad = np.zeros((P, 64 * ldw), dtype=bool)
    pad[:, :Q] = M
    by = np.packbits(pad, axis=1, bitorder="little")      # byte k of a word = its bits 8 k .. 8 k + 7
    return np.ascontiguousarray(by).view("<u8").reshape(P, ldw)


def unpack(adj, Q):
    """uint64 [P, ldw] -> bool [P, Q]"""
    adj = np.ascontiguousarray(adj, dtype="<u8")
    by = adj.view(np.uint8).reshape(adj.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :Q].astype(bool)


def popcount(a):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).astype(np.int64)
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=(-1, -2)).astype(np.int64)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def _graphs(off, total):
    off = [int(v) for v in off]
    return [(off[g], off[g + 1], off[g] >= 0 and off[g + 1] >= off[g] and off[g + 1] <= total) for g in range(len(off) - 1)]


def _row_graph(off, G, r):
    """lc_graph of the kernel"""
    if not off[0] <= r:
        return -1
    lo, hi = 0, G
    for _ in range(17):
        if not lo + 1 < hi:
            break
        mid = (lo + hi) >> 1
        if off[mid] <= r:
            lo = mid
        else:
            hi = mid
    return lo


def consistency(pose, edge, meas, weight, w_or, w_ot, gate, node_off=None, loop_off=None, ldw=None, stats=False):
    """lpd_loop_consistency -> (adj [P, ldw] uint64, degree [P] int32); stats=True adds the dense statistic [P, P] (NaN where none)"""
    pose = np.ascontiguousarray(pose, dtype=f64).reshape(-1, 12)
    edge = np.ascontiguousarray(edge, dtype=np.int32).reshape(-1, 2)
    meas = np.ascontiguousarray(meas, dtype=f64).reshape(-1, 12)
    weight = np.ascontiguousarray(weight, dtype=f64).reshape(-1, 2)
    Vt, Pt = pose.shape[0], edge.shape[0]
    node_off = [0, Vt] if node_off is None else [int(v) for v in node_off]
    loop_off = [0, Pt] if loop_off is None else [int(v) for v in loop_off]
    G = len(loop_off) - 1
    if ldw is None:
        ldw = max(1, max(-(-(b - a) // 64) for a, b in zip(loop_off, loop_off[1:])))
    adj = np.zeros((Pt, ldw), dtype=u64)
    degree = np.full(Pt, -1, dtype=np.int32)
    S = np.full((Pt, Pt), np.nan) if stats else None
    rows_of = {}
    for r in range(Pt):      # which graph a row belongs to, as the kernel finds it
        g = _row_graph(loop_off, G, r)
        if g >= 0:
            rows_of.setdefault(g, []).append(r)
    for g, rows in rows_of.items():
        p0, p1, n0, n1 = loop_off[g], loop_off[g + 1], node_off[g], node_off[g + 1]
        P, V = p1 - p0, n1 - n0
        rows = [r for r in rows if p0 <= r < p1]
        if not (p0 >= 0 and p1 <= Pt and P <= 64 * ldw and P <= MAX_LOOPS and n0 >= 0 and n1 >= n0 and n1 <= Vt) or not rows:
            continue
        e, Z, w = edge[p0:p1], meas[p0:p1], weight[p0:p1]
        ok = valid(e, V, Z, w)
        ok &= np.isin(np.arange(P) + p0, rows)
        vi = np.flatnonzero(ok)
        M = np.zeros((P, P), dtype=bool)
        if len(vi) > 1:
            ka, kb = np.triu_indices(len(vi), 1)
            a, b = vi[ka], vi[kb]
            X = pose[n0:n1]
            s = np.empty(len(a))
            for c0 in range(0, len(a), 1 << 19):      # in pieces: the temporaries of 8 million pairs at once are gigabytes
                ac, bc = a[c0:c0 + (1 << 19)], b[c0:c0 + (1 << 19)]
                s[c0:c0 + (1 << 19)] = stat(X[e[ac, 0]], X[e[ac, 1]], Z[ac], w[ac], e[ac, 0], e[ac, 1], X[e[bc, 0]], X[e[bc, 1]], Z[bc], w[bc], e[bc, 0],
                                            e[bc, 1], f64(w_or), f64(w_ot))
            c = consistent(s, f64(gate))
            M[a, b] = c
            M[b, a] = c
            if stats:
                S[p0 + a, p0 + b] = s
                S[p0 + b, p0 + a] = s
        adj[p0:p1] = pack(M, ldw)
        degree[p0 + vi] = M[vi].sum(axis=1)
    return (adj, degree, S) if stats else (adj, degree)


def _grow(A, P, nw, valid_row, seed):
    """one workgroup of loop_grow_kernel -> (chosen bit row [nw], size)"""
    one = u64(1)
    mask = np.array([word_mask(w, P) for w in range(nw)], dtype=u64)
    self_bit = np.zeros(nw, dtype=u64)
    self_bit[seed >> 6] = one << u64(seed & 63)
    cand = A[seed, :nw] & valid_row & mask & ~self_bit
    chosen = self_bit.copy()
    size = 1
    for _ in range(P):
        members = np.flatnonzero(unpack(cand[None, :], P)[0])
        if len(members) == 0:
            break
        cnt = popcount(A[members, :nw] & cand[None, :]).sum(axis=1)
        keys = key(cnt, members)
        u = int(key_loop(int(keys.max())))
        bit = np.zeros(nw, dtype=u64)
        bit[u >> 6] = one << u64(u & 63)
        cand = cand & A[u, :nw] & ~bit
        chosen |= bit
        size += 1
    return chosen, size


def select(adj, degree, loop_off=None, seeds=8, min_size=3):
    """lpd_loop_select -> (accepted [P] uint8, info [G, 8] int32).  Rows of no graph keep 0."""
    adj = np.ascontiguousarray(adj, dtype=u64)
    degree = np.ascontiguousarray(degree, dtype=np.int32)
    Pt, ldw = adj.shape
    loop_off = [0, Pt] if loop_off is None else [int(v) for v in loop_off]
    G = len(loop_off) - 1
    accepted = np.zeros(Pt, dtype=np.uint8)
    info = np.zeros((G, 8), dtype=np.int32)
    for g, (p0, p1, sane) in enumerate(_graphs(loop_off, Pt)):
        P = p1 - p0
        too_many = sane and (P > 64 * ldw or P > MAX_LOOPS)
        if not sane or too_many:
            info[g] = (TOO_MANY if too_many else NOTHING, 0, 0, 0, -1, 0, 0, 0)
            continue
        d = np.minimum(degree[p0:p1], MAX_LOOPS - 1).astype(np.int64)
        ok = d >= 0
        nvalid, dsum = int(ok.sum()), int(d[d > 0].sum())
        nw = -(-P // 64)
        sizes, rows, seed_of = [], [], []
        if nvalid:
            keys = np.sort(key(d[ok], np.flatnonzero(ok)))[::-1]
            valid_row = pack(ok[None, :], nw)[0]
            A = adj[p0:p1]
            for s in range(min(seeds, nvalid)):
                seed = int(key_loop(int(keys[s])))
                chosen, size = _grow(A, P, nw, valid_row, seed)
                sizes.append(size), rows.append(chosen), seed_of.append(seed)
        best, best_s = 0, -1
        for s, sz in enumerate(sizes):
            if sz > best:
                best, best_s = sz, s
        status = NOTHING if best_s < 0 else (TOO_FEW if best < min_size else OK)
        if status == OK:
            accepted[p0:p1] = unpack(rows[best_s][None, :], P)[0]
        info[g] = (status, nvalid, best if status == OK else 0, len(sizes), -1 if best_s < 0 else seed_of[best_s], dsum // 2, 0, 0)
    return accepted, info


# ---- an exact maximum clique, to measure the greedy sets against -------------------------------------------------------------------------
def max_clique(M):
    """bool [P, P] symmetric, zero diagonal -> a maximum clique (sorted list) by Bron-Kerbosch with pivoting on Python integers"""
    P = M.shape[0]
    nb = [int.from_bytes(np.packbits(M[u], bitorder="little").tobytes(), "little") for u in range(P)]
    best = []

    def expand(Rs, Pm, Xm):
        nonlocal best
        if Pm == 0:
            if Xm == 0 and len(Rs) > len(best):
                best = list(Rs)
            return
        if len(Rs) + bin(Pm).count("1") <= len(best):
            return
        PX = Pm | Xm
        pivot = max((u for u in range(P) if PX >> u & 1), key=lambda u: bin(nb[u] & Pm).count("1"))
        todo = Pm & ~nb[pivot]
        while todo:
            u = (todo & -todo).bit_length() - 1
            expand(Rs + [u], Pm & nb[u], Xm & nb[u])
            Pm &= ~(1 << u)
            Xm |= 1 << u
            todo &= ~(1 << u)

    expand([], (1 << P) - 1 if P else 0, 0)
    return sorted(best)


def is_maximal(M, chosen, ok):
    """no valid loop outside `chosen` (bool [P]) is consistent with all of it"""
    inside = np.flatnonzero(chosen)
    return not any(M[u, inside].all() for u in np.flatnonzero(ok & ~chosen))


# ---- the quality cases: pgo_ref.two_laps with gross loops ----------------------------------------------------------------------------------
QUALITY_CASES = ((1, 64, 1, 0.3), (2, 64, 1, 0.3), (3, 64, 2, 0.3), (5, 64, 4, 0.4), (4, 128, 1, 0.4))      # seed, V, loops_every, outliers
GATE, SEEDS, MIN_SIZE = 16.81, 8, 3


def case_inputs(seed, V, loops_every, outliers):
    """-> (graph, loops = (edge, meas, weight) of the loop edges, (w_or, w_ot) as two_laps gives them)"""
    g = R.two_laps(seed, V, loops_every=loops_every, outliers=outliers)
    lp = g["is_loop"]
    w_od = g["weight"][~lp][0]
    return g, (g["edge"][lp], g["meas"][lp], g["weight"][lp]), (float(w_od[0]), float(w_od[1]))


def solve_with(g, keep, huber=0.0):
    """the restatement's solve of the graph with the loops `keep` (bool over the loop edges) -> ATE"""
    use = ~g["is_loop"]
    use[np.flatnonzero(g["is_loop"])[keep]] = True
    pose = R.solve(g["start"], g["edge"][use], g["meas"][use], g["weight"][use], huber=huber, **R.QUALITY_SOLVER)[0]
    return R.ate(pose, g["gt"])


@functools.lru_cache(maxsize=None)
def quality_case(seed, V, loops_every, outliers):
    """a case's restated selection and the four trajectories' errors, made once a process"""
    g, (edge, meas, weight), (w_or, w_ot) = case_inputs(seed, V, loops_every, outliers)
    adj, degree = consistency(g["start"], edge, meas, weight, w_or, w_ot, GATE)
    accepted, info = select(adj, degree, seeds=SEEDS, min_size=MIN_SIZE)
    gross = g["is_outlier"][g["is_loop"]]
    P = len(edge)
    return dict(graph=g, loops=(edge, meas, weight), w=(w_or, w_ot), adj=adj, degree=degree, accepted=accepted, info=info, gross=gross,
                M=unpack(adj, P), ate_start=R.ate(g["start"], g["gt"]), ate_all_huber=solve_with(g, np.ones(P, dtype=bool), huber=3.0),
                ate_true=solve_with(g, ~gross), ate_chosen=solve_with(g, accepted.astype(bool)))


# ---- synthetic loops at any size ---------------------------------------------------------------------------------------------------------
def drive_loops(seed, V, P, gross=0.3):
    """A noisy chain of V nodes (the start = its odometry integrated) and P loops between random pairs of its nodes, measured with a
    little noise, a share `gross` of them grossly wrong -> (start [V, 12], edge [P, 2] int32, meas [P, 12], weight [P, 2], (w_or, w_ot))"""
    g = np.random.default_rng(seed)
    drift, noise = (0.004, 0.05), (0.003, 0.07)
    gt, start = [R.pose12(np.eye(3), [0.0, 0.0, 0.0])], [R.pose12(np.eye(3), [0.0, 0.0, 0.0])]
    for _ in range(V - 1):
        step = R.pose12(R.rot_of(g.normal(0, 0.15, 3)), [3.0 + g.normal(0, 0.3), g.normal(0, 0.3), g.normal(0, 0.1)])
        gt.append(R.mul12(gt[-1], step))
        start.append(R.mul12(start[-1], R.mul12(step, R.pose12(R.rot_of(g.normal(0, drift[0], 3)), g.normal(0, drift[1], 3)))))
    edge = np.empty((P, 2), dtype=np.int32)
    meas = np.empty((P, 12))
    for p in range(P):
        i, j = (int(v) for v in g.choice(V, 2, replace=False)) if V > 1 else (0, 0)
        Z = R.mul12(R.mul12(R.inv12(gt[i]), gt[j]), R.pose12(R.rot_of(g.normal(0, noise[0], 3)), g.normal(0, noise[1], 3)))
        if g.random() < gross:
            Z = R.mul12(Z, R.pose12(R.yaw_rot(g.uniform(0.5, 3.0)), g.uniform(2.0, 15.0, 3) * g.choice([-1.0, 1.0], 3)))
        edge[p], meas[p] = (i, j), Z
    weight = np.array([[1.0 / noise[0] ** 2, 1.0 / noise[1] ** 2]]) * g.uniform(0.5, 2.0, (P, 1))
    return np.array(start), edge, meas, np.ascontiguousarray(weight), (1.0 / drift[0] ** 2, 1.0 / drift[1] ** 2)


@functools.lru_cache(maxsize=None)
def random_matrix(seed, P, density):
    """a seeded symmetric bit matrix with a zero diagonal -> (adj [P, ceil(P / 64)] uint64, degree [P] int32)"""
    g = np.random.default_rng(seed)
    M = np.triu(g.random((P, P)) < density, 1)
    M = M | M.T
    return pack(M), M.sum(axis=1).astype(np.int32)
