"""numpy restatement of csrc/lpd_pgo_math.h and of the whole of lpd_pgo_solve (csrc/lpd_pgo.hip), in the kernel's order of operations:
float64 throughout, one rounding an operation, a node's sum in CSR order, every dot product as 256 strided partials and a fixed tree.
Functions take arrays with a leading batch axis, so that a phase of the kernel is a handful of numpy operations; the tests compare them
with the header compiled by the host compiler value for value, and with the kernel bit for bit.  Also here: the synthetic graphs of the
tests, and the independent reference (scipy.optimize.least_squares on the same cost from the same start)."""
import functools

import numpy as np

THREADS = 256
FTOL = 1e-12
XTOL = 1e-12
LAMBDA_MIN = 1e-9
DBL_MAX = np.finfo(np.float64).max
CONVERGED, ITERATIONS, NOTHING, REFUSED = 0, 1, 2, 3
DIAG = (0, 6, 11, 15, 18, 20)
f64 = np.float64


def finite(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v) <= DBL_MAX      # false for NaN


# ---- the header, function for function ------------------------------------------------------------------------------------------------
def dot3(a0, a1, a2, b0, b1, b2):
    return ((a0 * b0) + (a1 * b1)) + (a2 * b2)


def dot6(a, b):
    return (((((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])) + (a[..., 3] * b[..., 3])) + (a[..., 4] * b[..., 4])) + (a[..., 5] * b[..., 5])


def edge_ok(edge, V, meas, weight):
    """edge [n, 2] local, V [n] or a number -> [n] bool"""
    i, j = edge[:, 0], edge[:, 1]
    ok = (i >= 0) & (i < V) & (j >= 0) & (j < V) & (i != j)
    with np.errstate(invalid="ignore"):
        return ok & finite(meas).all(axis=1) & finite(weight).all(axis=1) & (weight[:, 0] >= 0.0) & (weight[:, 1] >= 0.0)


def between(X, Y):
    """X, Y [n, 12] -> (R [n, 9], t [n, 3]) of X^-1 Y"""
    d0, d1, d2 = Y[:, 3] - X[:, 3], Y[:, 7] - X[:, 7], Y[:, 11] - X[:, 11]
    R = np.empty((X.shape[0], 9))
    t = np.empty((X.shape[0], 3))
    for r in range(3):
        for c in range(3):
            R[:, 3 * r + c] = dot3(X[:, r], X[:, 4 + r], X[:, 8 + r], Y[:, c], Y[:, 4 + c], Y[:, 8 + c])
        t[:, r] = dot3(X[:, r], X[:, 4 + r], X[:, 8 + r], d0, d1, d2)
    return R, t


def quat(R):
    """R [n, 9] -> (q [n, 4] = (w, x, y, z), branch [n])"""
    R = np.asarray(R, dtype=f64)
    tr = (R[:, 0] + R[:, 4]) + R[:, 8]
    c = np.stack((tr, R[:, 0], R[:, 4], R[:, 8]), axis=1)
    m = np.zeros(R.shape[0], dtype=np.int64)
    best = c[:, 0].copy()
    with np.errstate(all="ignore"):
        for a in range(1, 4):
            win = c[:, a] > best
            best = np.where(win, c[:, a], best)
            m = np.where(win, a, m)
        s0 = np.sqrt(1.0 + tr) * 2.0
        s1 = np.sqrt(((1.0 + R[:, 0]) - R[:, 4]) - R[:, 8]) * 2.0
        s2 = np.sqrt(((1.0 + R[:, 4]) - R[:, 0]) - R[:, 8]) * 2.0
        s3 = np.sqrt(((1.0 + R[:, 8]) - R[:, 0]) - R[:, 4]) * 2.0
        q0 = np.stack((s0 * 0.25, (R[:, 7] - R[:, 5]) / s0, (R[:, 2] - R[:, 6]) / s0, (R[:, 3] - R[:, 1]) / s0), axis=1)
        q1 = np.stack(((R[:, 7] - R[:, 5]) / s1, s1 * 0.25, (R[:, 1] + R[:, 3]) / s1, (R[:, 2] + R[:, 6]) / s1), axis=1)
        q2 = np.stack(((R[:, 2] - R[:, 6]) / s2, (R[:, 1] + R[:, 3]) / s2, s2 * 0.25, (R[:, 5] + R[:, 7]) / s2), axis=1)
        q3 = np.stack(((R[:, 3] - R[:, 1]) / s3, (R[:, 2] + R[:, 6]) / s3, (R[:, 5] + R[:, 7]) / s3, s3 * 0.25), axis=1)
    q = np.where((m == 0)[:, None], q0, np.where((m == 1)[:, None], q1, np.where((m == 2)[:, None], q2, q3)))
    return q, m


def rot_residual(R):
    q, _ = quat(R)
    with np.errstate(invalid="ignore"):
        neg = q[:, 0] < 0.0
    v = 2.0 * q[:, 1:]
    return np.where(neg[:, None], -v, v)


def edge_lin(Xi, Xj, Z):
    """-> (jc [n, 36] = (A, B, C, Re), r [n, 6])"""
    n = Xi.shape[0]
    RT, tT = between(Xi, Xj)
    Tp = np.stack((RT[:, 0], RT[:, 1], RT[:, 2], tT[:, 0], RT[:, 3], RT[:, 4], RT[:, 5], tT[:, 1], RT[:, 6], RT[:, 7], RT[:, 8], tT[:, 2]), axis=1)
    Re, te = between(Z, Tp)
    jc = np.empty((n, 36))
    r = np.empty((n, 6))
    jc[:, 27:] = Re
    r[:, 3:] = te
    r[:, :3] = rot_residual(Re)
    for a in range(3):
        for b in range(3):
            jc[:, 3 * a + b] = RT[:, 3 * b + a]
            jc[:, 18 + 3 * a + b] = Z[:, 4 * b + a]
    for a in range(3):
        c0, c1, c2 = jc[:, 18 + 3 * a], jc[:, 19 + 3 * a], jc[:, 20 + 3 * a]
        jc[:, 9 + 3 * a] = (c1 * tT[:, 2]) - (c2 * tT[:, 1])
        jc[:, 10 + 3 * a] = (c2 * tT[:, 0]) - (c0 * tT[:, 2])
        jc[:, 11 + 3 * a] = (c0 * tT[:, 1]) - (c1 * tT[:, 0])
    return jc, r


def residual(Xi, Xj, Z):
    return edge_lin(Xi, Xj, Z)[1]


def chi2(r, w):
    return (w[:, 0] * dot3(r[:, 0], r[:, 1], r[:, 2], r[:, 0], r[:, 1], r[:, 2])) + (w[:, 1] * dot3(r[:, 3], r[:, 4], r[:, 5], r[:, 3], r[:, 4], r[:, 5]))


def rho(s, huber):
    if not huber > 0.0:
        return s
    with np.errstate(invalid="ignore"):
        a = np.sqrt(s)
        return np.where(a > huber, ((2.0 * huber) * a) - (huber * huber), s)


def irls(s, huber):
    if not huber > 0.0:
        return np.ones_like(s)
    with np.errstate(all="ignore"):
        a = np.sqrt(s)
        return np.where(a > huber, huber / a, 1.0)


def jac(jc, end):
    """jc [n, 36], end [n] (0 or 1) or a number -> J [n, 36]"""
    n = jc.shape[0]
    J0 = np.zeros((n, 36))
    J1 = np.zeros((n, 36))
    for a in range(3):
        for b in range(3):
            J0[:, 6 * a + b] = -jc[:, 3 * a + b]
            J0[:, 6 * (3 + a) + b] = jc[:, 9 + 3 * a + b]
            J0[:, 6 * (3 + a) + 3 + b] = -jc[:, 18 + 3 * a + b]
            J1[:, 6 * a + b] = 1.0 if a == b else 0.0
            J1[:, 6 * (3 + a) + 3 + b] = jc[:, 27 + 3 * a + b]
    end = np.broadcast_to(np.asarray(end), (n,))
    return np.where((end == 0)[:, None], J0, J1)


def _w6(w):
    return np.concatenate((np.repeat(w[:, :1], 3, axis=1), np.repeat(w[:, 1:], 3, axis=1)), axis=1)


def ju_dense(Ji, Jj, w, pi, pj):
    """s [n, 6] = W (Ji pi + Jj pj) from the dense Jacobians [n, 36]"""
    A, B = Ji.reshape(-1, 6, 6), Jj.reshape(-1, 6, 6)
    return _w6(w) * (dot6(A, pi[:, None, :]) + dot6(B, pj[:, None, :]))


def ju(jc, w, pi, pj):
    return ju_dense(jac(jc, 0), jac(jc, 1), w, pi, pj)


def wr(r, w):
    return _w6(w) * r


def jt(J, s):
    A = J.reshape(-1, 6, 6)
    return (((((A[:, 0, :] * s[:, 0:1]) + (A[:, 1, :] * s[:, 1:2])) + (A[:, 2, :] * s[:, 2:3])) + (A[:, 3, :] * s[:, 3:4])) + (A[:, 4, :] * s[:, 4:5])) + (A[:, 5, :] * s[:, 5:6])


def jtwj(J, w):
    A = J.reshape(-1, 6, 6)
    w6 = _w6(w)
    blk = np.empty((J.shape[0], 21))
    e = 0
    for r in range(6):
        for c in range(r, 6):
            acc = (w6[:, 0] * A[:, 0, r]) * A[:, 0, c]
            for a in range(1, 6):
                acc = acc + ((w6[:, a] * A[:, a, r]) * A[:, a, c])
            blk[:, e] = acc
            e += 1
    return blk


def ldl6(A, g):
    """A [n, 6, 6] symmetric, g [n, 6] -> (x [n, 6], ok [n]); x of a refused row is meaningless"""
    n = A.shape[0]
    L = np.zeros((n, 6, 6))
    D, v, y, x = np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 6))
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[:, j, j].copy()
            for k in range(j):
                v[:, k] = L[:, j, k] * D[:, k]
                d = d - (L[:, j, k] * v[:, k])
            ok &= (d > 0.0) & finite(d)      # a row that failed earlier stays failed, as the early return does
            D[:, j] = d
            for i in range(j + 1, 6):
                s = A[:, i, j].copy()
                for k in range(j):
                    s = s - (L[:, i, k] * v[:, k])
                L[:, i, j] = s / d
        for i in range(6):
            s = g[:, i].copy()
            for k in range(i):
                s = s - (L[:, i, k] * y[:, k])
            y[:, i] = s
        for i in range(6):
            y[:, i] = y[:, i] / D[:, i]
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - (L[:, k, i] * x[:, k])
            x[:, i] = s
    return x, ok


def precond(D, lam, r):
    """D [n, 21], r [n, 6] -> (z [n, 6], ok [n])"""
    n = D.shape[0]
    A = np.empty((n, 6, 6))
    e = 0
    for a in range(6):
        for b in range(a, 6):
            A[:, a, b] = A[:, b, a] = D[:, e]
            e += 1
    with np.errstate(all="ignore"):
        for a in range(6):
            A[:, a, a] = A[:, a, a] + (lam * A[:, a, a])
    z, ok = ldl6(A, r)
    return z, ok & finite(z).all(axis=1)


def dR(x):
    """x [n, >= 3] -> [n, 3, 3]: lpd_icp_dR"""
    with np.errstate(all="ignore"):
        hx, hy, hz = x[:, 0] * 0.5, x[:, 1] * 0.5, x[:, 2] * 0.5
        ln = np.sqrt(((1.0 + (hx * hx)) + (hy * hy)) + (hz * hz))
        qw, qx, qy, qz = 1.0 / ln, hx / ln, hy / ln, hz / ln
        xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
        M = np.empty((x.shape[0], 3, 3))
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = 1.0 - (2.0 * (yy + zz)), 2.0 * (xy - wz), 2.0 * (xz + wy)
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = 2.0 * (xy + wz), 1.0 - (2.0 * (xx + zz)), 2.0 * (yz - wx)
        M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = 2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - (2.0 * (xx + yy))
    return M


def retract(pose, x):
    """pose [n, 12], x [n, 6] -> (out [n, 12], ok [n])"""
    M = dR(x)
    out = np.empty_like(pose)
    with np.errstate(all="ignore"):
        for i in range(3):
            r0, r1, r2 = pose[:, 4 * i], pose[:, 4 * i + 1], pose[:, 4 * i + 2]
            for j in range(3):
                out[:, 4 * i + j] = dot3(r0, r1, r2, M[:, 0, j], M[:, 1, j], M[:, 2, j])
            out[:, 4 * i + 3] = pose[:, 4 * i + 3] + dot3(r0, r1, r2, x[:, 3], x[:, 4], x[:, 5])
    return out, finite(x).all(axis=1) & finite(out).all(axis=1)


def accept(cost, trial):
    return bool(trial < cost)


def converged(cost, trial):
    return bool((cost - trial) <= FTOL * cost)


def small_step(xx):
    return bool(xx <= XTOL * XTOL)


def lambda_up(lam):
    l = lam * 10.0
    return l if l > LAMBDA_MIN else LAMBDA_MIN


def cg_continue(rz, rz0, cg_tol):
    return bool(rz > (cg_tol * cg_tol) * rz0)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def tree_sum(vals):
    """the sum of vals [n] as the workgroup takes it: thread t adds the entries t, t + 256, ... in ascending order to a partial that
    starts at 0, the partials meet in a binary tree.  (An entry a thread does not have is a +0.0 here: a partial is never -0.0, so
    adding it changes no bit.)"""
    vals = np.asarray(vals, dtype=f64)
    rows = -(-max(len(vals), 1) // THREADS)
    pad = np.zeros(rows * THREADS)
    pad[:len(vals)] = vals
    part = np.zeros(THREADS)
    with np.errstate(all="ignore"):
        for row in pad.reshape(rows, THREADS):
            part = part + row
        s = THREADS // 2
        while s > 0:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
    return f64(part[0])


def csr(edge, node_off, edge_off, V):
    """what ops.pgo_csr makes: (csr_ptr [V + 1], csr_idx [2 E]) -- the ends 2 e + end by a stable sort on their global node"""
    E = edge.shape[0]
    if E == 0:
        return np.zeros(V + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    G = len(node_off) - 1
    gid = np.minimum(np.searchsorted(np.asarray(edge_off[1:]), np.arange(E), side="right"), G - 1)
    off = np.asarray(node_off, dtype=np.int64)
    n0, n1 = off[gid], off[gid + 1]
    ends = edge.astype(np.int64)
    inside = (ends >= 0) & (ends < (n1 - n0)[:, None]) & (n0 >= 0)[:, None] & (n1 <= V)[:, None]
    key = np.where(inside, ends + n0[:, None], V).reshape(2 * E)
    order = np.argsort(key, kind="stable")
    ptr = np.searchsorted(key[order], np.arange(V + 1), side="left")
    return ptr.astype(np.int32), order.astype(np.int32)


class _Graph:
    """one graph's arrays in local numbering, and the lists its node phases walk"""

    def __init__(self, pose, fixed, edge, meas, weight, rows):
        self.pose, self.edge, self.meas, self.weight = pose, edge, meas, weight
        V = pose.shape[0]
        self.V, self.E = V, edge.shape[0]
        self.use = edge_ok(edge, V, meas, weight) if self.E else np.zeros(0, dtype=bool)
        fix = fixed != 0
        if not fix.any() and V:
            fix = fix.copy()
            fix[0] = True
        # rows: per node the (local edge, end) entries in CSR order, already filtered to this graph's edges
        en, ee, eend, rank = [], [], [], []
        for k, row in enumerate(rows):
            d = 0
            for e, end in row:
                if self.use[e] and edge[e, end] == k:
                    en.append(k), ee.append(e), eend.append(end), rank.append(d)
                    d += 1
        self.en, self.ee, self.eend, self.rank = (np.array(v, dtype=np.int64) for v in (en, ee, eend, rank))
        deg = np.bincount(self.en, minlength=V) if V else np.zeros(0, dtype=np.int64)
        self.free = ~fix & (deg > 0)
        self.maxdeg = int(deg.max()) if V and len(deg) else 0
        self.ue = np.flatnonzero(self.use)      # the used edges, ascending

    def gather(self, contrib, width):
        """the node sums of contrib [entries, width] in CSR order, from 0"""
        acc = np.zeros((self.V, width))
        with np.errstate(all="ignore"):
            for d in range(self.maxdeg):
                sel = self.rank == d
                acc[self.en[sel]] = acc[self.en[sel]] + contrib[sel]
        return acc

    def edge_vals(self, vals_used):
        """[E] with the used edges' values, 0 elsewhere (what tree_sum takes)"""
        out = np.zeros(self.E)
        out[self.ue] = vals_used
        return out

    def cost(self, P, huber):
        if len(self.ue) == 0:
            return f64(0.0), np.zeros(0)
        with np.errstate(all="ignore"):
            r = residual(P[self.edge[self.ue, 0]], P[self.edge[self.ue, 1]], self.meas[self.ue])
            c = chi2(r, self.weight[self.ue])
            return tree_sum(self.edge_vals(rho(c, huber))), c


def _solve_graph(g, outer, cg_iters, cg_tol, lambda0, huber):
    V, E = g.V, g.E
    pose = g.pose.copy()
    costs = np.zeros(outer + 1)
    used, nfree = int(g.use.sum()), int(g.free.sum())
    free = g.free
    cost, _ = g.cost(pose, huber)
    costs[0] = cost
    status, accepted, refused, cg_total = ITERATIONS, 0, 0, 0
    done, relin, lam = False, True, f64(lambda0)
    if used == 0 or nfree == 0:
        status, done = NOTHING, True
    elif not finite(cost):
        status, done = REFUSED, True
    ue = g.ue
    ei, ej = g.edge[ue, 0], g.edge[ue, 1]
    pos_of = np.full(E, -1, dtype=np.int64)
    pos_of[ue] = np.arange(len(ue))
    ent = pos_of[g.ee]      # an entry's row among the used edges
    with np.errstate(all="ignore"):
        for it in range(outer):
            if not done:
                if relin:
                    jc, res = edge_lin(pose[ei], pose[ej], g.meas[ue])
                    f = irls(chi2(res, g.weight[ue]), huber)
                    weff = np.stack((g.weight[ue, 0] * f, g.weight[ue, 1] * f), axis=1)
                    Ji, Jj = jac(jc, 0), jac(jc, 1)
                    Jent = np.where((g.eend == 0)[:, None], Ji[ent], Jj[ent])
                    gv = g.gather(jt(Jent, wr(res, weff)[ent]), 6)
                    D = g.gather(jtwj(Jent, weff[ent]), 21)
                    gv[~free] = 0.0
                    D[~free] = 0.0
                    relin = False
                r = np.zeros((V, 6))
                z = np.zeros((V, 6))
                r[free] = -gv[free]
                zz, ok = precond(D[free], lam, r[free])
                z[free] = zz
                bad = not ok.all()
                d = np.zeros(V)
                d[free] = dot6(r[free], zz)
                rz = tree_sum(d)
                p, x = z.copy(), np.zeros((V, 6))
                if bad or not finite(rz):
                    status, done = REFUSED, True
                elif not rz > 0.0:
                    status, done = CONVERGED, True
                if not done:
                    rz0 = rz
                    Dd = D[:, DIAG]
                    for n in range(cg_iters):
                        s = ju_dense(Ji, Jj, weff, p[ei], p[ej])
                        Ap = g.gather(jt(Jent, s[ent]), 6)
                        Ap = Ap + ((lam * Dd) * p)
                        d = np.zeros(V)
                        d[free] = dot6(p[free], Ap[free])
                        pAp = tree_sum(d)
                        if not (pAp > 0.0 and finite(pAp)):
                            break
                        al = rz / pAp
                        x[free] = x[free] + (al * p[free])
                        r[free] = r[free] - (al * Ap[free])
                        zz, ok = precond(D[free], lam, r[free])
                        okf = np.zeros(V, dtype=bool)
                        okf[free] = ok
                        d = np.zeros(V)
                        d[okf] = dot6(r[okf], zz[ok])
                        z[okf] = zz[ok]
                        rz2 = tree_sum(d)
                        cg_total += 1
                        if not ok.all():
                            status, done = REFUSED, True
                            break
                        if not cg_continue(rz2, rz0, cg_tol):
                            break
                        be = rz2 / rz
                        p[free] = z[free] + (be * p[free])
                        rz = rz2
                if not done:
                    d = np.zeros(V)
                    d[free] = dot6(x[free], x[free])
                    if small_step(tree_sum(d)):
                        status, done = CONVERGED, True
                if not done:
                    pn = pose.copy()
                    out, ok = retract(pose[free], x[free])
                    pn[free] = out
                    if not ok.all():
                        status, done = REFUSED, True
                if not done:
                    trial, _ = g.cost(pn, huber)
                    if accept(cost, trial):
                        pose = pn
                        if converged(cost, trial):
                            status, done = CONVERGED, True
                        cost = trial
                        accepted += 1
                        lam = lam * 0.1
                        relin = True
                    else:
                        refused += 1
                        lam = f64(lambda_up(lam))
            costs[it + 1] = cost
    chi = np.full(E, -1.0)
    if len(ue):
        chi[ue] = g.cost(pose, huber)[1]
    info = np.array([status, accepted, refused, cg_total, used, E - used, nfree if accepted > 0 else 0, 0], dtype=np.int32)
    return pose, costs, chi, info


def solve(pose, edge, meas, weight, fixed=None, node_off=None, edge_off=None, outer=10, cg_iters=100, cg_tol=1e-6, lambda0=1e-4, huber=0.0):
    """lpd_pgo_solve behind ops.pgo_solve: -> (pose [V, 12], cost [G, outer + 1], chi2 [E], info [G, 8])"""
    pose = np.ascontiguousarray(pose, dtype=f64).reshape(-1, 12)
    edge = np.ascontiguousarray(edge, dtype=np.int32).reshape(-1, 2)
    meas = np.ascontiguousarray(meas, dtype=f64).reshape(-1, 12)
    weight = np.ascontiguousarray(weight, dtype=f64).reshape(-1, 2)
    V, E = pose.shape[0], edge.shape[0]
    fixed = np.zeros(V, dtype=np.uint8) if fixed is None else np.asarray(fixed).astype(np.uint8)
    node_off = [0, V] if node_off is None else [int(v) for v in node_off]
    edge_off = [0, E] if edge_off is None else [int(v) for v in edge_off]
    G = len(node_off) - 1
    ptr, idx = csr(edge, node_off, edge_off, V)
    out_pose, cost, chi, info = pose.copy(), np.zeros((G, outer + 1)), np.full(E, -1.0), np.zeros((G, 8), dtype=np.int32)
    for gi in range(G):
        n0, n1, e0, e1 = node_off[gi], node_off[gi + 1], edge_off[gi], edge_off[gi + 1]
        rows = []
        for k in range(n0, n1):
            rows.append([((m >> 1) - e0, m & 1) for m in idx[ptr[k]:ptr[k + 1]] if 2 * e0 <= m < 2 * e1])
        g = _Graph(pose[n0:n1], fixed[n0:n1], edge[e0:e1], meas[e0:e1], weight[e0:e1], rows)
        out_pose[n0:n1], cost[gi], chi[e0:e1], info[gi] = _solve_graph(g, int(outer), int(cg_iters), float(cg_tol), float(lambda0), float(huber))
    return out_pose, cost, chi, info


# ---- synthetic graphs ----------------------------------------------------------------------------------------------------------------
def rot_of(w):
    """[3] -> [3, 3]: the rotation of the unit quaternion (1, w / 2) normalised (no trigonometry: what the retraction uses)"""
    return dR(np.asarray(w, dtype=f64).reshape(1, 3))[0]


def yaw_rot(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def pose12(R, t):
    return np.concatenate((R, np.asarray(t, dtype=f64).reshape(3, 1)), axis=1).reshape(12)


def mul12(A, B):
    A, B = A.reshape(3, 4), B.reshape(3, 4)
    return pose12(A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3] + A[:, 3])


def inv12(A):
    A = A.reshape(3, 4)
    return pose12(A[:, :3].T, -A[:, :3].T @ A[:, 3])


def two_laps(seed, V, loops_every=4, drift=(0.004, 0.05), loop_noise=(0.003, 0.07), outliers=0.0, radius=50.0):
    """Two laps of a loop of radius `radius` with a gentle roll / pitch / height wave: the true poses gt [V, 12]; odometry edges Z =
    the true step times a random rotation and translation (sigma drift); the start = the odometry integrated from gt[0]; loop edges
    between a node of the second lap and its place on the first (sigma loop_noise), every loops_every nodes; a share `outliers` of the
    loops replaced by a gross error.  -> dict(gt, start, edge, meas, weight, is_loop, is_outlier)"""
    rng = np.random.default_rng(seed)
    half = V // 2
    gt = []
    for k in range(V):
        th = 2.0 * np.pi * k / half
        R = yaw_rot(th + np.pi / 2.0) @ rot_of([0.02 * np.sin(3 * th), 0.02 * np.cos(2 * th), 0.0])
        gt.append(pose12(R, [radius * np.cos(th), radius * np.sin(th), 2.0 * np.sin(th)]))
    gt = np.array(gt)
    edge, meas, is_loop, is_out = [], [], [], []
    for k in range(V - 1):
        Z = mul12(mul12(inv12(gt[k]), gt[k + 1]), pose12(rot_of(rng.normal(0.0, drift[0], 3)), rng.normal(0.0, drift[1], 3)))
        edge.append((k, k + 1)), meas.append(Z), is_loop.append(False), is_out.append(False)
    for k in range(0, half, loops_every):
        j = k + half
        if j >= V:
            break
        Z = mul12(mul12(inv12(gt[j]), gt[k]), pose12(rot_of(rng.normal(0.0, loop_noise[0], 3)), rng.normal(0.0, loop_noise[1], 3)))
        out = bool(rng.random() < outliers)
        if out:
            Z = mul12(Z, pose12(yaw_rot(rng.uniform(0.5, 1.5)), rng.uniform(8.0, 15.0, 3) * rng.choice([-1.0, 1.0], 3)))
        edge.append((j, k)), meas.append(Z), is_loop.append(True), is_out.append(out)
    start = [gt[0]]
    for k in range(V - 1):
        start.append(mul12(start[-1], meas[k]))
    is_loop = np.array(is_loop)
    weight = np.where(is_loop[:, None], np.array([[1.0 / loop_noise[0] ** 2, 1.0 / loop_noise[1] ** 2]]), np.array([[1.0 / drift[0] ** 2, 1.0 / drift[1] ** 2]]))
    return dict(gt=gt, start=np.array(start), edge=np.array(edge, dtype=np.int32), meas=np.array(meas), weight=np.ascontiguousarray(weight),
                is_loop=is_loop, is_outlier=np.array(is_out))


def ate(pose, gt):
    """root mean square of the position error, metres"""
    return float(np.sqrt(np.mean(np.sum((pose.reshape(-1, 3, 4)[:, :, 3] - gt.reshape(-1, 3, 4)[:, :, 3]) ** 2, axis=1))))


def total_cost(pose, edge, meas, weight, huber=0.0):
    r = residual(pose[edge[:, 0]], pose[edge[:, 1]], meas)
    return float(np.sum(rho(chi2(r, weight), huber)))


LSMR = dict(atol=1e-12, btol=1e-12)      # the trust-region step by LSMR to this residual: at its default 1e-2 the iteration crawls


def scipy_solve(start, edge, meas, weight, huber=0.0):
    """The independent reference: scipy.optimize.least_squares (trust-region reflective, finite-difference Jacobian on the sparsity
    pattern of the graph) on the same residuals from the same start, node 0 fixed, the same retraction as the parametrisation of the
    steps around the start.  huber > 0 uses scipy's own 'huber' loss on the per-edge residual norm, which is the same rho.
    -> (pose [V, 12], cost)"""
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix
    V, E = start.shape[0], edge.shape[0]
    sw = np.sqrt(_w6(weight))

    def poses_of(dv):
        x = np.zeros((V, 6))
        x[1:] = dv.reshape(V - 1, 6)
        return retract(start, x)[0]

    def fun(dv):
        P = poses_of(dv)
        return (sw * residual(P[edge[:, 0]], P[edge[:, 1]], meas)).reshape(-1)

    sp = lil_matrix((6 * E, 6 * (V - 1)), dtype=np.int8)
    for e, (i, j) in enumerate(edge):
        for n in (i, j):
            if n > 0:
                sp[6 * e:6 * e + 6, 6 * (n - 1):6 * (n - 1) + 6] = 1
    if huber > 0.0:
        # scipy's loss acts on single squared residuals; the cost here thresholds an EDGE's chi2, so the robust case is minimised by IRLS
        # around scipy's linear loss: the weights are re-made from the current chi2 until they stop changing
        dv = np.zeros(6 * (V - 1))
        for _ in range(30):
            P = poses_of(dv)
            f = np.sqrt(irls(chi2(residual(P[edge[:, 0]], P[edge[:, 1]], meas), weight), huber))

            def fun_w(d, f=f):
                return (fun(d).reshape(E, 6) * f[:, None]).reshape(-1)
            s = least_squares(fun_w, dv, jac_sparsity=sp, xtol=1e-12, ftol=1e-12, gtol=1e-12, tr_options=LSMR)
            if np.max(np.abs(s.x - dv)) < 1e-9:
                dv = s.x
                break
            dv = s.x
    else:
        dv = least_squares(fun, np.zeros(6 * (V - 1)), jac_sparsity=sp, xtol=1e-12, ftol=1e-12, gtol=1e-12, tr_options=LSMR).x
    P = poses_of(dv)
    return P, total_cost(P, edge, meas, weight, huber)


@functools.lru_cache(maxsize=None)
def quality_case(seed, V, outliers=0.0, huber=0.0):
    """a two-lap graph, the restatement's solution and scipy's, made once a process: dict(graph, ref = (pose, cost, chi2, info), scipy
    = (pose, cost))"""
    g = two_laps(seed, V, outliers=outliers)
    ref = solve(g["start"], g["edge"], g["meas"], g["weight"], huber=huber, **QUALITY_SOLVER)
    return dict(graph=g, ref=ref, scipy=scipy_solve(g["start"], g["edge"], g["meas"], g["weight"], huber))


QUALITY_SOLVER = dict(outer=24, cg_iters=200, cg_tol=1e-6, lambda0=1e-4)
