"""fp64 reference of the local point-distribution features (include/lpd_hip.h, lpd_local_features) and the seeded test clouds of
tests/test_local_features_{cpu,gpu}.py.  numpy only: the definition, stated on the float32 inputs promoted to float64, with
numpy.linalg.eigh.  The neighbour lists are an ARGUMENT: the GPU tests pass the GPU's own lists, so kNN near-ties never enter a
comparison of feature values."""
import numpy as np

COLUMNS = ("C", "O", "L", "A", "V", "S2", "L2", "dZ", "sZ", "D")
KINDS = ("cube", "slab", "wire", "mixed")

# gates of the issue that introduced the kernel (absolute unless noted); floors measured for a plain fp32 restatement in its text
GATE_RATIO = 2e-5      # C, O, L, A, L2
GATE_MOMENT = 1e-6     # S2, dZ, sZ
GATE_DENSITY = 1e-5    # D, relative
GATE_V = 1e-4          # V, only where the fp64 gap (l2 - l3) / l1 > V_GAP
V_GAP = 1e-2
V_MAX_EXCLUDED = 0.10


def _wire(rng, n):
    t = rng.uniform(-1.0, 1.0, n)
    return np.stack((t, 0.3 * np.sin(3.0 * t), 0.2 * t), axis=1) + 0.01 * rng.standard_normal((n, 3))


def cloud(kind, N, seed):
    """One [N,3] float32 cloud, coordinates in [-1, 1]."""
    rng = np.random.default_rng(seed)
    if kind == "cube":
        p = rng.uniform(-1.0, 1.0, (N, 3))
    elif kind == "slab":
        p = np.concatenate((rng.uniform(-1.0, 1.0, (N, 2)), 0.02 * rng.standard_normal((N, 1))), axis=1)
    elif kind == "wire":
        p = _wire(rng, N)
    elif kind == "mixed":
        h = N // 2
        a = rng.uniform(-1.0, 1.0, (h, 3)) * np.array([1.0, 1.0, 0.05])
        b = _wire(rng, N - h) + np.array([0.0, 0.0, 0.5])
        p = np.concatenate((a, b), axis=0)[rng.permutation(N)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p, dtype=np.float32)


def clouds(B, N, seed=0, kinds=KINDS):
    """[B,N,3] float32: a batch that cycles through `kinds`."""
    return np.stack([cloud(kinds[b % len(kinds)], N, seed * 1000 + b) for b in range(B)], axis=0)


def knn_lists(x, K):
    """fp64 brute-force lists [B,N,K] int32, nearest first, self included (stable argsort)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape[:2] + (K,), dtype=np.int32)
    for b in range(x.shape[0]):
        d = ((x[b][:, None, :] - x[b][None, :, :]) ** 2).sum(-1)
        out[b] = np.argsort(d, axis=1, kind="stable")[:, :K]
    return out


def _xlogx(e):
    return np.where(e > 0, e * np.log(np.where(e > 0, e, 1.0)), 0.0)


def features_fixed(x, idx, k):
    """x [B,N,3], idx [B,N,>=k] -> (features [B,N,10] float64, gap [B,N] = (l2 - l3) / l1 (0 where l1 == 0)) at size k."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape[:2]
    f = np.zeros((B, N, 10))
    gap = np.zeros((B, N))
    for b in range(B):
        d = x[b][idx[b, :, :k].astype(np.int64)] - x[b][:, None, :]      # [N,k,3]
        mu = d.mean(axis=1)
        S = np.einsum("nki,nkj->nij", d, d) / k - mu[:, :, None] * mu[:, None, :]
        w, v = np.linalg.eigh(S)                                          # ascending
        l3, l2, l1 = (np.maximum(w[:, i], 0.0) for i in range(3))
        s = l1 + l2 + l3
        ok = s > 0
        sd = np.where(ok, s, 1.0)
        e1, e2, e3 = l1 / sd, l2 / sd, l3 / sd
        l1d = np.where(l1 > 0, l1, 1.0)
        f[b, :, 0] = np.where(ok, e3, 0.0)
        f[b, :, 1] = np.where(ok, np.cbrt(e1 * e2 * e3), 0.0)
        f[b, :, 2] = np.where(ok & (l1 > 0), (l1 - l2) / l1d, 0.0)
        f[b, :, 3] = np.where(ok, -(_xlogx(e1) + _xlogx(e2) + _xlogx(e3)), 0.0)
        f[b, :, 4] = np.where(ok, np.abs(v[:, 2, 0]), 0.0)
        f[b, :, 5] = S[:, 0, 0] + S[:, 1, 1]
        w2 = np.maximum(np.linalg.eigvalsh(S[:, :2, :2]), 0.0)
        f[b, :, 6] = np.where(w2[:, 1] > 0, w2[:, 0] / np.where(w2[:, 1] > 0, w2[:, 1], 1.0), 0.0)
        f[b, :, 7] = d[:, :, 2].max(axis=1) - d[:, :, 2].min(axis=1)
        f[b, :, 8] = S[:, 2, 2]
        r = np.sqrt((d[:, k - 1, :] ** 2).sum(-1))
        f[b, :, 9] = np.where(r > 0, k / (4.0 / 3.0 * np.pi * np.where(r > 0, r, 1.0) ** 3), 0.0)
        gap[b] = np.where(l1 > 0, (l2 - l3) / l1d, 0.0)
    return f, gap


def features(x, idx, k=None, kopt=None):
    """Fixed size k (default: the list length), or per-point sizes kopt [B,N] -> (features, gap) as features_fixed."""
    if kopt is None:
        return features_fixed(x, idx, idx.shape[2] if k is None else k)
    kopt = np.asarray(kopt)
    f = np.zeros(kopt.shape + (10,))
    gap = np.zeros(kopt.shape)
    for kk in np.unique(kopt):
        fk, gk = features_fixed(x, idx, int(kk))
        m = kopt == kk
        f[m], gap[m] = fk[m], gk[m]
    return f, gap


def entropies(x, idx, candidates):
    """eigenentropy at every candidate size: [B,N,len(candidates)] float64"""
    return np.stack([features_fixed(x, idx, int(k))[0][:, :, 3] for k in candidates], axis=-1)


def check_columns(got, ref, gap, label, columns=range(10)):
    """Print the MEASURE line of every column and return the list of gate violations (empty = pass).  got / ref [...,10] (got in
    float32 or float64), gap [...] the fp64 eigengap that qualifies a point for the V check."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 10)
    ref = np.asarray(ref).reshape(-1, 10)
    gap = np.asarray(gap).reshape(-1)
    bad = []
    if not np.isfinite(got).all():
        bad.append("non-finite output")
    for c in columns:
        name = COLUMNS[c]
        if name == "D":
            err = float((np.abs(got[:, c] - ref[:, c]) / np.maximum(np.abs(ref[:, c]), 1e-300)).max())
            gate = GATE_DENSITY
        elif name == "V":
            keep = gap > V_GAP
            excluded = 1.0 - keep.mean()
            err = float(np.abs(got[keep, c] - ref[keep, c]).max()) if keep.any() else 0.0
            gate = GATE_V
            print(f"MEASURE local_features/{label} V_excluded frac={excluded:.4f} cap={V_MAX_EXCLUDED}")
            if excluded > V_MAX_EXCLUDED:
                bad.append(f"V: {excluded:.3f} of the points excluded by the gap condition (cap {V_MAX_EXCLUDED})")
        else:
            err = float(np.abs(got[:, c] - ref[:, c]).max())
            gate = GATE_MOMENT if name in ("S2", "dZ", "sZ") else GATE_RATIO
        print(f"MEASURE local_features/{label} {name} err={err:.3e} gate={gate:.0e}")
        if not err <= gate:
            bad.append(f"{name}: err {err:.3e} > gate {gate:.0e}")
    return bad
