"""numpy restatement of lpd_radius_count / lpd_radius_fill (definitions: include/lpd_hip.h and csrc/lpd_places_math.h), shared by
tests/test_places_cpu.py and tests/test_places_gpu.py.  Everything is numpy float64, whose elementwise subtract / multiply / add are
single IEEE operations, rounded once each: the arithmetic of the definition.  Chunked over the queries so that a [chunk, D] mask is
all that is ever held."""
import numpy as np

ORIGIN = np.array([5735712.768124, 620084.402381])      # a UTM (northing, easting) magnitude: an fp32 ulp is 0.5 m there


def radius_sq(r):
    """the right-hand side of the comparison: one product"""
    return np.float64(r) * np.float64(r)


def within(qx, qy, px, py, r2):
    """the predicate, elementwise: (dx * dx) + (dy * dy) <= r2; NaN compares false"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.asarray(qx, dtype=np.float64) - np.asarray(px, dtype=np.float64)
        dy = np.asarray(qy, dtype=np.float64) - np.asarray(py, dtype=np.float64)
        return (dx * dx) + (dy * dy) <= r2


def radius_lists(qpos, dpos, r, seg_off=None, skip_seg=None, self_item=None, chunk=512):
    """the definition -> (off int32 [Q*S+1], idx int32, counts int32 [Q*S]); row g * S + s, local indices, ascending"""
    qpos = np.asarray(qpos, dtype=np.float64).reshape(-1, 2)
    dpos = np.asarray(dpos, dtype=np.float64).reshape(-1, 2)
    Q, D = qpos.shape[0], dpos.shape[0]
    seg = np.array([0, D] if seg_off is None else seg_off, dtype=np.int64)
    S = seg.size - 1
    assert seg[0] == 0 and seg[-1] == D and (np.diff(seg) >= 0).all()
    seg_of = np.repeat(np.arange(S), np.diff(seg))      # segment of item j
    local = np.arange(D) - seg[seg_of] if D else np.zeros(0, dtype=np.int64)
    r2 = radius_sq(r)
    counts = np.zeros(Q * S, dtype=np.int64)
    parts = []
    for q0 in range(0, Q, chunk):
        q1 = min(Q, q0 + chunk)
        m = within(qpos[q0:q1, 0, None], qpos[q0:q1, 1, None], dpos[None, :, 0], dpos[None, :, 1], r2)
        if self_item is not None:
            me = np.asarray(self_item[q0:q1], dtype=np.int64)
            ok = (me >= 0) & (me < D)
            m[np.nonzero(ok)[0], me[ok]] = False
        if skip_seg is not None:
            m &= seg_of[None, :] != np.asarray(skip_seg[q0:q1], dtype=np.int64)[:, None]
        rows, cols = np.nonzero(m)      # row-major: ascending g, then ascending j = ascending (segment, local index)
        counts += np.bincount((rows + q0) * S + seg_of[cols], minlength=Q * S)
        parts.append(local[cols])
    off = np.zeros(Q * S + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    idx = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return off.astype(np.int32), idx.astype(np.int32), counts.astype(np.int32)


def rows_of(off, idx):
    return [idx[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def route(T, seed):
    """route-like positions at UTM magnitude: a drive of T / 2 steps of 3 .. 7 m with a slowly turning heading, then the same road
    driven back with 3 m of lateral noise -- every place is visited twice, as in the data set's repeated runs"""
    g = np.random.default_rng(seed)
    half = (T + 1) // 2
    heading = np.cumsum(g.normal(0.0, 0.08, half))
    step = g.uniform(3.0, 7.0, half)
    xy = np.cumsum(np.stack((step * np.cos(heading), step * np.sin(heading)), 1), 0)
    back = xy[::-1][:T - half] + g.normal(0.0, 3.0, (T - half, 2))
    return np.concatenate((xy, back)) + ORIGIN


def training_lists(positions, pos_radius=10.0, near_radius=50.0):
    """-> (positives, near) as lists of ascending arrays: the item itself removed from positives, kept in near"""
    T = len(positions)
    po, pi, _ = radius_lists(positions, positions, pos_radius, self_item=np.arange(T))
    no, ni, _ = radius_lists(positions, positions, near_radius)
    return rows_of(po, pi), rows_of(no, ni)


def truth_table(db_positions, query_positions, r=25.0):
    """the layout of harness.build_truth_csr from positions -> (truth_off, truth_idx)"""
    seg = np.concatenate(([0], np.cumsum([len(d) for d in db_positions])))
    own = np.repeat(np.arange(len(query_positions)), [len(q) for q in query_positions])
    off, idx, _ = radius_lists(np.concatenate(query_positions), np.concatenate(db_positions), r, seg_off=seg, skip_seg=own)
    return off, idx
