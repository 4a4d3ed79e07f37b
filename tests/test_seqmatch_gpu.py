"""lpd_seq_match and lpdnet_hip/sequence.py on the GPU against the numpy restatement (tests/seq_ref.py).

The block of quantised distances is compared with float64 distances quantised the same way: at most 1 quantum apart.  For unit
descriptors the fp32 chain of 256 products carries an a-priori error of 4 * 256 * 2^-24 = 6.1e-5 = 1.0 quantum of 2^-14 (norms, dot
product and the three operations of the difference); the bound needs no measurement, and the MEASURE lines show how far below it the
kernel stays.  Everything behind the block is integers: `best` and `order` must EQUAL the restatement applied to the device's own
block.  The kernel gives a query to a workgroup of four waves and a candidate to a wave, lanes take hypotheses 64 at a time: the
sizes below lie on both sides of each.  (This module makes torch side streams: it sorts behind tests/test_clean_gpu.py)"""
import ctypes

import numpy as np
import pytest
import torch

import seq_ref as R
from lpdnet_hip import _lib, ops, sequence, verify
from test_seqmatch_cpu import QUALITY_MOVED_GATE, QUALITY_SEQ_GATE, QUALITY_SINGLE_MAX, quality_case

pytestmark = pytest.mark.gpu
f32 = np.float32
i32 = np.int32
GUARD = 2048
VEL = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def _up(dev, v, dt):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)


def _unit(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)


def _velocities(V, h, S):
    """V velocities whose steps reach the band's edge: max|steps| + S == 15 when V > 1"""
    if V == 1:
        return (float((ops.SEQ_BAND - S) // h),)
    top = (ops.SEQ_BAND - S) / h
    return tuple(np.linspace(-top, top, V).tolist())


def _offsets(g, n, runs):
    return np.unique(np.concatenate(([0, n], g.integers(0, n + 1, max(runs - 1, 0))))).astype(i32)


def _candidates(g, nq, nd, K, d_off):
    """random rows, both kinds of skipped entry, and the first and last row of the table and of every run"""
    cand = g.integers(0, nd, (nq, K)).astype(i32)
    cand[g.random((nq, K)) < 0.08] = -1
    cand[g.random((nq, K)) < 0.05] = nd
    cand[g.random((nq, K)) < 0.02] = nd + 7
    ends = np.unique(np.concatenate((d_off[:-1], d_off[1:] - 1, [0, nd - 1]))).clip(0, nd - 1)
    sel = g.random((nq, K)) < 0.2
    cand[sel] = g.choice(ends, int(sel.sum()))
    return cand


def _gpu(dev, Q, D, cand, steps, S, mt, q_off=None, d_off=None, want_block=True, same=False):
    q = _up(dev, Q, f32)
    d = q if same else _up(dev, D, f32)
    out = ops.seq_match(q, d, _up(dev, cand, i32), steps, S, mt, q_off=q_off, d_off=d_off, want_block=want_block)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _check(tag, Q, D, cand, steps, S, mt, q_off, d_off, got):
    """block within one quantum of float64 and -1 exactly where defined; best and order equal to the restatement of the device's block"""
    best, order, block = got
    h = (np.asarray(steps).shape[1] - 1) // 2
    ref = R.blocks_f64(Q, D, cand, h)
    assert np.array_equal(block == -1, ref == -1), tag
    dev_q = int(np.abs(block.astype(np.int64) - ref)[ref >= 0].max()) if (ref >= 0).any() else 0
    print(f"MEASURE seq/block {tag} largest deviation {dev_q} quanta over {int((ref >= 0).sum())} entries")
    assert dev_q <= 1, tag
    assert (block[:, :, 31] == -1).all() and (block[:, :, :, 31] == -1).all() and (block[:, :, 2 * h + 1:] == -1).all()
    wb, wo = R.match(block, cand, steps, S, mt, len(D), q_off, d_off)
    assert np.array_equal(best, wb), tag
    assert np.array_equal(order, wo), tag
    assert (np.sort(order, axis=1) == np.arange(order.shape[1])).all()
    return dev_q


# ---- 1. block, best and order over the sizes ------------------------------------------------------------------------------------------
# (nq, nd, K, h, S, V, dim, runs): nq = 1, 2, 31, 33, 130; nd = 1, 16, 31, 32, 33, 200; K = 1, 3, 4, 5, 25, 64 (both sides of the four
# waves); h = 1, 5, 15; S = 0, 2 and the largest a table allows (15 - max|steps|); V = 1, 6; V (2S + 1) = 60, 63, 64, 65, 66, 1023, 1024 on
# both sides of the 64 lanes; dim = 64, 128, 256
SHAPES = [
    (1, 1, 1, 1, 0, 1, 64, 1),
    (2, 16, 3, 5, 2, 6, 128, 1),
    (31, 31, 4, 15, 0, 1, 256, 2),        # h = 15: 31 query rows, the velocity 1 reaches the band's edge, S = 0 is the largest
    (33, 32, 5, 5, 2, 6, 256, 3),
    (130, 200, 25, 5, 2, 6, 256, 4),
    (33, 33, 64, 1, 14, 1, 64, 2),        # h = 1 and the velocity 1: S = 14 is the largest
    (31, 200, 5, 5, 5, 6, 128, 3),        # max|steps| = 10: S = 5 is the largest; 66 hypotheses
    (33, 200, 4, 5, 2, 12, 64, 3),        # 60
    (33, 200, 3, 5, 2, 13, 64, 3),        # 65
    (2, 33, 3, 1, 0, 63, 64, 1),
    (2, 33, 4, 1, 0, 64, 64, 1),
    (2, 33, 5, 1, 0, 65, 64, 2),
    (2, 33, 2, 1, 1, 341, 128, 1),        # 1023
    (2, 16, 2, 1, 0, 1024, 64, 1),        # 1024
]


@pytest.mark.parametrize("nq,nd,K,h,S,V,dim,runs", SHAPES)
def test_block_best_and_order(cuda, nq, nd, K, h, S, V, dim, runs):
    g = np.random.default_rng(nq * 1000 + nd * 10 + K)
    Q, D = _unit(nq, dim, nq + 1), _unit(nd, dim, nd + 2)
    if nd > 4:
        D[g.integers(0, nd, 3)] = D[1]                      # duplicated rows
        Q[g.integers(0, nq, 2)] = D[g.integers(0, nd, 2)]   # exact zeros
    q_off, d_off = _offsets(g, nq, runs), _offsets(g, nd, runs)
    cand = _candidates(g, nq, nd, K, d_off)
    steps = R.steps_table(_velocities(V, h, S), h)
    assert np.abs(steps).max() + S == 15 or (V == 1 and h > 1 and np.abs(steps).max() + S <= 15)
    mt = 1 + (nq + K) % (h + 1)
    got = _gpu(cuda, Q, D, cand, steps, S, mt, q_off, d_off)
    _check(f"nq={nq} nd={nd} K={K} h={h} S={S} V={V} dim={dim}", Q, D, cand, steps, S, mt, q_off, d_off, got)
    if nq >= 31 and nd >= 31:
        assert (got[0][:, :, 0] >= 0).any() and (got[0][:, :, 0] < 0).any()      # both outcomes occur


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------------
def test_runs_of_one_row(cuda):
    nq, nd, K, h, S = 9, 12, 5, 5, 2
    Q, D = _unit(nq, 64, 1), _unit(nd, 64, 2)
    cand = np.random.default_rng(3).integers(0, nd, (nq, K)).astype(i32)
    steps = R.steps_table(VEL, h)
    q_off, d_off = np.arange(nq + 1, dtype=i32), np.arange(nd + 1, dtype=i32)
    got = _gpu(cuda, Q, D, cand, steps, S, 1, q_off, d_off)
    _check("runs of one row", Q, D, cand, steps, S, 1, q_off, d_off, got)
    assert (got[0][:, :, 2] == 1).all() and (got[0][:, :, 3] == cand).all() and (got[0][:, :, 0] == R.hyp(0, 0, S)).all()
    got = _gpu(cuda, Q, D, cand, steps, S, 2, q_off, d_off)      # two terms never fit into a run of one row
    assert (got[0] == (-1, 0, 0, -1)).all() and (got[1] == np.arange(K)).all()


def test_first_and_last_rows_of_runs_and_of_the_table(cuda):
    nq, nd, h, S = 40, 50, 5, 2
    Q, D = _unit(nq, 128, 4), _unit(nd, 128, 5)
    d_off = np.array([0, 1, 20, 20, 49, 50], dtype=i32)      # a run of one row at each end of the table, an empty run
    q_off = np.array([0, 3, 40], dtype=i32)
    cand = np.tile(np.array([0, 1, 19, 20, 48, 49], dtype=i32), (nq, 1))
    steps = R.steps_table(VEL, h)
    for mt in (1, 6):
        got = _gpu(cuda, Q, D, cand, steps, S, mt, q_off, d_off)
        _check(f"run ends min_terms={mt}", Q, D, cand, steps, S, mt, q_off, d_off, got)
    assert (got[0][:, (0, 5), 0] == -1).all()      # six terms do not fit into a run of one row
    rows = got[0][:, :, 3]
    assert ((rows[:, 1:3] >= 1) & (rows[:, 1:3] < 20) | (rows[:, 1:3] == -1)).all() and ((rows[:, 3:5] >= 20) & (rows[:, 3:5] < 49) | (rows[:, 3:5] == -1)).all()


def _raw(dev, Q, D, cand, steps, S, mt, q_off, d_off, want_block=True, guard=GUARD, over=None):
    """the library called through the binding with guard rows around every output -> (rc, best, order, block) with the guards checked"""
    nq, nd, K = len(Q), len(D), cand.shape[1]
    V, L = steps.shape
    fill = -77
    q, d = _up(dev, Q, f32), _up(dev, D, f32)
    bufs = {n: torch.full((guard + size + guard,), fill, dtype=torch.int32, device=dev)
            for n, size in (("best", nq * K * 4), ("order", nq * K), ("block", nq * K * 1024))}
    ws = torch.zeros((nq + nd + 2 * guard,), dtype=torch.float32, device=dev)
    t = dict(cand=_up(dev, cand, i32), steps=_up(dev, steps, i32), q_off=_up(dev, q_off, i32), d_off=_up(dev, d_off, i32))
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)      # noqa: E731
    a = dict(Q=p(q), ldq=Q.shape[1], nq=nq, q_off=p(t["q_off"]), SQ=len(q_off) - 1, D=p(d), ldd=D.shape[1], nd=nd, d_off=p(t["d_off"]),
             SD=len(d_off) - 1, dim=Q.shape[1], cand=p(t["cand"]), K=K, steps=p(t["steps"]), V=V, h=(L - 1) // 2, S=S, min_terms=mt,
             best=p(bufs["best"], 4 * guard), order=p(bufs["order"], 4 * guard), block=p(bufs["block"], 4 * guard) if want_block else None,
             ws=p(ws, 4 * guard), stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    a.update(over or {})
    rc = _lib.load().lpd_seq_match(*a.values())
    torch.cuda.synchronize()
    out = {n: b.cpu().numpy() for n, b in bufs.items()}
    for n, b in out.items():
        assert (b[:guard] == fill).all() and (b[-guard:] == fill).all(), n      # nothing is written outside
    wsn = ws.cpu().numpy()
    assert (wsn[:guard] == 0).all() and (wsn[-guard:] == 0).all()
    return (rc, out["best"][guard:-guard].reshape(nq, K, 4), out["order"][guard:-guard].reshape(nq, K),
            out["block"][guard:-guard].reshape(nq, K, 32, 32))


def test_skipped_candidates_between_guard_rows(cuda):
    nq, nd, K, h, S = 7, 40, 6, 5, 2
    Q, D = _unit(nq, 64, 6), _unit(nd, 64, 7)
    cand = np.tile(np.array([-1, 5, nd, 39, -2147483648, 2147483647], dtype=i32), (nq, 1))
    cand[3] = -1
    cand[4] = nd + 1
    steps = R.steps_table(VEL, h)
    off = np.array([0, nq], dtype=i32), np.array([0, nd], dtype=i32)
    rc, best, order, block = _raw(cuda, Q, D, cand, steps, S, 3, *off)
    assert rc == 0
    _check("skipped", Q, D, cand, steps, S, 3, off[0], off[1], (best, order, block))
    skipped = (cand < 0) | (cand >= nd)
    assert (best[skipped] == (-1, 0, 0, -1)).all() and (block[skipped] == -1).all() and (best[~skipped][:, 0] >= 0).all()
    assert (order[3] == np.arange(K)).all() and (order[4] == np.arange(K)).all()
    assert set(order[0, :2].tolist()) == {1, 3} and order[0, 2:].tolist() == [0, 2, 4, 5]      # the others in retrieval order
    rc2, best2, order2, block2 = _raw(cuda, Q, D, cand, steps, S, 3, *off, want_block=False)
    assert rc2 == 0 and np.array_equal(best, best2) and np.array_equal(order, order2) and (block2 == -77).all()      # NULL: not written


def test_ties_go_to_the_lower_hypothesis_and_rank(cuda):
    nq, nd, K, h, S = 30, 60, 6, 3, 2
    D = _unit(nd, 128, 8)
    D[20:45] = D[20]                                  # a stretch of one repeated place: every line through it has the same sum
    Q = _unit(nq, 128, 9)
    Q[5:25] = D[20]
    cand = np.tile(np.array([30, 31, 30, 7, 31, 30], dtype=i32), (nq, 1))      # duplicated candidates
    steps = R.steps_table((1.0, 1.0, -1.0, 0.5, 1.0), h)                       # duplicated velocities
    got = _gpu(cuda, Q, D, cand, steps, S, h + 1, None, None)
    _check("ties", Q, D, cand, steps, S, h + 1, None, None, got)
    best, order, _ = got
    mid = best[10:20]
    assert (mid[:, (0, 1, 2, 4, 5), 1] == 0).all() and (mid[:, (0, 1, 2, 4, 5), 0] == 0).all()      # sum 0 everywhere: e = 0 = (v 0, s -S)
    assert (mid[:, 0, 3] == 30 - S).all()
    assert (order[10:20] == [0, 1, 2, 4, 5, 3]).all()                                                  # equal means: the lower r


def test_nan_and_inf_rows_on_either_side(cuda):
    nq, nd, K, h, S = 33, 64, 5, 5, 2
    Q, D = _unit(nq, 256, 10), _unit(nd, 256, 11)
    Q[4, 17] = np.nan
    Q[20] = np.nan
    Q[9, 0] = np.inf
    D[30, 255] = np.nan
    D[31, 3] = -np.inf
    D[50] = np.nan
    g = np.random.default_rng(12)
    cand = g.integers(20, 60, (nq, K)).astype(i32)
    steps = R.steps_table(VEL, h)
    got = _gpu(cuda, Q, D, cand, steps, S, 4, None, None)
    _check("nan", Q, D, cand, steps, S, 4, None, None, got)
    block = got[2]
    assert (block[20, :, 5, :] == -1).all() and (block[19, :, 6, :] == -1).all()      # the NaN query row, seen from its neighbours too
    assert (block[25, :, 5, :][:, np.array([15])] >= 0).all()                         # a finite pair of rows in the table is a distance
    assert (got[0][:, :, 2] <= 11).all() and (got[0][:, :, 2][got[0][:, :, 0] >= 0] >= 4).all()


def test_one_tensor_for_both_tables_and_strided_views(cuda):
    n, K, h, S, dim = 70, 5, 5, 2, 128
    X = _unit(n, dim, 13)
    g = np.random.default_rng(14)
    off = _offsets(g, n, 3)
    cand = _candidates(g, n, n, K, off)
    steps = R.steps_table(VEL, h)
    got = _gpu(cuda, X, X, cand, steps, S, 6, off, off, same=True)
    _check("Q is D", X, X, cand, steps, S, 6, off, off, got)
    two = _gpu(cuda, X, X, cand, steps, S, 6, off, off)
    assert all(np.array_equal(a, b) for a, b in zip(got, two))
    # every tensor argument as a strided view: rows with a leading dimension, every other column of a wider cand, a reversed steps
    # table and offsets cut out of longer arrays
    wide = torch.zeros((n, dim + 24), dtype=torch.float32, device=cuda)
    wide[:, 8:8 + dim] = _up(cuda, X, f32)
    dwide = torch.zeros((n, 2 * dim), dtype=torch.float32, device=cuda)
    dwide[:, dim:] = _up(cuda, X, f32)
    cwide = torch.full((n, 2 * K), -5, dtype=torch.int32, device=cuda)
    cwide[:, ::2] = _up(cuda, cand, i32)
    qv, dv, cv = wide[:, 8:8 + dim], dwide[:, dim:], cwide[:, ::2]
    assert not qv.is_contiguous() and not dv.is_contiguous() and not cv.is_contiguous()
    sv = np.ascontiguousarray(steps[::-1])[::-1]
    ov = np.concatenate((off, off))[:len(off)]
    assert not sv.flags.c_contiguous
    out = ops.seq_match(qv, dv, cv, sv, S, 6, q_off=torch.from_numpy(ov), d_off=ov, want_block=True)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(got, out))
    # a table of fewer channels is padded with zero channels, which add nothing
    X48 = np.ascontiguousarray(X[:, :48])
    X48 /= np.linalg.norm(X48, axis=1, keepdims=True)
    got = _gpu(cuda, X48, X48, cand, steps, S, 6, off, off)
    _check("dim 48", X48, X48, cand, steps, S, 6, off, off, got)


# ---- 3. behaviour ---------------------------------------------------------------------------------------------------------------------
def _case(seed, nq=96, nd=150, K=25, dim=256):
    g = np.random.default_rng(seed)
    Q, D = _unit(nq, dim, seed + 1), _unit(nd, dim, seed + 2)
    q_off, d_off = _offsets(g, nq, 3), _offsets(g, nd, 3)
    return Q, D, _candidates(g, nq, nd, K, d_off), R.steps_table(VEL, 5), q_off, d_off


def test_without_a_block_and_repeated(cuda):
    Q, D, cand, steps, q_off, d_off = _case(20)
    a = _gpu(cuda, Q, D, cand, steps, 2, 6, q_off, d_off)
    b = _gpu(cuda, Q, D, cand, steps, 2, 6, q_off, d_off, want_block=False)
    assert b[2] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for _ in range(3):
        c = _gpu(cuda, Q, D, cand, steps, 2, 6, q_off, d_off)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))


def test_two_streams_give_equal_bits(cuda):
    Q, D, cand, steps, q_off, d_off = _case(21)
    want = _gpu(cuda, Q, D, cand, steps, 2, 6, q_off, d_off)
    q, d, c = _up(cuda, Q, f32), _up(cuda, D, f32), _up(cuda, cand, i32)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    outs = []
    for rep in range(3):
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(ops.seq_match(q, d, c, steps, 2, 6, q_off=q_off, d_off=d_off, want_block=True))
    torch.cuda.synchronize()
    for out in outs:
        assert all(w.tobytes() == o.cpu().numpy().tobytes() for w, o in zip(want, out))


def test_library_checks_its_arguments(cuda):
    nq, nd, K, h, S = 4, 20, 3, 5, 2
    Q, D = _unit(nq, 64, 30), _unit(nd, 64, 31)
    cand = np.zeros((nq, K), dtype=i32)
    steps = R.steps_table(VEL, h)
    off = np.array([0, nq], dtype=i32), np.array([0, nd], dtype=i32)
    lib = _lib.load()
    assert _raw(cuda, Q, D, cand, steps, S, 6, *off)[0] == 0
    for over in (dict(dim=100), dict(dim=32), dict(ldq=63), dict(ldq=66), dict(ldd=62), dict(nq=0), dict(nd=0), dict(SQ=0), dict(SD=0), dict(K=0), dict(K=65),
                 dict(h=0), dict(h=16), dict(S=-1), dict(S=16), dict(V=0), dict(V=205), dict(V=1025, S=0), dict(min_terms=0), dict(min_terms=12),
                 dict(Q=None), dict(D=None), dict(q_off=None), dict(d_off=None), dict(cand=None), dict(steps=None), dict(best=None), dict(order=None),
                 dict(ws=None)):
        rc, best, order, block = _raw(cuda, Q, D, cand, steps, S, 6, *off, over=over)
        assert rc != 0 and b"lpd_seq_match" in lib.lpd_last_error(), over
        assert (best == -77).all() and (order == -77).all() and (block == -77).all(), over      # refused before anything is launched
    q = _up(cuda, np.concatenate((Q, Q), 1)[:, 1:65].copy(), f32)
    misaligned = ctypes.c_void_p(q.data_ptr() + 4)
    assert _raw(cuda, Q, D, cand, steps, S, 6, *off, over=dict(Q=misaligned))[0] != 0


# ---- 4. the wrapper -------------------------------------------------------------------------------------------------------------------
def test_match_sequences_equals_the_restatements_chain(cuda):
    Q, D, cand, steps, q_off, d_off = _case(40, nq=60, nd=90, K=7, dim=128)
    s = sequence.SeqSearch()
    assert np.array_equal(steps, s.steps_table())
    _, _, block = _gpu(cuda, Q, D, cand, steps, s.shifts, s.min_terms, q_off, d_off)
    wb, wo = R.match(block, cand, steps, s.shifts, s.min_terms, len(D), q_off, d_off)
    for topk, max_mean in ((_up(cuda, cand, i32), 1.9), (_up(cuda, cand, np.int64), None)):
        m = sequence.match_sequences(_up(cuda, Q, f32), _up(cuda, D, f32), topk, q_off, d_off, search=s, max_mean=max_mean)
        torch.cuda.synchronize()
        want = R.chain(wb, wo, s.velocities, s.shifts, max_mean)
        for name in ("hypothesis", "velocity", "shift", "row", "sum", "terms", "valid", "order", "mean"):
            got = getattr(m, name).cpu().numpy()
            assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
        assert (m.accepted is None) == (max_mean is None)
        if max_mean is not None:
            acc = m.accepted.cpu().numpy()
            assert np.array_equal(acc, want["accepted"]) and 0 < acc.sum() < want["valid"].sum()
        assert m.topk().dtype == torch.int32 and np.array_equal(m.topk().cpu().numpy(), want["topk"])
        assert np.array_equal(m.topk(3).cpu().numpy(), want["topk"][:, :3])
        with pytest.raises(ValueError):
            m.topk(8)
    one = sequence.match_sequences(_up(cuda, Q, f32), _up(cuda, D, f32), _up(cuda, cand, i32))      # None offsets: one run
    assert np.array_equal(one.best.cpu().numpy(), R.match(block, cand, steps, s.shifts, s.min_terms, len(D))[0])


def test_self_candidates_equal_a_numpy_mask(cuda):
    n, dim = 120, 64
    base = _unit(n, dim, 50)
    X = base + 0.8 * np.roll(base, 1, axis=0) + 0.8 * np.roll(base, -1, axis=0)      # neighbours along the drive are near: they must go
    X[90:110] = X[10:30] + 0.01 * _unit(20, dim, 51)                                  # a loop: these must stay
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(f32)
    x = _up(cuda, X, f32)
    for off, k, exclude in ((None, 5, 3), (np.array([0, 50, 120], dtype=i32), 4, 10), (None, 64, 40), (None, 3, 0)):
        kk = min(k + 2 * exclude + 1, n)
        idx = ops.retrieval_topk(x, x, kk)[0].cpu().numpy()
        got = sequence.self_candidates(x, off, k=k, exclude=exclude)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, k)
        got = got.cpu().numpy()
        assert np.array_equal(got, R.self_candidates(idx, off, k, exclude))
        i = np.arange(n)[:, None]
        if off is None:
            assert ((got < 0) | (np.abs(got - i) > exclude)).all()
    loop = sequence.self_candidates(x, None, k=5, exclude=3).cpu().numpy()
    assert (loop[95:105, 0] == np.arange(15, 25)).all()
    assert (sequence.self_candidates(x, None, k=64, exclude=40).cpu().numpy()[40:80, -1] == -1).all()      # 39 rows stay, fewer than k: padded


def test_quality_on_the_device(cuda):
    def scorer(Q, D, q_off, s):
        q, d = _up(cuda, Q, f32), _up(cuda, D, f32)
        cand, _ = ops.retrieval_topk(q, d, 10)
        best, order, _ = ops.seq_match(q, d, cand, s.steps_table(), s.shifts, s.min_terms, q_off=q_off)
        torch.cuda.synchronize()
        return cand.cpu().numpy(), best.cpu().numpy(), order.cpu().numpy()
    single, seq, moved = quality_case(0, scorer=scorer)
    print(f"MEASURE seq/quality-device seed=0 single-frame {single:.3f} sequence {seq:.3f} after the shift {moved:.3f}")
    assert single <= QUALITY_SINGLE_MAX
    assert seq >= QUALITY_SEQ_GATE and moved >= QUALITY_MOVED_GATE


def test_topk_goes_into_verify_candidates(cuda):
    nq, nd, N = 6, 12, 256
    g = np.random.default_rng(60)
    Q, D = _unit(nq, 64, 61), _unit(nd, 64, 62)
    cand = g.integers(0, nd, (nq, 4)).astype(i32)
    cand[0] = -1
    cand[2, 1] = nd
    m = sequence.match_sequences(_up(cuda, Q, f32), _up(cuda, D, f32), _up(cuda, cand, i32), search=sequence.SeqSearch(half_length=2, min_terms=2))
    rows = m.topk(3)
    clouds_q = _up(cuda, g.uniform(-20, 20, (nq, N, 3)), f32)
    clouds_d = _up(cuda, g.uniform(-20, 20, (nd, N, 3)), f32)
    v = verify.verify_candidates(clouds_q, clouds_d, rows, search=verify.AlignSearch(yaw_steps=8, shifts=2, fine=False))
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    assert tuple(v.valid.shape) == (nq, 3) and tuple(v.order.shape) == (nq, 3) and tuple(v.translation.shape) == (nq, 3, 2)
    assert np.array_equal(v.valid.cpu().numpy(), rows >= 0) and (rows[0] == -1).all() and (rows[1:, 0] >= 0).all()
