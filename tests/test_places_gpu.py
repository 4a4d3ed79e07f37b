"""lpd_radius_count / lpd_radius_fill, ops.radius_lists and lpdnet_hip.places on the GPU against tests/places_ref.py.

`off`, `idx` and `counts` are integer outputs of IEEE float64 arithmetic: they equal the numpy restatement EXACTLY in every case;
there is no tolerance and no case is excluded.  Every result also passes the structural checks of `_check`: strictly ascending rows
inside their segment, off = the scan of the counts, off[-1] == idx.numel(), and a second call that is torch.equal.
Measured on an MI355X (MEASURE lines of this file): see DESIGN.md section 13e."""
import ctypes

import numpy as np
import pytest
import torch

import places_ref as R

pytestmark = pytest.mark.gpu
CHUNK = 1024      # LPD_PLACES_CHUNK: candidates staged in LDS at a time
_ROUTES = {}


def _route(T):
    if T not in _ROUTES:
        _ROUTES[T] = R.route(T, seed=T)
    return _ROUTES[T]


def _dev(cuda, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def _run(cuda, qpos, dpos, r, seg_off=None, skip_seg=None, self_item=None):
    from lpdnet_hip import ops
    args = (_dev(cuda, qpos, np.float64), _dev(cuda, dpos, np.float64), r)
    kw = dict(seg_off=seg_off, skip_seg=_dev(cuda, skip_seg, np.int32), self_item=_dev(cuda, self_item, np.int32))
    a = ops.radius_lists(*args, **kw)
    b = ops.radius_lists(*args, **kw)
    torch.cuda.synchronize()
    assert all(x.dtype == torch.int32 and x.is_cuda for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))      # the same bits in every launch
    return tuple(x.cpu().numpy() for x in a)


def _check(got, want, seg_sizes):
    off, idx, counts = got
    woff, widx, wcounts = want
    assert np.array_equal(counts, wcounts), (counts[:16], wcounts[:16])
    assert np.array_equal(off, woff) and np.array_equal(idx, widx)
    assert off[0] == 0 and off[-1] == idx.size and np.array_equal(np.diff(off), counts)
    S = len(seg_sizes)
    rows = np.repeat(np.arange(counts.size), counts)
    assert (idx >= 0).all() and (idx < np.asarray(seg_sizes)[rows % S]).all()      # local to the row's segment
    inner = np.ones(idx.size, dtype=bool)
    inner[off[:-1][counts > 0]] = False      # first entry of every non-empty row
    assert (np.diff(idx)[inner[1:]] > 0).all()      # strictly ascending inside a row


def _queries(dpos, Q, equal):
    """Q query positions for the database dpos: the database itself (Q == D, equal), or items of it moved by a few metres"""
    if equal:
        assert Q == len(dpos)
        return dpos
    g = np.random.default_rng(Q + 31 * len(dpos))
    return dpos[g.integers(0, len(dpos), size=Q)] + g.normal(0.0, 4.0, (Q, 2))


@pytest.mark.parametrize("D", [1, 63, 64, 65, 130, CHUNK + 1, 4097])
def test_one_segment_equals_the_restatement(cuda, D):
    dpos = _route(4097)[:D] if D < 4097 else _route(4097)
    members = 0
    for Q, equal in sorted({(1, D == 1), (1, False), (5, False), (33, False), (D, True), (D, False)}):
        qpos = _queries(dpos, Q, equal)
        for r in (10.0, 50.0):
            want = R.radius_lists(qpos, dpos, r)
            _check(_run(cuda, qpos, dpos, r), want, [D])
            members += int(want[0][-1])
    me = np.arange(D)
    _check(_run(cuda, dpos, dpos, 10.0, self_item=me), R.radius_lists(dpos, dpos, 10.0, self_item=me), [D])      # the positives
    print(f"MEASURE places/one-segment/D{D} members compared {members}")
    assert members > 0


SEG_SIZES = (0, 1, 70, 64, 3)      # an empty segment, a 64-boundary, a last short one


@pytest.mark.parametrize("use_skip", [False, True])
@pytest.mark.parametrize("use_self", [False, True])
def test_segments_skip_and_self(cuda, use_skip, use_self):
    D, Q = sum(SEG_SIZES), 37
    seg = np.concatenate(([0], np.cumsum(SEG_SIZES)))
    dpos = _route(4097)[1000:1000 + D]
    qpos = np.concatenate((dpos[::4], dpos[:2] + 3.0))
    assert len(qpos) == Q
    g = np.random.default_rng(5)
    skip = g.integers(-1, len(SEG_SIZES), size=Q) if use_skip else None      # -1: none
    me = np.concatenate((np.arange(0, D, 4), [-1, D + 5])) if use_self else None      # the item itself; none; outside the table
    for r in (10.0, 50.0, 1e4):
        want = R.radius_lists(qpos, dpos, r, seg_off=seg, skip_seg=skip, self_item=me)
        got = _run(cuda, qpos, dpos, r, seg_off=seg.tolist(), skip_seg=skip, self_item=me)
        _check(got, want, SEG_SIZES)
    counts = got[2].reshape(Q, len(SEG_SIZES))      # r = 1e4 covers everything: full rows but for the refinements
    full = np.tile(SEG_SIZES, (Q, 1))
    if use_self:
        own = np.searchsorted(seg, np.arange(0, D, 4), side="right") - 1
        full[np.arange(len(own)), own] -= 1
    if use_skip:
        full[np.arange(Q)[skip >= 0], skip[skip >= 0]] = 0
    assert np.array_equal(counts, full) and (counts[:, 0] == 0).all()
    rows = R.rows_of(got[0], got[1])
    if not use_skip and not use_self:
        assert rows[2].tolist() == list(range(70)) and rows[4].tolist() == [0, 1, 2]      # local indices, every segment from 0


def test_radii_zero_and_covering(cuda):
    same = np.tile(R.ORIGIN, (130, 1))      # a cloud of identical points: full rows at r = 0
    got = _run(cuda, same[:5], same, 0.0)
    _check(got, R.radius_lists(same[:5], same, 0.0), [130])
    assert got[2].tolist() == [130] * 5
    dpos = _route(4097).copy()
    dpos[100] = dpos[7]      # a coincident pair
    got = _run(cuda, dpos, dpos, 0.0)
    _check(got, R.radius_lists(dpos, dpos, 0.0), [4097])
    assert got[2][7] == 2 and got[2][100] == 2 and got[2].sum() == 4097 + 2
    qpos = _queries(dpos, 33, False)
    got = _run(cuda, qpos, dpos, 1e7)      # a radius that covers everything
    _check(got, R.radius_lists(qpos, dpos, 1e7), [4097])
    assert got[2].tolist() == [4097] * 33 and got[1].max() == 4096 and got[1].size == 33 * 4097


def test_boundary_nan_and_inf_positions(cuda):
    q = R.ORIGIN
    pts = [q]
    for bx, by in ((6.0, 8.0), (8.0, 6.0), (10.0, 0.0)):      # exactly on the circle of r = 10 at UTM magnitude, and one ulp off it
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            p = q + np.array([sx * bx, sy * by])
            pts.append(p)
            for axis in (0, 1):
                for toward in (-np.inf, np.inf):
                    pp = p.copy()
                    pp[axis] = np.nextafter(pp[axis], toward)
                    pts.append(pp)
    dpos = np.array(pts)
    want = R.radius_lists(dpos[:1], dpos, 10.0)
    got = _run(cuda, dpos[:1], dpos, 10.0)
    _check(got, want, [len(dpos)])
    on_circle = 1 + 5 * np.arange(12)
    assert set(on_circle) <= set(got[1].tolist()) and 12 < got[2][0] < len(dpos)      # members; some neighbours are not
    assert np.array_equal(_run(cuda, dpos, dpos[:1], 10.0)[2], np.isin(np.arange(len(dpos)), got[1]).astype(np.int32))      # and the other way round
    # NaN / inf on either side: never members, and the rows around them are what they are without them
    dpos = _route(4097)[:200].copy()
    qpos = dpos[:70].copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        dpos[10 + k, 0] = v
        dpos[63 + k, 1] = v
        dpos[130 + k] = v
        qpos[5 + k, k % 2] = v
    for r in (0.0, 50.0, 1e7):
        want = R.radius_lists(qpos, dpos, r)
        got = _run(cuda, qpos, dpos, r)
        _check(got, want, [200])
        bad = [10, 11, 12, 63, 64, 65, 130, 131, 132]
        assert not np.isin(got[1], bad).any() and (got[2][5:8] == 0).all()
    assert got[2][0] == 200 - len(bad)


def test_membership_is_symmetric(cuda):
    T = 4097
    pos = _route(T)
    off, idx, counts = _run(cuda, pos, pos, 25.0)
    rows = np.repeat(np.arange(T, dtype=np.int64), counts)
    assert np.array_equal(np.sort(rows * T + idx), np.sort(idx.astype(np.int64) * T + rows)) and idx.size > T
    assert (counts >= 1).all()      # every item is within 25 m of itself


def _raw(cuda, lib, which, Q, D, S, r, counts, idx, nnz, qpos=True, dpos=True, seg=True, off=True):
    """one entry point with arguments as given -> (rc, message)"""
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    pos = torch.zeros((8, 2), dtype=torch.float64, device=cuda)
    so = torch.tensor([0, 8], dtype=torch.int32, device=cuda)
    ro = torch.zeros((9,), dtype=torch.int32, device=cuda)
    head = (p(pos) if qpos else None, Q, p(pos) if dpos else None, D, p(so) if seg else None, S, r, None, None)
    if which == "lpd_radius_count":
        rc = lib.lpd_radius_count(*head, p(counts) if counts is not None else None, None)
    else:
        rc = lib.lpd_radius_fill(*head, p(ro) if off else None, p(idx) if idx is not None else None, nnz, None)
    return rc, lib.lpd_last_error().decode()


def test_argument_errors_launch_nothing(cuda):
    from lpdnet_hip import LpdHipError, _lib, ops
    lib = _lib.load()
    counts = torch.full((8,), 7, dtype=torch.int32, device=cuda)
    idx = torch.full((64,), 7, dtype=torch.int32, device=cuda)
    good = dict(Q=8, D=8, S=1, r=10.0, counts=counts, idx=idx, nnz=64)
    bad = [dict(Q=-1), dict(D=-1), dict(Q=(1 << 22) + 1), dict(D=(1 << 22) + 1), dict(S=0), dict(S=-3), dict(S=4097), dict(r=-1.0), dict(r=-1e-300),
           dict(r=float("nan")), dict(r=float("inf")), dict(Q=1 << 22, S=512), dict(Q=1 << 21, S=1024), dict(Q=1 << 22, S=4096),      # Q * S >= 2^31
           dict(qpos=False), dict(dpos=False), dict(seg=False)]
    for kw in bad:
        for which in ("lpd_radius_count", "lpd_radius_fill"):
            rc, msg = _raw(cuda, lib, which, **{**good, **kw})
            assert rc == -1 and msg.startswith(which + ":"), (kw, which, rc, msg)
    rc, msg = _raw(cuda, lib, "lpd_radius_count", **{**good, "counts": None})
    assert rc == -1 and msg.startswith("lpd_radius_count:")
    for kw in (dict(idx=None), dict(nnz=-1), dict(off=False)):
        rc, msg = _raw(cuda, lib, "lpd_radius_fill", **{**good, **kw})
        assert rc == -1 and msg.startswith("lpd_radius_fill:"), (kw, rc, msg)
    torch.cuda.synchronize()
    assert (counts == 7).all() and (idx == 7).all()      # nothing was launched
    pos = torch.zeros((8, 2), dtype=torch.float64, device=cuda)
    for call in (lambda: ops.radius_lists(pos, pos, -1.0), lambda: ops.radius_lists(pos, pos, float("nan")), lambda: ops.radius_lists(pos, pos, float("inf")),
                 lambda: ops.radius_lists(pos, pos, 1.0, seg_off=[0, 5, 3, 8]), lambda: ops.radius_lists(pos, pos, 1.0, seg_off=[0, 7]),
                 lambda: ops.radius_lists(pos, pos, 1.0, seg_off=[1, 8]), lambda: ops.radius_lists(pos, pos, 1.0, seg_off=[0]),
                 lambda: ops.radius_lists(pos, pos, 1.0, seg_off=[0] * 4097 + [8]), lambda: ops.radius_lists(pos.view(-1), pos, 1.0),
                 lambda: ops.radius_lists(pos, pos[:, :1], 1.0), lambda: ops.radius_lists(pos, pos, 1.0, skip_seg=torch.zeros(7, dtype=torch.int32, device=cuda)),
                 lambda: ops.radius_lists(pos, pos, 1.0, self_item=torch.zeros((8, 1), dtype=torch.int32, device=cuda))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.radius_lists(pos.float(), pos, 1.0)
    with pytest.raises(TypeError):
        ops.radius_lists(pos, pos, 1.0, skip_seg=torch.zeros(8, dtype=torch.int64, device=cuda))
    with pytest.raises(LpdHipError):
        ops.radius_lists(pos.cpu(), pos, 1.0)
    # empty sides are legal: no rows, or rows without entries
    off, ix, cnt = ops.radius_lists(pos[:0], pos, 1.0)
    assert off.tolist() == [0] and ix.numel() == 0 and cnt.numel() == 0
    off, ix, cnt = ops.radius_lists(pos, pos[:0], 1.0)
    assert off.tolist() == [0] * 9 and ix.numel() == 0 and cnt.tolist() == [0] * 8
    # a row_off that is not the scan of the counts writes nothing outside idx
    small = torch.full((4,), 7, dtype=torch.int32, device=cuda)
    guard = torch.tensor([0, 2, 2, 2, 2, 2, 2, 2, 2], dtype=torch.int32, device=cuda)      # rows of one entry where eight belong
    so = torch.tensor([0, 8], dtype=torch.int32, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.lpd_radius_fill(p(pos), 8, p(pos), 8, p(so), 1, 1.0, None, None, p(guard), p(small), 2, None) == 0
    torch.cuda.synchronize()
    assert small[2:].tolist() == [7, 7] and set(small[:2].tolist()) <= {0, 1, 2, 3, 4, 5, 6, 7}


# ---- TupleBank.from_positions ------------------------------------------------------------------------------------------------------
T_BANK, N_BANK, P_, NG = 300, 256, 2, 18


def test_bank_from_positions_equals_bank_from_lists(cuda):
    from lpdnet_hip import tuples
    clouds = np.random.default_rng(5).uniform(-1, 1, size=(T_BANK, N_BANK, 3))      # float64: narrowed on the device
    positions = np.stack((R.ORIGIN[0] + 2.0 * np.arange(T_BANK), np.full(T_BANK, R.ORIGIN[1])), 1)      # places on a line, 2 m apart
    positives, near = R.training_lists(positions, 10.0, 50.0)
    assert positives[150].tolist() == [j for j in range(145, 156) if j != 150] and len(near[150]) == 51 and near[0].tolist() == list(range(26))
    a = tuples.TupleBank.from_positions(clouds, positions, device=cuda)
    b = tuples.TupleBank(clouds, positives, near, device=cuda)
    for name in ("pos_off", "pos_idx", "near_off", "near_idx", "table"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), name
    assert a.pos_len.dtype == b.pos_len.dtype and np.array_equal(a.pos_len, b.pos_len) and np.array_equal(a.near_len, b.near_len)
    assert (a.T, a.N, a.max_pos, a.max_near) == (b.T, b.N, b.max_pos, b.max_near) == (T_BANK, N_BANK, 10, 51)
    queries = [0, 150, 299, 150]
    assert torch.equal(a.sample(queries, P_, NG, seed=4), b.sample(queries, P_, NG, seed=4))
    assert torch.equal(a.candidates(queries, 100, seed=2), b.candidates(queries, 100, seed=2))
    items = a.sample(queries, P_, NG, seed=9)
    assert torch.equal(a.assemble(items, rotate=True, jitter=True, seed=3), b.assemble(items, rotate=True, jitter=True, seed=3))
    c = tuples.TupleBank.from_positions(clouds, torch.from_numpy(positions).to(cuda), pos_radius=4.0, near_radius=6.0)      # device positions, other radii
    assert c.device == cuda and (c.max_pos, c.max_near) == (4, 7)
    with pytest.raises(ValueError):
        tuples.TupleBank.from_positions(clouds, positions[:-1], device=cuda)
    with pytest.raises(ValueError):
        a.sample(queries, 11, NG, seed=0)      # at most 10 positives


# ---- evaluation_truth ----------------------------------------------------------------------------------------------------------------
def _three_runs():
    from lpdnet_hip import places
    road = R.route(222, seed=9)
    db = [road[0:40] + 1.0, road[20:160:2] - 2.0, road[30:31] + 0.5]
    centres = [road[25], road[110]]
    return db, [d[places.in_test_regions(d, centres, 60, 60)] for d in db]


def _reference_query_sets(db, qs):
    """generate_test_sets.py:71-109 restated: a KDTree per database run, every query of run j searched in run i != j at r = 25"""
    from sklearn.neighbors import KDTree
    trees = [KDTree(d) for d in db]
    test_sets = [{k: {} for k in range(len(q))} for q in qs]
    for i in range(len(db)):
        for j in range(len(qs)):
            if i == j:
                continue
            for key in range(len(qs[j])):
                index = trees[i].query_radius(np.array([[qs[j][key][0], qs[j][key][1]]]), r=25)
                test_sets[j][key][i] = index[0].tolist()
    return test_sets


def test_evaluation_truth_equals_the_reference_recipe(cuda):
    from lpdnet_hip import harness, places
    db, qs = _three_runs()
    assert [len(d) for d in db] == [40, 70, 1] and all(1 <= len(q) for q in qs) and len(qs[0]) < 40 and len(qs[1]) < 70
    table = places.evaluation_truth(db, qs, device=cuda)
    torch.cuda.synchronize()
    assert table.truth_off.is_cuda and table.truth_off.dtype == torch.int32 and table.truth_idx.dtype == torch.int32
    assert len(table) == 3 and table.n_db_runs == 3 and table.q_counts == [len(q) for q in qs] and table.radius == 25.0
    sets = _reference_query_sets(db, qs)
    pairs = harness.all_pairs(3)
    woff, widx = harness.build_truth_csr(sets, table.q_counts, 3, pairs)
    widx_sorted = np.concatenate([np.sort(widx[woff[i]:woff[i + 1]]) for i in range(len(woff) - 1)])      # KDTree's lists are unordered
    off, idx = table.truth_off.cpu().numpy(), table.truth_idx.cpu().numpy()
    assert np.array_equal(off, woff) and np.array_equal(idx, widx_sorted) and idx.size > 0
    roff, ridx = R.truth_table(db, qs, 25.0)
    assert np.array_equal(off, roff) and np.array_equal(idx, ridx)
    back = table.to_query_sets()
    assert all(sorted(back[n][i][m]) == sorted(sets[n][i][m]) for n in range(3) for i in range(len(qs[n])) for m in range(3) if m != n)
    # the table goes where QUERY_SETS went
    g = np.random.default_rng(11)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)      # noqa: E731
    dvec = [unit(g.standard_normal((len(d), 256))) for d in db]
    qvec = [unit(g.standard_normal((len(q), 256))) for q in qs]
    want = harness.evaluate_pairs(dvec, qvec, sets, device=cuda)
    got = harness.evaluate_pairs(dvec, qvec, table, device=cuda)
    assert len(got) == len(want) == 6
    for (gr, gs, go), (wr, ws, wo) in zip(got, want):
        assert np.array_equal(gr, wr) and gs == ws and go == wo
    assert harness.evaluate_from_descriptors(dvec, qvec, table, device=cuda) == harness.evaluate_from_descriptors(dvec, qvec, sets, device=cuda)
    sub = pairs[[0, 3]]
    assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(harness.evaluate_pairs(dvec, qvec, table, pairs=sub, device=cuda),
                                                                               harness.evaluate_pairs(dvec, qvec, sets, pairs=sub, device=cuda)))
    with pytest.raises(ValueError):
        harness.evaluate_pairs(dvec, qvec[:2] + [np.concatenate((qvec[2], qvec[2]))], table, device=cuda)      # descriptors of other run sizes
    with pytest.raises(ValueError):
        places.evaluation_truth(db, qs[:2], device=cuda)


# ---- one larger case with the launch times ------------------------------------------------------------------------------------------
def test_measure_route_of_8192(cuda):
    from lpdnet_hip import _lib, ops
    T = 8192
    pos = _route(T)
    dpos = _dev(cuda, pos, np.float64)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    seg = torch.tensor([0, T], dtype=torch.int32, device=cuda)
    for r in (10.0, 50.0):
        want = R.radius_lists(pos, pos, r)
        got = _run(cuda, pos, pos, r)
        _check(got, want, [T])
        off, idx = _dev(cuda, got[0]), torch.empty((got[1].size,), dtype=torch.int32, device=cuda)
        counts = torch.empty((T,), dtype=torch.int32, device=cuda)
        head = (p(dpos), T, p(dpos), T, p(seg), 1, r, None, None)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for rep in range(2):      # the second trip is the timed one
            ev[0].record()
            assert lib.lpd_radius_count(*head, p(counts), ops._stream()) == 0
            ev[1].record()
            assert lib.lpd_radius_fill(*head, p(off), p(idx), idx.numel(), ops._stream()) == 0
            ev[2].record()
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want[2]) and np.array_equal(idx.cpu().numpy(), want[1])
        print(f"MEASURE places/route/T{T}/r{r:g} entries {got[1].size} longest row {got[2].max()} count {ev[0].elapsed_time(ev[1]) * 1e3:.1f} us "
              f"fill {ev[1].elapsed_time(ev[2]) * 1e3:.1f} us")
