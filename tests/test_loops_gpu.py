"""lpd_loop_consistency and lpd_loop_select on the device against the numpy restatement (tests/loops_ref.py), equal in every bit --
adj, degree, accepted and info -- at the loop counts around the wave (64 lanes = one word) and the workgroup (256 threads), the
conditions and gates of tests/test_loops_cpu.py on the device's result, and posegraph.close_loops(consistent=True) end to end on a small
synthetic drive with one loop's measurement replaced by a gross one."""
import copy

import numpy as np
import pytest
import torch

import align_ref as AR
import loops_ref as L
import pgo_ref as R
from test_loops_cpu import ATE_RATIO_GATE, HAND_CASES, SIZE_SHARE_GATE
from lpdnet_hip import LpdHipError, consistency, drive, ops, posegraph, verify

pytestmark = pytest.mark.gpu


def _up(dev, a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def _consistency(dev, pose, edge, meas, weight, w, gate=L.GATE, **kw):
    adj, degree = ops.loop_consistency(_up(dev, pose, np.float64).reshape(-1, 12), _up(dev, edge, np.int32).reshape(-1, 2),
                                       _up(dev, meas, np.float64).reshape(-1, 12), _up(dev, weight, np.float64).reshape(-1, 2), w[0], w[1], gate, **kw)
    return adj, degree


def _select(dev, adj, degree, **kw):
    if not isinstance(adj, torch.Tensor):
        adj, degree = _up(dev, np.ascontiguousarray(adj, dtype=np.uint64).view(np.int64), np.int64), _up(dev, degree, np.int32)
    accepted, info = ops.loop_select(adj, degree, **kw)
    torch.cuda.synchronize()
    return accepted.cpu().numpy(), info.cpu().numpy()


def _host(adj, degree):
    return adj.cpu().numpy().view(np.uint64), degree.cpu().numpy()


def _equal(got, want, what):
    for name, g, w in zip(("adj", "degree", "accepted", "info"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _both(dev, pose, edge, meas, weight, w, what, gate=L.GATE, node_off=None, loop_off=None, ldw=None, seeds=8, min_size=3):
    adj, degree = _consistency(dev, pose, edge, meas, weight, w, gate, node_off=node_off, loop_off=loop_off, ldw=ldw)
    accepted, info = _select(dev, adj, degree, loop_off=loop_off, seeds=seeds, min_size=min_size)
    got = _host(adj, degree) + (accepted, info)
    want = L.consistency(pose, edge, meas, weight, w[0], w[1], gate, node_off=node_off, loop_off=loop_off, ldw=ldw)
    want += L.select(want[0], want[1], loop_off=loop_off, seeds=seeds, min_size=min_size)
    _equal(got, want, what)
    return got


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025])
def test_loop_counts_around_the_word_and_the_workgroup(cuda, P):
    start, edge, meas, weight, w = L.drive_loops(P, 12 + P // 16, P)
    adj, degree, accepted, info = _both(cuda, start, edge, meas, weight, w, f"P={P}", min_size=1)
    M = L.unpack(adj, P)
    assert (M == M.T).all() and not M.diagonal().any() and adj.shape == (P, -(-P // 64)) and (degree == M.sum(axis=1)).all()
    assert info[0, 0] == L.OK and info[0, 1] == P and info[0, 2] == accepted.sum() >= (2 if P > 2 else 1)
    if P >= 63:
        assert 0.1 < M.mean() < 0.9      # neither empty nor full: both outcomes of the gate are on the device


def test_a_stride_larger_than_needed(cuda):
    start, edge, meas, weight, w = L.drive_loops(3, 16, 65)
    wide = _both(cuda, start, edge, meas, weight, w, "ldw=5", ldw=5)
    tight = _both(cuda, start, edge, meas, weight, w, "ldw=2")
    assert wide[0].shape == (65, 5) and not wide[0][:, 2:].any() and (wide[0][:, :2] == tight[0]).all()
    assert (wide[2] == tight[2]).all() and (wide[3] == tight[3]).all()


# ---- the selection alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seeds", [1, 8, 64])
@pytest.mark.parametrize("density", [0.1, 0.9])
def test_selection_alone_on_random_matrices_at_the_largest_size(cuda, density, seeds):
    adj, degree = L.random_matrix(11, L.MAX_LOOPS, density)
    got = _select(cuda, adj, degree, seeds=seeds, min_size=1)
    want = L.select(adj, degree, seeds=seeds, min_size=1)
    _equal((adj, degree) + got, (adj, degree) + want, f"density={density} seeds={seeds}")
    chosen = got[0].astype(bool)
    M = L.unpack(adj, L.MAX_LOOPS)
    assert got[1][0, 3] == seeds and M[np.ix_(chosen, chosen)].sum() == chosen.sum() * (chosen.sum() - 1)
    assert L.is_maximal(M, chosen, np.ones(L.MAX_LOOPS, dtype=bool))


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_selection_on_hand_written_matrices(cuda, case):
    name, adj, degree, kw, accepted, info = case
    got = _select(cuda, adj, np.asarray(degree, dtype=np.int32), **kw)
    assert got[0].tolist() == accepted and got[1].tolist() == info, name


# ---- several graphs, skipped loops, bad numbers ----------------------------------------------------------------------------------------
def test_three_graphs_one_of_them_empty(cuda):
    parts = [L.drive_loops(21, 14, 30), L.drive_loops(22, 40, 300)]
    pose, edge, meas, weight = (np.concatenate((parts[0][k], parts[1][k])) for k in range(4))
    node_off, loop_off = [0, 14, 14, 54], [0, 30, 30, 330]
    got = _both(cuda, pose, edge, meas, weight, parts[0][4], "G=3", node_off=node_off, loop_off=loop_off)
    assert got[0].shape == (330, 5) and got[3][1].tolist() == [L.NOTHING, 0, 0, 0, -1, 0, 0, 0] and got[3][0, 0] == got[3][2, 0] == L.OK
    alone = _both(cuda, *parts[0][:4], parts[0][4], "the first alone")
    assert (alone[0][:, 0] == got[0][:30, 0]).all() and not got[0][:30, 1:].any() and (alone[1] == got[1][:30]).all()
    assert (alone[2] == got[2][:30]).all() and (alone[3][0] == got[3][0]).all()
    # device offsets are taken as they are
    dev_off = dict(node_off=torch.tensor(node_off, dtype=torch.int32, device=cuda), loop_off=torch.tensor(loop_off, dtype=torch.int32, device=cuda))
    adj, degree = _consistency(cuda, pose, edge, meas, weight, parts[0][4], ldw=5, **dev_off)
    accepted, info = _select(cuda, adj, degree, loop_off=dev_off["loop_off"])
    _equal(_host(adj, degree) + (accepted, info), got, "device offsets")


def test_every_kind_of_skipped_loop(cuda):
    start, edge, meas, weight, w = L.drive_loops(23, 12, 24)
    n = 24
    edge, meas, weight = (np.concatenate((a, a[:10])) for a in (edge, meas, weight))
    edge[n] = (3, 12)              # out of range
    edge[n + 1] = (-1, -1)         # what loop_edges writes for a pair that is not accepted
    edge[n + 2] = (7, 7)           # i == j
    meas[n + 3, 5] = np.nan
    meas[n + 4, 11] = np.inf
    weight[n + 5, 0] = np.nan
    weight[n + 6, 1] = -1.0
    weight[n + 7, 1] = np.inf
    weight[n + 8, 0] = 0.0         # a zero weight is no variance
    weight[n + 9, 1] = 0.0
    place = np.random.default_rng(1).permutation(n + 10)      # the skipped loops anywhere among the others, which keep their order
    good, bad = np.sort(place[:n]), np.sort(place[n:])
    order = np.empty(n + 10, dtype=np.int64)
    order[good], order[bad] = np.arange(n), np.arange(n, n + 10)
    got = _both(cuda, start, edge[order], meas[order], weight[order], w, "skipped")
    clean = _both(cuda, start, edge[:n], meas[:n], weight[:n], w, "clean")
    assert (got[1][bad] == -1).all() and not got[0][bad].any() and not got[2][bad].any()
    assert (got[2][good] == clean[2]).all() and (got[1][good] == clean[1]).all() and clean[2].sum() >= 3
    assert got[3][0].tolist() == [L.OK, n, int(clean[2].sum()), 8, int(good[clean[3][0, 4]]), int(clean[3][0, 5]), 0, 0]


def test_a_nan_node_pose(cuda):
    start, edge, meas, weight, w = L.drive_loops(24, 12, 40)
    start = start.copy()
    start[5, 7] = np.nan
    got = _both(cuda, start, edge, meas, weight, w, "nan pose")
    touched = (edge == 5).any(axis=1)
    assert touched.any() and (got[1][touched] == 0).all() and not got[2][touched].any() and got[3][0, 1] == 40


def test_a_graph_over_the_stride(cuda):
    parts = [L.drive_loops(25, 10, 130), L.drive_loops(26, 10, 20)]
    pose, edge, meas, weight = (np.concatenate((parts[0][k], parts[1][k])) for k in range(4))
    got = _both(cuda, pose, edge, meas, weight, parts[0][4], "TOO_MANY", node_off=[0, 10, 20], loop_off=[0, 130, 150], ldw=2)
    assert got[3][0].tolist() == [L.TOO_MANY, 0, 0, 0, -1, 0, 0, 0] and not got[0][:130].any() and (got[1][:130] == -1).all() and not got[2][:130].any()
    assert got[3][1, 0] == L.OK and got[2][130:].sum() == got[3][1, 2] >= 3
    adj, degree = L.random_matrix(12, 130, 0.5)      # the selection alone: 130 loops under a stride of 3 words run, under 2 they do not
    assert _select(cuda, adj, degree)[1][0, 0] == L.OK
    assert _select(cuda, adj[:, :2].copy(), degree)[1][0].tolist() == [L.TOO_MANY, 0, 0, 0, -1, 0, 0, 0]


def test_repeatable_and_two_streams(cuda):
    start, edge, meas, weight, w = L.drive_loops(27, 30, 300)
    one = _both(cuda, start, edge, meas, weight, w, "first")
    two = _both(cuda, start, edge, meas, weight, w, "second")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    args = (_up(cuda, start, np.float64), _up(cuda, edge, np.int32), _up(cuda, meas, np.float64), _up(cuda, weight, np.float64))
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream(), torch.cuda.Stream()], []
    for s in streams:
        with torch.cuda.stream(s):
            adj, degree = ops.loop_consistency(*args, w[0], w[1], L.GATE)      # its own outputs and workspace
            outs.append((adj, degree) + ops.loop_select(adj, degree))
    torch.cuda.synchronize()
    for adj, degree, accepted, info in outs:
        _equal(_host(adj, degree) + (accepted.cpu().numpy(), info.cpu().numpy()), one, "stream")


def test_argument_errors(cuda):
    start, edge, meas, weight, w = L.drive_loops(28, 8, 6)
    p, e, m, wt = _up(cuda, start, np.float64), _up(cuda, edge, np.int32), _up(cuda, meas, np.float64), _up(cuda, weight, np.float64)
    with pytest.raises(ValueError):
        ops.loop_consistency(p, e, m[:, :11], wt, *w, L.GATE)
    with pytest.raises(LpdHipError):      # one tensor left on the host
        ops.loop_consistency(p, e, m, wt.cpu(), *w, L.GATE)
    with pytest.raises(LpdHipError):
        ops.loop_select(torch.zeros((6, 1), dtype=torch.int64), torch.zeros(6, dtype=torch.int32, device=cuda))
    lib, ptr = ops._lib.load(), ops._ptr
    noff, loff = torch.tensor([0, 8], dtype=torch.int32, device=cuda), torch.tensor([0, 6], dtype=torch.int32, device=cuda)
    adj, deg = torch.full((6, 2), -1, dtype=torch.int64, device=cuda), torch.full((6,), 77, dtype=torch.int32, device=cuda)
    acc, info = torch.full((6,), 9, dtype=torch.uint8, device=cuda), torch.full((1, 8), 9, dtype=torch.int32, device=cuda)
    ws = torch.empty(int(lib.lpd_loop_select_workspace_bytes(1, 8, 2)), dtype=torch.uint8, device=cuda)
    assert lib.lpd_loop_select_workspace_bytes(1, 8, 2) == 8 * (8 * 2 + 8) + 16
    assert lib.lpd_loop_select_workspace_bytes(0, 8, 2) == 0 and lib.lpd_loop_select_workspace_bytes(1, 65, 2) == 0 and lib.lpd_loop_select_workspace_bytes(1, 8, 65) == 0

    def cons(**kw):
        a = dict(pose=ptr(p), node_off=ptr(noff), V=8, edge=ptr(e), meas=ptr(m), weight=ptr(wt), loop_off=ptr(loff), P=6, G=1, w_or=w[0], w_ot=w[1],
                 gate=L.GATE, adj=ptr(adj), ldw=2, degree=ptr(deg))
        a.update(kw)
        return lib.lpd_loop_consistency(*a.values(), None)

    def sel(**kw):
        a = dict(adj=ptr(adj), ldw=2, degree=ptr(deg), loop_off=ptr(loff), P=6, G=1, seeds=8, min_size=3, accepted=ptr(acc), info=ptr(info), ws=ptr(ws))
        a.update(kw)
        return lib.lpd_loop_select(*a.values(), None)
    for kw in (dict(pose=None), dict(adj=None), dict(degree=None), dict(loop_off=None), dict(node_off=None), dict(G=0), dict(G=65536), dict(V=-1), dict(P=-1),
               dict(ldw=0), dict(ldw=65), dict(w_or=0.0), dict(w_ot=-1.0), dict(w_or=float("nan")), dict(w_ot=float("inf")), dict(gate=-1.0),
               dict(gate=float("nan")), dict(gate=float("inf"))):
        assert cons(**kw) != 0, kw
        assert b"lpd_loop_consistency" in lib.lpd_last_error(), kw
    for kw in (dict(adj=None), dict(degree=None), dict(accepted=None), dict(info=None), dict(ws=None), dict(loop_off=None), dict(G=0), dict(P=-1), dict(ldw=0),
               dict(ldw=65), dict(seeds=0), dict(seeds=65), dict(min_size=0)):
        assert sel(**kw) != 0, kw
        assert b"lpd_loop_select" in lib.lpd_last_error(), kw
    torch.cuda.synchronize()
    assert (adj == -1).all() and (deg == 77).all() and (acc == 9).all() and (info == 9).all()      # a refused call writes nothing
    assert cons() == 0 and sel() == 0
    torch.cuda.synchronize()
    want = L.consistency(start, edge, meas, weight, w[0], w[1], L.GATE, ldw=2)
    want += L.select(want[0], want[1], seeds=8, min_size=3)
    _equal(_host(adj, deg) + (acc.cpu().numpy(), info.cpu().numpy()), want, "C entry")


# ---- quality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.QUALITY_CASES)
def test_quality_conditions_on_the_device(cuda, case):
    q = L.quality_case(*case)
    g, (edge, meas, weight), w = q["graph"], q["loops"], q["w"]
    adj, degree = _consistency(cuda, g["start"], edge, meas, weight, w)
    accepted, info = _select(cuda, adj, degree, seeds=L.SEEDS, min_size=L.MIN_SIZE)
    adj, degree = _host(adj, degree)
    _equal((adj, degree, accepted, info), (q["adj"], q["degree"], q["accepted"], q["info"]), f"quality {case}")
    acc, gross, M = accepted.astype(bool), q["gross"], L.unpack(adj, len(edge))
    ate = q["ate_chosen"]      # the device's set is the restatement's, bit for bit: so is the solve of it
    share, ratio = acc.sum() / len(L.max_clique(M)), ate / q["ate_true"]
    print(f"MEASURE loops device case={case}: chosen {int(acc.sum())} false {int((acc & gross).sum())}; size share {share:.4f}; ATE start {q['ate_start']:.3f} "
          f"all loops huber=3 {q['ate_all_huber']:.3f} chosen {ate:.3f} = {ratio:.4f} of the true loops'")
    assert not (acc & gross).any() and L.is_maximal(M, acc, degree >= 0)
    assert ate < q["ate_start"] and ate < q["ate_all_huber"]
    assert SIZE_SHARE_GATE <= share <= 1.0 and ratio <= ATE_RATIO_GATE


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_close_loops_end_to_end_with_a_gross_loop(cuda):
    """The drive of tests/test_posegraph_gpu.py's end-to-end test: two laps of a circle of 80 m through a street scene, windows of 20 m
    every 10 m, each window of the second lap paired with the window one lap earlier, aligned and refined on the device.  One loop's
    refined pose is then moved by metres: close_loops(consistent=True) must reject it, its solve must be the restatement's solve of the
    filtered graph, and where the selection keeps every loop the poses must be those of plain close_loops bit for bit."""
    sc = AR.scene(3, extent=40.0)
    g = np.random.default_rng(21)
    S, radius, n = 81, 80.0 / (2.0 * np.pi), 1024
    th = np.arange(S) * (2.0 / radius)
    true = np.array([R.pose12(R.yaw_rot(t + np.pi / 2), [radius * np.cos(t), radius * np.sin(t), 0.0]) for t in th])
    pts = np.concatenate([AR.submap(sc, true[s].reshape(3, 4)[:2, 3], th[s] + np.pi / 2, 100 + s, n=n) for s in range(S)])
    drifted = [true[0]]
    for s in range(S - 1):
        step = R.mul12(R.inv12(true[s]), true[s + 1])
        drifted.append(R.mul12(drifted[-1], R.mul12(step, R.pose12(R.yaw_rot(g.normal(0.002, 0.002)), [g.normal(0, 0.01), g.normal(0.01, 0.01), 0.0]))))
    drifted = np.array(drifted)
    sub, _ = drive.submaps_from_drive(torch.from_numpy(pts), [n] * S, drifted, 20.0, 10.0, num_points=2048, device=cuda)
    W, lap = len(sub.plan), 8
    pairs = torch.tensor([[w, w - lap] for w in range(lap, W)], dtype=torch.int32, device=cuda)
    rf = verify.refine_pairs(sub, sub, pairs, init=verify.align_pairs(sub, sub, pairs))
    assert len(pairs) >= 5 and rf.valid.all()
    solver = dict(outer=12, cg_iters=60)
    nodes = drifted[sub.plan.ref.cpu().numpy()]
    od = posegraph.odometry_edges(torch.from_numpy(nodes).to(cuda))

    def restated(res, loops, search):
        """the restatement of the selection and of the solve of the filtered graph, against what close_loops returned"""
        edge, meas, weight = (t.cpu().numpy() for t in loops)
        want = L.consistency(nodes, edge, meas, weight, *posegraph.ODOMETRY_WEIGHTS, search.gate)
        want += L.select(want[0], want[1], seeds=search.seeds, min_size=search.min_size)
        sel = res.selection
        _equal(_host(sel.adjacency, sel.degree) + (sel.accepted.cpu().numpy().astype(np.uint8), sel.info[None].cpu().numpy()), want, "selection")
        kept = np.where(want[2].astype(bool)[:, None], edge, -1).astype(np.int32)
        e, m, w = (np.concatenate((a.cpu().numpy(), b)) for a, b in zip(od, (kept, meas, weight)))
        pose, cost, chi, info = R.solve(nodes, e, m, w, **solver)
        assert res.poses.reshape(-1, 12).cpu().numpy().tobytes() == pose.tobytes() and res.cost.cpu().numpy().tobytes() == cost[0].tobytes()
        assert (res.info.cpu().numpy() == info[0]).all() and (res.chi2.cpu().numpy()[len(od[0]):][~want[2].astype(bool)] == -1.0).all()
        return want

    # one loop's measurement is replaced by a gross one
    k = 2
    bad = copy.copy(rf)
    bad.pose = rf.pose.clone()
    bad.pose[k, 0, 3] += 9.0
    bad.pose[k, 1, 3] -= 7.0
    res = posegraph.close_loops(sub, drifted, bad, pairs, consistent=True, **solver)
    torch.cuda.synchronize()
    want = restated(res, posegraph.loop_edges(bad, pairs), consistency.ConsistencySearch())
    assert not res.selection.accepted[k] and res.selection.accepted.sum() >= 3 and bool(res.selection.ok) and int(res.info[5]) == int((want[2] == 0).sum())
    plain = posegraph.close_loops(sub, drifted, bad, pairs, **solver)
    ref = sub.plan.ref.cpu().numpy()
    ate = [R.ate(p.poses.reshape(-1, 12).cpu().numpy(), true[ref]) for p in (res, plain)]
    print(f"MEASURE loops close_loops: W={W} loops={len(pairs)} kept {int(res.selection.accepted.sum())}; ATE start {R.ate(nodes, true[ref]):.3f} m, with the "
          f"gross loop {ate[1]:.3f} m, with the selection {ate[0]:.3f} m; selection info {res.selection.info.cpu().tolist()}")
    assert plain.selection is None and ate[0] < ate[1]
    # a gate that every loop passes: the selection keeps them all, and the solve is plain close_loops bit for bit
    everything = consistency.ConsistencySearch(gate=1e12, seeds=1, min_size=1)
    res = posegraph.close_loops(sub, drifted, rf, pairs, consistent=everything, **solver)
    plain = posegraph.close_loops(sub, drifted, rf, pairs, **solver)
    torch.cuda.synchronize()
    restated(res, posegraph.loop_edges(rf, pairs), everything)
    assert res.selection.accepted.all() and int(res.selection.info[2]) == len(pairs)
    for a, b in ((res.poses, plain.poses), (res.cost, plain.cost), (res.chi2, plain.chi2), (res.info, plain.info)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
