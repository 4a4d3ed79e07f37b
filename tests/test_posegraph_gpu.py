"""lpd_pgo_solve on the device against the numpy restatement (tests/pgo_ref.py) bit for bit -- pose, cost, chi2 and info -- at the
smallest sizes that reach each path of the kernel (the workgroup has 256 threads, a wave 64 lanes), the quality gates of
tests/test_posegraph_cpu.py on the device's result, and posegraph.close_loops end to end on a small synthetic drive."""
import numpy as np
import pytest
import torch

import align_ref as AR
import pgo_ref as R
from test_posegraph_cpu import ATE_GATE, OUTLIER_CASE, QUALITY_CASES, RATIO_CASES, RATIO_GATE
from lpdnet_hip import LpdHipError, drive, ops, posegraph, verify

pytestmark = pytest.mark.gpu

SOLVER = dict(outer=4, cg_iters=12, cg_tol=1e-6, lambda0=1e-4)


def _gpu(dev, pose, edge, meas, weight, fixed=None, node_off=None, edge_off=None, **kw):
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    out = ops.pgo_solve(up(pose, np.float64), up(edge, np.int32).reshape(-1, 2), up(meas, np.float64).reshape(-1, 12), up(weight, np.float64).reshape(-1, 2),
                        fixed=None if fixed is None else up(fixed, np.uint8), node_off=node_off, edge_off=edge_off, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _equal(got, want, what=""):
    for name, g, w in zip(("pose", "cost", "chi2", "info"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w).astype(g.dtype)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1)
        if g.dtype == np.float64:
            bad = bad.reshape(-1, 8).any(axis=1) & ~(np.isnan(g).reshape(-1) & np.isnan(w).reshape(-1))
        assert not bad.any(), (what, name, np.flatnonzero(bad)[:6], g.reshape(-1)[:8], w.reshape(-1)[:8])


def _both(dev, pose, edge, meas, weight, what="", **kw):
    got = _gpu(dev, pose, edge, meas, weight, **kw)
    want = R.solve(pose, edge, meas, weight, **kw)
    _equal(got, want, what)
    return got


def _chain(seed, V, loops=0, hub=0):
    """a noisy chain of V nodes with `loops` random extra edges and `hub` edges from node 0 to the last `hub` nodes"""
    g = np.random.default_rng(seed)
    gt = [R.pose12(np.eye(3), [0.0, 0.0, 0.0])]
    for k in range(V - 1):
        gt.append(R.mul12(gt[-1], R.pose12(R.rot_of(g.normal(0, 0.2, 3)), [2.0 + g.normal(0, 0.3), g.normal(0, 0.3), g.normal(0, 0.1)])))
    gt = np.array(gt)
    pairs = [(k, k + 1) for k in range(V - 1)]
    for _ in range(loops):
        i, j = g.choice(V, 2, replace=False)
        pairs.append((int(i), int(j)))
    pairs += [(0, V - 1 - k) if k % 2 else (V - 1 - k, 0) for k in range(hub)]
    meas = np.array([R.mul12(R.mul12(R.inv12(gt[i]), gt[j]), R.pose12(R.rot_of(g.normal(0, 0.01, 3)), g.normal(0, 0.05, 3))) for i, j in pairs]).reshape(-1, 12)
    start = np.array([gt[0]] + [R.mul12(x, R.pose12(R.rot_of(g.normal(0, 0.03, 3)), g.normal(0, 0.3, 3))) for x in gt[1:]])
    weight = np.tile(np.array([[1e4, 4e2]]), (len(pairs), 1)) * g.uniform(0.5, 2.0, (len(pairs), 1))
    return start, np.array(pairs, dtype=np.int32).reshape(-1, 2), meas, weight


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 3, 255, 256, 257])
def test_node_counts_around_the_workgroup(cuda, V):
    start, edge, meas, weight = _chain(V, V, loops=min(V // 4, 40) if V > 2 else 0)
    got = _both(cuda, start, edge, meas, weight, f"V={V}", **SOLVER)
    if V == 1:
        assert got[3][0].tolist() == [R.NOTHING, 0, 0, 0, 0, 0, 0, 0]
    else:
        assert got[3][0, 1] >= 1 and got[1][0, -1] < got[1][0, 0] and got[3][0, 6] == V - 1


def test_degree_above_the_wave_width_and_an_isolated_node(cuda):
    start, edge, meas, weight = _chain(11, 90, loops=10, hub=70)      # node 0 has 71 edges
    edge = edge.copy()
    edge[edge == 40] = 41                                             # node 40 loses every edge (the chain skips over it)
    edge[39] = (39, 41)
    assert np.bincount(edge.reshape(-1))[0] > 64 and 40 not in edge
    fixed = np.zeros(90, np.uint8)
    fixed[5] = 1                                                      # the gauge is not node 0: the hub moves
    got = _both(cuda, start, edge, meas, weight, "hub", fixed=fixed, **SOLVER)
    assert got[0][40].tobytes() == start[40].tobytes() and got[0][5].tobytes() == start[5].tobytes()
    assert got[3][0, 6] == 88 and got[3][0, 1] >= 1


def test_all_nodes_fixed_and_outer_zero(cuda):
    start, edge, meas, weight = _chain(12, 20, loops=5)
    got = _both(cuda, start, edge, meas, weight, "fixed", fixed=np.ones(20, np.uint8), **SOLVER)
    assert got[3][0, 0] == R.NOTHING and got[0].tobytes() == start.tobytes() and (got[2] >= 0).all()
    got = _both(cuda, start, edge, meas, weight, "outer=0", outer=0)
    assert got[3][0, 0] == R.ITERATIONS and got[0].tobytes() == start.tobytes() and got[1].shape == (1, 1)


def test_three_graphs_one_of_them_empty(cuda):
    parts = [_chain(13, 30, loops=6), _chain(14, 300, loops=30)]
    pose = np.concatenate((parts[0][0], parts[1][0]))
    edge = np.concatenate((parts[0][1], parts[1][1]))
    meas = np.concatenate((parts[0][2], parts[1][2]))
    weight = np.concatenate((parts[0][3], parts[1][3]))
    node_off, edge_off = [0, 30, 30, 330], [0, len(parts[0][1]), len(parts[0][1]), len(edge)]
    fixed = np.zeros(330, np.uint8)
    fixed[30 + 7] = 1
    got = _both(cuda, pose, edge, meas, weight, "G=3", fixed=fixed, node_off=node_off, edge_off=edge_off, **SOLVER)
    assert got[3][1].tolist() == [R.NOTHING, 0, 0, 0, 0, 0, 0, 0] and (got[1][1] == 0.0).all()
    # a graph of a batch is the graph alone
    alone = _gpu(cuda, *parts[0], **SOLVER)
    assert alone[0].tobytes() == got[0][:30].tobytes() and alone[1][0].tobytes() == got[1][0].tobytes()
    # device offsets are taken as they are
    dev_off = _gpu(cuda, pose, edge, meas, weight, fixed=fixed, node_off=torch.tensor(node_off, dtype=torch.int32, device=cuda),
                   edge_off=torch.tensor(edge_off, dtype=torch.int32, device=cuda), **SOLVER)
    _equal(dev_off, got, "device offsets")


def test_skipped_edges(cuda):
    start, edge, meas, weight = _chain(15, 24, loops=12)
    edge, meas, weight = edge.copy(), meas.copy(), weight.copy()
    n = len(edge)
    edge[n - 1] = (3, 24)           # out of range
    edge[n - 2] = (-1, 2)
    edge[n - 3] = (7, 7)            # i == j
    meas[n - 4, 5] = np.nan
    meas[n - 5, 11] = np.inf
    weight[n - 6, 0] = np.nan
    weight[n - 7, 1] = -1.0
    weight[n - 8, 1] = np.inf
    got = _both(cuda, start, edge, meas, weight, "skipped", **SOLVER)
    assert got[3][0, 4:6].tolist() == [n - 8, 8] and (got[2][n - 8:] == -1.0).all() and (got[2][:n - 8] >= 0).all()
    # the same as the graph without them
    clean = _gpu(cuda, start, edge[:n - 8], meas[:n - 8], weight[:n - 8], **SOLVER)
    assert clean[0].tobytes() == got[0].tobytes() and clean[1].tobytes() == got[1].tobytes()


def test_refused_solve_leaves_the_pose_bits(cuda):
    start, edge, meas, weight = _chain(16, 12)
    weight = weight.copy()
    weight[10:] = 0.0               # node 11's only edge weighs nothing: a zero diagonal block
    got = _both(cuda, start, edge, meas, weight, "zero block", **SOLVER)
    assert got[3][0, 0] == R.REFUSED and got[0].tobytes() == start.tobytes() and (got[1][0] == got[1][0, 0]).all()
    # a start that is not finite
    bad = start.copy()
    bad[4, 3] = np.nan
    got = _both(cuda, bad, edge, meas, _chain(16, 12)[3], "nan start", **SOLVER)
    assert got[3][0, 0] == R.REFUSED and got[0].tobytes() == bad.tobytes()
    # refused TRIALS: from the minimum with a large first damping no trial lowers the cost by rounding luck alone; whatever is
    # refused leaves the bits, and the cost never rises
    full = _chain(16, 12)
    best = R.solve(*full, outer=30, cg_iters=60)
    got = _both(cuda, best[0], *full[1:], "at the minimum", outer=6, cg_iters=12, lambda0=1e6)
    assert (np.diff(got[1][0]) <= 0).all()
    if got[3][0, 1] == 0:
        assert got[0].tobytes() == best[0].tobytes()


@pytest.mark.parametrize("huber", [0.0, 2.0])
def test_huber_on_and_off(cuda, huber):
    g = R.two_laps(7, 48, outliers=0.3)
    got = _both(cuda, g["start"], g["edge"], g["meas"], g["weight"], f"huber={huber}", huber=huber, outer=6, cg_iters=30)
    assert got[3][0, 1] >= 1


def test_repeatable_and_two_streams(cuda):
    start, edge, meas, weight = _chain(17, 300, loops=40)
    one = _gpu(cuda, start, edge, meas, weight, **SOLVER)
    two = _gpu(cuda, start, edge, meas, weight, **SOLVER)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(cuda)
    args = (up(start, np.float64), up(edge, np.int32), up(meas, np.float64), up(weight, np.float64))
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream(), torch.cuda.Stream()], []
    for s in streams:
        with torch.cuda.stream(s):
            outs.append(ops.pgo_solve(*args, **SOLVER))      # its own workspace and outputs
    torch.cuda.synchronize()
    for out in outs:
        assert all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(one, out))


def test_argument_errors(cuda):
    start, edge, meas, weight = _chain(18, 6)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(cuda)
    p, e, m, w = up(start, np.float64), up(edge, np.int32), up(meas, np.float64), up(weight, np.float64)
    with pytest.raises(ValueError):
        ops.pgo_solve(p, e, m[:, :11], w)
    with pytest.raises(ValueError):
        ops.pgo_solve(p, e, m, w, fixed=torch.zeros(5, dtype=torch.uint8, device=cuda))
    with pytest.raises(LpdHipError):      # one tensor left on the host
        ops.pgo_solve(p, e, m, w.cpu())
    with pytest.raises(LpdHipError):
        ops.pgo_solve(p.cpu(), e.cpu(), m.cpu(), w.cpu())
    lib, ptr = ops._lib.load(), ops._ptr
    off = torch.tensor([0, 6], dtype=torch.int32, device=cuda)
    eoff = torch.tensor([0, 5], dtype=torch.int32, device=cuda)
    cp, ci = ops.pgo_csr(e, off, eoff, 6)
    assert cp.cpu().tolist() == [0, 1, 3, 5, 7, 9, 10] and ci.cpu().tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    cost, chi, info = torch.zeros((1, 3), dtype=torch.float64, device=cuda), torch.zeros(5, dtype=torch.float64, device=cuda), torch.zeros((1, 8), dtype=torch.int32, device=cuda)
    fx = torch.zeros(6, dtype=torch.uint8, device=cuda)
    ws = torch.empty(int(lib.lpd_pgo_workspace_bytes(6, 5, 1)), dtype=torch.uint8, device=cuda)
    assert lib.lpd_pgo_workspace_bytes(-1, 5, 1) == 0 and lib.lpd_pgo_workspace_bytes(6, 5, 0) == 0 and lib.lpd_pgo_workspace_bytes(6, 5, 65536) == 0

    def call(**kw):
        a = dict(pose=ptr(p), fixed=ptr(fx), node_off=ptr(off), V=6, edge=ptr(e), meas=ptr(m), weight=ptr(w), edge_off=ptr(eoff), E=5, G=1, cp=ptr(cp),
                 ci=ptr(ci), outer=2, cg=5, tol=1e-6, lam=1e-4, huber=0.0, cost=ptr(cost), chi=ptr(chi), info=ptr(info), ws=ptr(ws))
        a.update(kw)
        return lib.lpd_pgo_solve(*a.values(), None)
    pose_before = p.clone()
    for kw in (dict(pose=None), dict(ws=None), dict(G=0), dict(G=65536), dict(V=-1), dict(outer=65), dict(cg=0), dict(cg=1025), dict(tol=1.0),
               dict(lam=-1.0), dict(lam=float("nan")), dict(huber=float("inf")), dict(cost=None), dict(cp=None), dict(chi=None)):
        assert call(**kw) != 0, kw
        assert b"lpd_pgo_solve" in lib.lpd_last_error(), kw
    torch.cuda.synchronize()
    assert torch.equal(p, pose_before)
    assert call() == 0
    torch.cuda.synchronize()
    want = R.solve(start, edge, meas, weight, outer=2, cg_iters=5)
    _equal((p.cpu().numpy(), cost.cpu().numpy(), chi.cpu().numpy(), info.cpu().numpy()), want, "C entry")


# ---- quality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,V", RATIO_CASES)
def test_quality_gates_on_the_device(cuda, seed, V):
    c = R.quality_case(seed, V)
    g = c["graph"]
    got = _gpu(cuda, g["start"], g["edge"], g["meas"], g["weight"], **R.QUALITY_SOLVER)
    _equal(got, c["ref"], f"quality {seed}")
    ours, theirs = got[1][0, -1], c["scipy"][1]
    before, after, sci = R.ate(g["start"], g["gt"]), R.ate(got[0], g["gt"]), R.ate(c["scipy"][0], g["gt"])
    print(f"MEASURE pgo device seed={seed} V={V}: cost ratio - 1 = {ours / theirs - 1.0:.3e}; ATE start {before:.4f} device {after:.6f} scipy {sci:.6f}")
    assert got[3][0, 0] == R.CONVERGED and ours / theirs <= RATIO_GATE
    if (seed, V) in QUALITY_CASES:
        assert after < before and after <= ATE_GATE * sci


def test_outliers_on_the_device(cuda):
    o = OUTLIER_CASE
    c = R.quality_case(o["seed"], o["V"], o["outliers"], o["huber"])
    g = c["graph"]
    got = _gpu(cuda, g["start"], g["edge"], g["meas"], g["weight"], huber=o["huber"], **R.QUALITY_SOLVER)
    _equal(got, c["ref"], "outliers")
    out = g["is_outlier"]
    assert got[2][out].min() > got[2][~out].max()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_close_loops_end_to_end(cuda):
    """Two laps of a circle of 80 m through a street scene, a scan every 2 m, input poses that drift; windows of 20 m every 10 m; each
    window of the second lap paired with the window one lap earlier, aligned and refined on the device; close_loops must be the
    restatement's solve of the very graph it built, bit for bit, and must bring the windows' positions nearer the truth."""
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
    sub, positions = drive.submaps_from_drive(torch.from_numpy(pts), [n] * S, drifted, 20.0, 10.0, num_points=2048, device=cuda)
    W = len(sub.plan)
    lap = 8                                          # windows a lap: 80 m / 10 m
    assert W >= lap + 3
    pairs = torch.tensor([[w, w - lap] for w in range(lap, W)], dtype=torch.int32, device=cuda)
    al = verify.align_pairs(sub, sub, pairs)
    rf = verify.refine_pairs(sub, sub, pairs, init=al)
    res = posegraph.close_loops(sub, drifted, rf, pairs, outer=12, cg_iters=60)
    torch.cuda.synchronize()
    ref = sub.plan.ref.cpu().numpy()
    nodes = drifted[ref]
    od = posegraph.odometry_edges(torch.from_numpy(nodes).to(cuda))
    lp = posegraph.loop_edges(rf, pairs)
    edge, meas, weight = (torch.cat((a, b)).cpu().numpy() for a, b in zip(od, lp))
    assert (lp[0].cpu().numpy() == pairs.cpu().numpy()[:, ::-1]).all() and rf.valid.all()
    want = R.solve(nodes, edge, meas, weight, outer=12, cg_iters=60)
    _equal((res.poses.reshape(-1, 12).cpu().numpy(), res.cost[None].cpu().numpy(), res.chi2.cpu().numpy(), res.info[None].cpu().numpy()), want, "close_loops")
    assert torch.equal(res.positions, res.poses[:, :2, 3]) and tuple(res.positions.shape) == (W, 2) and res.positions.dtype == torch.float64
    before, after = R.ate(nodes, true[ref]), R.ate(res.poses.reshape(-1, 12).cpu().numpy(), true[ref])
    loop_err = max(np.abs(R.residual(true[ref][e[0]][None], true[ref][e[1]][None], z[None])[0, 3:]).max() for e, z in zip(lp[0].cpu().numpy(), lp[1].cpu().numpy()))
    print(f"MEASURE pgo close_loops: W={W} loops={len(pairs)} ATE before {before:.3f} m after {after:.3f} m; worst loop translation error {loop_err:.3f} m; "
          f"info {res.info.cpu().tolist()}")
    assert after < before
    # a world-frame drive is refused before any solve
    subw, _ = drive.submaps_from_drive(torch.from_numpy(pts), [n] * S, drifted, 20.0, 10.0, num_points=256, frame="world", device=cuda)
    with pytest.raises(ValueError, match="reference"):
        posegraph.close_loops(subw, drifted, rf, pairs)
