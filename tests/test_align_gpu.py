"""lpd_align_pairs and lpdnet_hip/verify.py on the GPU against the numpy restatement (tests/align_ref.py): `best` and `yaw_scores`
are integers and must be EQUAL.  The kernel has two paths, chosen by G = min(ceil(H / 4), max(1, 512 // P)) slices of a pair's
hypotheses: G = 1 (P >= 257, or H <= 4) -- one workgroup a pair writes `best` itself; G > 1 (a small P) -- the slices' keys go through
the workspace and a second launch.  lpd_align_workspace_bytes(P, H) is 0 exactly on the first path, which is how the tests name it."""
import ctypes
import math

import numpy as np
import pytest
import torch

import align_ref as R
from lpdnet_hip import LpdHipError, _lib, ops, submap, verify

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, FILL = 16, -77


def _tables(N, TA=3, TB=3, seed=0):
    """TA + TB submaps of one scene around one place, N points each: every (a, b) pair overlaps"""
    g = np.random.default_rng(50 + seed)
    sc = R.scene(seed)
    centre = g.uniform(-20, 20, 2)
    clouds = [R.submap(sc, centre + g.uniform(-2.5, 2.5, 2), g.uniform(0, 2 * np.pi), 100 * seed + i, n=N) for i in range(TA + TB)]
    return np.stack(clouds[:TA]), np.stack(clouds[TA:])


def _ref(A, B, pairs, rot, H, inv_cell, S, z0, inv_zcell, layers, **kw):
    """R.align_pairs; a pair that occurs more than once is computed once when nothing is per pair"""
    if kw.get("first") is not None or kw.get("t0") is not None:
        return R.align_pairs(A, B, pairs, rot, H, f32(inv_cell), S, z0, f32(inv_zcell), layers, **kw)
    uniq, inv = np.unique(np.asarray(pairs), axis=0, return_inverse=True)
    best, ys = R.align_pairs(A, B, uniq, rot, H, f32(inv_cell), S, z0, f32(inv_zcell), layers, **kw)
    inv = inv.reshape(-1)
    return best[inv], ys[inv]


def _gpu(dev, A, B, pairs, rot, H, inv_cell, S, z0, inv_zcell, layers, scaleA=None, scaleB=None, first=None, t0=None, same=False):
    def up(v, dt):
        return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)
    a = up(A, f32)
    b = a if same else up(B, f32)
    best, ys = ops.align_pairs(a, b, up(pairs, np.int32), up(rot, f32), H, inv_cell, S, z0, inv_zcell, layers, scale_a=up(scaleA, f32),
                               scale_b=up(scaleB, f32), first=up(first, np.int32), t0=up(t0, f32))
    torch.cuda.synchronize()
    return best.cpu().numpy(), ys.cpu().numpy()


def _pairs(g, P, TA, TB):
    return np.stack((g.integers(0, TA, P), g.integers(0, TB, P)), axis=1).astype(np.int32)


# (N, H, S, layers, P): a covering set of N = 1, 63, 64, 65, 1000, 4096, 16384; H = 1, 7, 64, 120; S = 0, 1, 8, 16; layers = 1, 4;
# P = 1, 3, 600.  split = the small-P path (slices, workspace, second launch); the others run one workgroup a pair.
SHAPES = [(1, 1, 0, 1, 1, False), (63, 7, 1, 4, 3, True), (64, 64, 8, 1, 1, True), (65, 120, 16, 4, 3, True), (1000, 7, 8, 4, 600, False),
          (1000, 1, 16, 1, 600, False), (64, 64, 0, 4, 3, True), (1000, 1, 1, 4, 3, False), (4096, 120, 8, 4, 3, True), (16384, 64, 1, 4, 1, True),
          (4097, 7, 1, 4, 3, True), (4097, 2, 8, 1, 300, False),      # N <= 4096: A's points are kept in LDS; 4097 is the first size read from memory
          (63, 7, 2, 4, 3, True), (1000, 7, 5, 4, 3, True), (1000, 5, 9, 1, 3, True)]      # the scoring loop is built for 1, 3, 9, 17, 33 dy rows: S = 2, 5, 9 are the first of a size


@pytest.mark.parametrize("N,H,S,layers,P,split", SHAPES)
def test_best_and_yaw_scores_equal_the_restatement(cuda, N, H, S, layers, P, split):
    g = np.random.default_rng(N + H + S)
    A, B = _tables(N, seed=N % 7)
    pairs = _pairs(g, P, len(A), len(B))
    rot = R.rot_table(H)
    assert (int(_lib.load().lpd_align_workspace_bytes(P, H)) > 0) == split
    want_best, want_ys = _ref(A, B, pairs, rot, H, 2.0, S, 0.0, 0.5, layers)
    best, ys = _gpu(cuda, A, B, pairs, rot, H, 2.0, S, 0.0, 0.5, layers)
    print(f"MEASURE align/equal N={N} H={H} S={S} layers={layers} P={P} split={split} scores {want_best[:3, 3].tolist()} of cells "
          f"{want_best[:3, 4].tolist()} / {want_best[:3, 5].tolist()}")
    assert np.array_equal(best, want_best) and np.array_equal(ys, want_ys)
    assert (best[:, 6] == 1).all() and (N < 63 or want_best[:, 3].max() > 0)      # the clouds do overlap: the scores are not all zero


@pytest.fixture(scope="module")
def small():
    A, B = _tables(1000, seed=3)
    return A, B, R.rot_table(16)


def test_first_wraps_around_the_table(cuda, small):
    A, B, rot = small
    pairs = np.array([[0, 0], [1, 2], [2, 1], [0, 1]], dtype=np.int32)
    first = np.array([12, 15, -3, 2147483647], dtype=np.int32)      # (first + h) mod 16 passes the table's end for h = 0 .. 6
    want = _ref(A, B, pairs, rot, 7, 2.0, 4, 0.0, 0.5, 4, first=first)
    got = _gpu(cuda, A, B, pairs, rot, 7, 2.0, 4, 0.0, 0.5, 4, first=first)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    plain = _ref(A, B, pairs, rot, 7, 2.0, 4, 0.0, 0.5, 4)
    assert not np.array_equal(plain[1], want[1])      # the table's other entries give other scores


def test_pre_translation(cuda, small):
    A, B, rot = small
    pairs = np.array([[0, 0], [1, 2], [2, 1]], dtype=np.int32)
    t0 = np.array([[1.5, -2.0], [0.3, 0.7], [-3.25, 0.125]], dtype=np.float32)
    want = _ref(A, B, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4, t0=t0)
    got = _gpu(cuda, A, B, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4, t0=t0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[1], _ref(A, B, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4)[1])


def test_one_table_for_both_clouds(cuda, small):
    A, _, rot = small
    pairs = np.array([[0, 0], [1, 2], [2, 1]], dtype=np.int32)
    want = _ref(A, A, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4)
    got = _gpu(cuda, A, None, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4, same=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][0].tolist()[:4] == [0, 0, 0, int(want[0][0, 4])] and want[0][0, 4] == want[0][0, 5]      # a cloud against itself


def _strided(t, fill):
    """the values of t as the leading columns of a tensor one column wider: not contiguous"""
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 1,), fill, dtype=t.dtype, device=t.device)
    wide[..., :-1] = t
    v = wide[..., :-1]
    assert not v.is_contiguous()
    return v


def test_non_contiguous_arguments_equal_the_contiguous_ones(cuda, small):
    """two distinct tables of one size, pairs and the rotation table as strided views: the wrapper's contiguous copies all live
    until the launch, so none of them takes another's memory"""
    A, B, rot = small
    a, b = torch.from_numpy(A).to(cuda), torch.from_numpy(B).to(cuda)
    pairs = torch.tensor([[0, 0], [1, 2], [2, 1], [0, 1]], dtype=torch.int32, device=cuda)
    r = torch.from_numpy(rot).to(cuda)
    want = ops.align_pairs(a, b, pairs, r, 16, 2.0, 4, 0.0, 0.5, 4)
    got = ops.align_pairs(_strided(a, float("nan")), _strided(b, float("nan")), _strided(pairs, -1), _strided(r, float("nan")), 16, 2.0, 4, 0.0, 0.5, 4)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want[0], ops.align_pairs(b, b, pairs, r, 16, 2.0, 4, 0.0, 0.5, 4)[0])      # b in a's place gives another answer


def test_scale_tables(cuda, small):
    A, B, rot = small
    sa, sb = np.array([25.0, 31.5, 0.9], dtype=np.float32), np.array([27.25, 1.0, 40.0], dtype=np.float32)
    An, Bn = (A / sa[:, None, None]).astype(np.float32), (B / sb[:, None, None]).astype(np.float32)
    pairs = np.array([[0, 0], [1, 2], [2, 1], [1, 1]], dtype=np.int32)
    want = _ref(An, Bn, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4, scaleA=sa, scaleB=sb)
    got = _gpu(cuda, An, Bn, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4, scaleA=sa, scaleB=sb)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0][:, 3].min() > 20


def test_points_on_cell_boundaries(cuda):
    """every point sits on a corner of four cells (and of two layers), and the table's entries are exact quarter turns: the products
    and sums are exact, so the point belongs to the cell the floor says -- on both sides of the comparison"""
    g = np.random.default_rng(8)
    k = g.integers(-66, 67, (2, 3, 1500, 2))      # beyond the grid's first and last cell too: fx = -1, 0, 127, 128
    z = g.integers(-1, 6, (2, 3, 1500, 1)) * 2.0
    T = np.concatenate((k * 0.5, z), axis=3).astype(np.float32)
    rot = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=np.float32)
    pairs = np.array([[0, 0], [1, 2], [2, 1]], dtype=np.int32)
    t0 = np.array([[0.5, -1.0], [0.0, 0.0], [-2.5, 32.0]], dtype=np.float32)
    want = _ref(T[0], T[1], pairs, rot, 4, 2.0, 2, 0.0, 0.5, 4, t0=t0)
    got = _gpu(cuda, T[0], T[1], pairs, rot, 4, 2.0, 2, 0.0, 0.5, 4, t0=t0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0][:, 3].min() > 0


def test_nan_and_inf_rows_set_no_bit(cuda, small):
    A, B, rot = (v.copy() for v in small)
    g = np.random.default_rng(9)
    for T in (A, B):
        for t in range(len(T)):
            rows = g.choice(T.shape[1], 300, replace=False)
            T[t, rows[:100], g.integers(0, 3, 100)] = np.nan
            T[t, rows[100:200], g.integers(0, 3, 100)] = np.inf
            T[t, rows[200:], g.integers(0, 3, 100)] = g.choice([-np.inf, 1e30, -3e38], 100)
    A[2] = np.nan      # a whole cloud: empty
    pairs = np.array([[0, 0], [1, 2], [2, 1], [1, 1]], dtype=np.int32)
    want = _ref(A, B, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4)
    got = _gpu(cuda, A, B, pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0][2].tolist() == [0, -4, -4, 0, 0, int(want[0][2, 5]), 1, 0] and want[0][2, 5] > 0


def _raw(dev, A, B, pairs, rot, H, S, best, ys, layers=4, N=None, TA=None, TB=None):
    """the C entry point itself, on the caller's output buffers"""
    lib = _lib.load()
    P = pairs.shape[0]
    ws = torch.empty(max(int(lib.lpd_align_workspace_bytes(P, H)), 16), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = lib.lpd_align_pairs(p(A), A.shape[0] if TA is None else TA, None, p(B), B.shape[0] if TB is None else TB, None, A.shape[1] if N is None else N,
                             p(pairs), P, p(rot), rot.shape[0], None, H, None, 2.0, S, 0.0, 0.5, layers, p(best), p(ys), p(ws),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("P,H", [(5, 16), (300, 3)])
def test_out_of_range_pairs_are_not_read_and_the_guards_stay(cuda, small, P, H):
    """both paths; rows outside the tables (negative, the table's length, far beyond) give (-1, 0, ...) and zero yaw_scores; `best`
    and `yaw_scores` lie between guard rows that keep their fill"""
    A, B, rot = small
    g = np.random.default_rng(P)
    pairs = _pairs(g, P, len(A), len(B))
    pairs[1], pairs[3], pairs[P - 1] = (-1, 0), (0, len(B)), (2147483647, -2147483648)
    pairs[2] = (len(A), 1)
    want = _ref(A, B, pairs, rot, H, 2.0, 2, 0.0, 0.5, 4)
    a, b, r = (torch.from_numpy(v).to(cuda) for v in (A, B, rot))
    best = torch.full((P + 2 * GUARD, 8), FILL, dtype=torch.int32, device=cuda)
    ys = torch.full((P + 2 * GUARD, H), FILL, dtype=torch.int32, device=cuda)
    assert _raw(cuda, a, b, torch.from_numpy(pairs).to(cuda), r, H, 2, best[GUARD:], ys[GUARD:]) == 0
    best, ys = best.cpu().numpy(), ys.cpu().numpy()
    assert (best[:GUARD] == FILL).all() and (best[GUARD + P:] == FILL).all() and (ys[:GUARD] == FILL).all() and (ys[GUARD + P:] == FILL).all()
    assert np.array_equal(best[GUARD:GUARD + P], want[0]) and np.array_equal(ys[GUARD:GUARD + P], want[1])
    for i in (1, 2, 3, P - 1):
        assert best[GUARD + i].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and not ys[GUARD + i].any()


@pytest.mark.parametrize("P,H", [(3, 16), (300, 3)])
def test_yaw_scores_may_be_null(cuda, small, P, H):
    A, B, rot = small
    pairs = _pairs(np.random.default_rng(P + 1), P, len(A), len(B))
    want = _ref(A, B, pairs, rot, H, 2.0, 2, 0.0, 0.5, 4)
    a, b, r = (torch.from_numpy(v).to(cuda) for v in (A, B, rot))
    best = torch.full((P + GUARD, 8), FILL, dtype=torch.int32, device=cuda)
    assert _raw(cuda, a, b, torch.from_numpy(pairs).to(cuda), r, H, 2, best, None) == 0
    best = best.cpu().numpy()
    assert np.array_equal(best[:P], want[0]) and (best[P:] == FILL).all()


def test_two_launches_and_two_streams_give_the_same_bits(cuda):
    """Two launches on the current stream and one on each of two streams of its own, on both paths: the same bits (the body is
    tests/align_streams_child.py).  The streams are made in a process of their own: torch's stream pool stays for the life of a
    process, and a suite that runs everything in one process should not have this test decide how many queues every later test
    runs beside (one existing case, two workgroups of lpd_clean_fill writing the same mask bytes, comes out the other
    way round once a process has launched on side streams)."""
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_streams_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "P=25 H=120" in r.stdout and "P=600 H=8" in r.stdout


# ---- the wrapper ----
@pytest.fixture(scope="module")
def scene_pairs():
    """8 pairs of the labelled scenes (6 true, 2 false) as two tables, and the restatement's chain on them"""
    a, b, truth = [], [], []
    for seed in range(6):
        x, y, yaw, t = R.true_pair(seed)
        a.append(x), b.append(y), truth.append((yaw, t))
    for seed in range(2):
        x, y = R.false_pair(seed)
        a.append(x), b.append(y)
    A, B = np.stack(a), np.stack(b)
    pairs = np.stack((np.arange(8), np.arange(8)), axis=1).astype(np.int32)
    return A, B, pairs, truth, R.chain(A, B, pairs)


def test_align_pairs_equals_the_chain_of_the_restatement(cuda, scene_pairs):
    A, B, pairs, truth, want = scene_pairs
    al = verify.align_pairs(torch.from_numpy(A).to(cuda), torch.from_numpy(B).to(cuda)[:, None], torch.from_numpy(pairs).to(cuda).long())
    assert np.array_equal(al.coarse.cpu().numpy(), want["coarse"]) and np.array_equal(al.fine.cpu().numpy(), want["fine"])
    assert np.array_equal(al.yaw_scores.cpu().numpy(), want["yaw_scores"])
    assert al.yaw.dtype == torch.float64 and al.translation.dtype == torch.float64 and al.overlap.dtype == torch.float64
    assert np.array_equal(al.yaw.cpu().numpy(), want["yaw"]) and np.array_equal(al.translation.cpu().numpy(), want["translation"])
    assert np.array_equal(al.score.cpu().numpy(), want["score"]) and np.array_equal(al.cells_a.cpu().numpy(), want["cells_a"])
    assert np.array_equal(al.cells_b.cpu().numpy(), want["cells_b"]) and np.allclose(al.overlap.cpu().numpy(), want["overlap"], rtol=1e-15, atol=0)
    assert al.valid.all()
    for i, (yaw, t) in enumerate(truth):      # and the chain finds the pairs' transforms (the conditions of tests/test_align_cpu.py)
        assert R.yaw_error(float(al.yaw[i]), yaw) <= 2 * (2 * math.pi / 960) + 1e-9 and np.abs(al.translation[i].cpu().numpy() - t).max() <= 0.25
    coarse_only = verify.align_pairs(torch.from_numpy(A).to(cuda), torch.from_numpy(B).to(cuda), torch.from_numpy(pairs).to(cuda),
                                     verify.AlignSearch(fine=False))
    assert coarse_only.fine is None and np.array_equal(coarse_only.coarse.cpu().numpy(), want["coarse"])
    assert np.array_equal(coarse_only.translation.cpu().numpy(), want["coarse"][:, [2, 1]] * 0.5)


def _moved(a, yaw, t):
    c, s = math.cos(yaw), math.sin(yaw)
    a = a.astype(np.float64)
    return np.column_stack((c * a[:, 0] - s * a[:, 1] + t[0], s * a[:, 0] + c * a[:, 1] + t[1], a[:, 2]))


def test_matrix_maps_a_onto_b(cuda):
    """B is A moved by a known transform: matrix() takes every point of A to its partner in B within one fine cell (0.25 m) per axis"""
    a = R.true_pair(2)[0]
    yaw, t = 2 * math.pi * 123 / 960, (1.75, -2.25)
    b = _moved(a, yaw, t).astype(np.float32)
    al = verify.align_pairs(torch.from_numpy(a[None]).to(cuda), torch.from_numpy(b[None]).to(cuda), torch.tensor([[0, 0]], device=cuda))
    M = al.matrix()[0].cpu().numpy()
    got = (M @ np.column_stack((a.astype(np.float64), np.ones(len(a)))).T).T[:, :3]
    err = np.abs(got - b.astype(np.float64)).max(axis=0)
    print(f"MEASURE align/matrix yaw error {math.degrees(R.yaw_error(float(al.yaw[0]), yaw)):.3f} deg, largest point error {err.tolist()} m")
    assert M.shape == (4, 4) and err[0] <= 0.25 and err[1] <= 0.25 and err[2] == 0.0 and float(al.overlap[0]) > 0.5


def test_verify_candidates_puts_the_true_candidate_first(cuda):
    """query 0's true place sits at rank 3 of its retrieval, query 1's at rank 0; a -1 entry is skipped and comes last"""
    qa, db0, _, _ = R.true_pair(0)
    qb, db1, _, _ = R.true_pair(1)
    others = [R.false_pair(s)[0] for s in (3, 4, 5)]      # other scenes than the two queries'
    query = torch.from_numpy(np.stack((qa, qb))).to(cuda)
    database = torch.from_numpy(np.stack([db0, db1] + others)).to(cuda)
    topk = torch.tensor([[2, 3, -1, 0], [1, 4, 2, 3]], dtype=torch.int32, device=cuda)
    v = verify.verify_candidates(query, database, topk, min_overlap=0.4)
    assert v.order.shape == (2, 4) and v.score.shape == (2, 4) and v.translation.shape == (2, 4, 2) and v.matrix().shape == (2, 4, 4, 4)
    assert v.yaw_scores.shape == (2, 4, 120)
    order, score, valid = v.order.cpu().numpy(), v.score.cpu().numpy(), v.valid.cpu().numpy()
    assert order[0, 0] == 3 and order[0, 3] == 2 and order[1, 0] == 0
    assert valid.tolist() == [[True, True, False, True], [True] * 4]
    for q in range(2):
        key = np.where(valid[q], score[q], -1)
        assert order[q].tolist() == sorted(range(4), key=lambda r: (-key[r], r))      # descending score, ties in retrieval order
    acc = v.accepted.cpu().numpy()
    assert acc[0, 3] and acc[1, 0] and not acc[0, 2] and np.array_equal(acc, valid & (v.overlap.cpu().numpy() >= 0.4))
    want = R.chain(query.cpu().numpy(), database.cpu().numpy(), [[0, 0], [1, 1]])
    assert np.array_equal(v.fine[0, 3].cpu().numpy(), want["fine"][0]) and np.array_equal(v.fine[1, 0].cpu().numpy(), want["fine"][1])
    assert verify.verify_candidates(query, database, topk.long()).accepted is None


def test_submaps_are_accepted_and_their_centres_honoured(cuda):
    a = R.true_pair(4)[0]
    yaw, t = 2 * math.pi * 700 / 960, (-1.25, 2.5)
    # the two scans' own frames are far apart; their centres (as make_submaps would find them) bring the centred clouds within
    # t' = (0.75, -1.0) of each other: p_B - c_B = R (p_A - c_A) + t' with c_B = t + R c_A - t' in plan view, and the heights differ
    # by the centres' difference alone
    ca = np.array([10.0, -5.0, 1.0])
    t_c = np.array([0.75, -1.0])
    cb = np.append(_moved(ca[None], yaw, t)[0, :2] - t_c, 2.5)
    b = _moved(a, yaw, t)
    b[:, 2] += cb[2] - ca[2]
    b = b.astype(np.float32)
    sa, sb = f32(26.0), f32(31.0)
    # the scans in their own frames: row = x * scale + centre
    xa, xb = ((a - ca.astype(f32)) / sa).astype(f32), ((b - cb.astype(f32)) / sb).astype(f32)

    def sub(x, c, s):
        xform = torch.tensor([[c[0], c[1], c[2], s]], dtype=torch.float32, device=cuda)
        return submap.Submaps(torch.from_numpy(x[None, None]).to(cuda), torch.zeros(1, 4, dtype=torch.int32, device=cuda), xform, None)
    search = verify.AlignSearch(z_lo=-3.0)
    al = verify.align_pairs(sub(xa, ca, sa), sub(xb, cb, sb), torch.tensor([[0, 0]], device=cuda), search)
    want = R.chain(xa[None], xb[None], [[0, 0]], dict(z_lo=-3.0), scaleA=np.array([sa]), scaleB=np.array([sb]))
    assert np.array_equal(al.coarse.cpu().numpy(), want["coarse"]) and np.array_equal(al.fine.cpu().numpy(), want["fine"])
    assert np.abs(al.translation[0].cpu().numpy() - t_c).max() <= 0.25      # the centred clouds' own offset
    M = al.matrix()[0].cpu().numpy()      # ... and with the centres: the scans' own rows of A onto B's
    rows_a = xa.astype(np.float64) * float(sa) + ca
    rows_b = xb.astype(np.float64) * float(sb) + cb
    got = (M @ np.column_stack((rows_a, np.ones(len(a)))).T).T[:, :3]
    err = np.abs(got - rows_b).max(axis=0)
    print(f"MEASURE align/submaps largest point error {err.tolist()} m")
    assert err[0] <= 0.25 and err[1] <= 0.25 and abs(M[2, 3] - (cb[2] - ca[2])) < 1e-12 and err[2] < 1e-4
    with pytest.raises(ValueError):
        verify.align_pairs(sub(xa, ca, sa), sub(xb, cb, sb), torch.tensor([[0, 0]], device=cuda), search, scale_a=torch.ones(1, device=cuda))


def test_argument_errors(cuda, small):
    A, B, rot = (torch.from_numpy(v).to(cuda) for v in small)
    pairs = torch.zeros(2, 2, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        ops.align_pairs(A, B, pairs, rot, 17, 2.0, 4, 0.0, 0.5, 4)
    with pytest.raises(ValueError):
        ops.align_pairs(A, B[:, :999], pairs, rot, 16, 2.0, 4, 0.0, 0.5, 4)
    with pytest.raises(LpdHipError):
        ops.align_pairs(A, B, pairs.cpu(), rot, 16, 2.0, 4, 0.0, 0.5, 4)
    with pytest.raises(TypeError):
        ops.align_pairs(A, B, pairs.long(), rot, 16, 2.0, 4, 0.0, 0.5, 4)
    with pytest.raises(LpdHipError):
        ops.align_pairs(A.cpu(), B.cpu(), pairs.cpu(), rot.cpu(), 16, 2.0, 4, 0.0, 0.5, 4)
    # the library's own checks, behind the wrapper's: the usual code, the text through lpd_last_error, nothing written
    best = torch.full((2, 8), FILL, dtype=torch.int32, device=cuda)
    lib = _lib.load()
    for kw, word in ((dict(S=17), "S=17"), (dict(layers=5), "layers=5"), (dict(H=17), "H=17"), (dict(N=16385), "N=16385"), (dict(TA=0), "TA=0")):
        args = dict(H=16, S=4, layers=4)
        args.update(kw)
        assert _raw(cuda, A, B, pairs, rot, args.pop("H"), args.pop("S"), best, None, **args) == _lib.DEFINES["LPD_ERR_ARG"]
        assert word in lib.lpd_last_error().decode()
    assert _raw(cuda, A, B, pairs, rot, 16, 4, None, None) == _lib.DEFINES["LPD_ERR_ARG"] and "null" in lib.lpd_last_error().decode()
    assert (best.cpu().numpy() == FILL).all()
    assert lib.lpd_align_workspace_bytes(0, 16) == 0 and lib.lpd_align_workspace_bytes(1, 1025) == 0
    assert lib.lpd_align_workspace_bytes(1, 120) == 30 * 16 and lib.lpd_align_workspace_bytes(25, 120) == 25 * 20 * 16
    assert lib.lpd_align_workspace_bytes(257, 120) == 0 and lib.lpd_align_workspace_bytes(256, 120) == 256 * 2 * 16
