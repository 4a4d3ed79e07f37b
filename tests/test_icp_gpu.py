"""lpd_point_normals, lpd_icp_pairs and lpdnet_hip/verify.py's refinement on the GPU against the numpy restatement (tests/icp_ref.py):
`nn`, `sums`, `info` are integers and must be EQUAL, and `pose` (float64, every operation rounded once) equal bit for bit.  The pass
kernel gives a workgroup 64 points of A (a chunk) and stages B in LDS 4096 points at a time (a tile); the step kernel takes 256
pairs a workgroup: the sizes below lie on both sides of each.  The restatement is given the device's own normals, so that what is
compared is the pass and the step, not the last bit of a square root."""
import ctypes

import numpy as np
import pytest
import torch

import align_ref as AR
import icp_ref as R
import walk_forms
from lpdnet_hip import _lib, ops, verify
from test_icp_cpu import NORMAL_GATE, NORMAL_MIN_GAP, QUALITY_GATE_DEG, QUALITY_GATE_M, _corner, _patches, _small_pose

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 64


def _up(dev, v, dt):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)


def _tables(N, TA=2, TB=3, seed=0):
    """TA + TB submaps of one scene around one place, N points each: every (a, b) pair overlaps"""
    g = np.random.default_rng(70 + seed)
    sc = AR.scene(seed)
    centre = g.uniform(-20, 20, 2)
    clouds = [AR.submap(sc, centre + g.uniform(-0.5, 0.5, 2), g.uniform(-0.05, 0.05), 100 * seed + i, n=N) for i in range(TA + TB)]
    return np.stack(clouds[:TA]), np.stack(clouds[TA:])


def _device_normals(dev, B):
    """[TB, N, 3] numpy: the device's normals of B (16 neighbours, fewer for a small cloud); random unit vectors below four points"""
    N = B.shape[1]
    if N < 4:
        v = np.random.default_rng(N).standard_normal(B.shape)
        return (v / np.linalg.norm(v, axis=2, keepdims=True)).astype(f32)
    n = verify.point_normals(_up(dev, B, f32), k=min(16, N))
    torch.cuda.synchronize()
    return n.cpu().numpy()


def _gpu(dev, A, B, nB, pairs, pose, dmax, min_inliers=6, scaleA=None, scaleB=None, same=False):
    a = _up(dev, A, f32)
    b = a if same else _up(dev, B, f32)
    out = ops.icp_pairs(a, b, _up(dev, nB, f32), _up(dev, pairs, np.int32), _up(dev, pose, np.float64), dmax, min_inliers,
                        scale_a=_up(dev, scaleA, f32), scale_b=_up(dev, scaleB, f32), want_nn=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _ref(A, B, nB, pairs, pose, dmax, min_inliers=6, scaleA=None, scaleB=None):
    """R.icp_pairs; a (pair, pose) that occurs more than once is computed once"""
    key = np.concatenate((np.asarray(pairs, dtype=np.float64), np.asarray(pose, dtype=np.float64).reshape(len(pairs), 12)), axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    po, info, sums, nn = R.icp_pairs(A, B, nB, np.asarray(pairs)[first], np.asarray(pose).reshape(-1, 12)[first], dmax, min_inliers, scaleA, scaleB)
    return po[inv], info[inv], sums[:, inv], nn[inv]


def _equal(got, want):
    pose, info, sums, nn = got
    return (pose.tobytes() == np.asarray(want[0], dtype=np.float64).tobytes() and np.array_equal(info, want[1]) and np.array_equal(sums, want[2])
            and np.array_equal(nn, want[3]))


# ---- 1. one pass -------------------------------------------------------------------------------------------------------------------
# (N, P): N = 1, 63, 64, 65 (the chunk of 64), 1000, 4095, 4096, 4097 (the tile of 4096: 4097 needs a second one), 8200 (a third);
# P = 1, 3, 25, 300 (the step kernel's 256 pairs a workgroup)
SHAPES = [(1, 1), (63, 3), (64, 25), (65, 3), (127, 300), (1000, 300), (1000, 1), (4095, 1), (4096, 3), (4097, 1), (8200, 1)]


@pytest.mark.parametrize("N,P", SHAPES)
def test_one_pass_equals_the_restatement(cuda, N, P):
    g = np.random.default_rng(N + P)
    A, B = _tables(N, seed=N % 5)
    nB = _device_normals(cuda, B)
    pairs = np.stack((g.integers(0, len(A), P), g.integers(0, len(B), P)), axis=1).astype(np.int32)
    starts = np.stack([_small_pose(g, 0.03, 0.3) for _ in range(6)])
    pose = starts[(pairs[:, 0] * 3 + pairs[:, 1]) % 6]      # one start per distinct pair: the restatement runs each once
    got = _gpu(cuda, A, B, nB, pairs, pose, [1.0])
    want = _ref(A, B, nB, pairs, pose, [1.0])
    print(f"MEASURE icp/one-pass N={N} P={P} correspondences {want[2][0, :3, 0].tolist()} of {N}")
    assert _equal(got, want)
    assert got[0].tobytes() == pose.tobytes() and (got[1][:, :3] == [1, 0, 0]).all()      # no step: the pose is the start
    assert N < 1000 or (want[2][0, :, 0] > N // 4).all()      # the clouds do overlap: the sums are not empty
    assert (got[2][:, :, 29:] == 0).all()


def test_one_table_for_both_clouds_and_scale_tables(cuda):
    g = np.random.default_rng(11)
    A, B = _tables(1000, seed=3)
    nA = _device_normals(cuda, A)
    pairs = np.array([[0, 0], [1, 0], [0, 1]], dtype=np.int32)
    pose = np.stack([_small_pose(g, 0.03, 0.3) for _ in range(3)])
    got = _gpu(cuda, A, None, nA, pairs, pose, [0.7], same=True)
    assert _equal(got, _ref(A, A, nA, pairs, pose, [0.7]))
    sa, sb = np.array([25.0, 0.9], dtype=f32), np.array([27.25, 1.0, 40.0], dtype=f32)
    An, Bn = (A / sa[:, None, None]).astype(f32), (B / sb[:, None, None]).astype(f32)
    nB = _device_normals(cuda, B)
    pairs = np.array([[0, 0], [1, 2], [0, 1], [1, 1]], dtype=np.int32)
    pose = np.stack([_small_pose(g, 0.03, 0.3) for _ in range(4)])
    got = _gpu(cuda, An, Bn, nB, pairs, pose, [1.0], scaleA=sa, scaleB=sb)
    want = _ref(An, Bn, nB, pairs, pose, [1.0], scaleA=sa, scaleB=sb)
    assert _equal(got, want) and want[2][0, :, 0].min() > 300
    assert not np.array_equal(want[2], _ref(An, Bn, nB, pairs, pose, [1.0])[2])      # the scales matter


def test_non_contiguous_arguments_equal_the_contiguous_ones(cuda):
    """a, b and normals_b of one size (TA = TB), pairs and pose as strided views: the wrapper's contiguous copies all live until the
    launch, so none of them takes another's memory"""
    from test_align_gpu import _strided
    g = np.random.default_rng(14)
    A, B = _tables(1000, TA=3, TB=3, seed=3)
    a, b, nb = _up(cuda, A, f32), _up(cuda, B, f32), _up(cuda, _device_normals(cuda, B), f32)
    pairs = torch.tensor([[0, 0], [1, 2], [2, 1], [0, 1]], dtype=torch.int32, device=cuda)
    pose = _up(cuda, np.stack([_small_pose(g, 0.03, 0.3) for _ in range(4)]), np.float64)
    nan = float("nan")
    want = ops.icp_pairs(a, b, nb, pairs, pose, [1.0, 1.0], 6, want_nn=True)
    got = ops.icp_pairs(_strided(a, nan), _strided(b, nan), _strided(nb, nan), _strided(pairs, -1), _strided(pose, nan), [1.0, 1.0], 6, want_nn=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and int(want[2][0, :, 0].min()) > 250      # the clouds do overlap
    assert not torch.equal(want[2], ops.icp_pairs(b, b, nb, pairs, pose, [1.0, 1.0], 6)[2])      # b in a's place gives other sums


# ---- 2. ties and edges -------------------------------------------------------------------------------------------------------------
def test_ties_and_edges(cuda):
    g = np.random.default_rng(12)
    eye = np.eye(3, 4).reshape(1, 12)
    # a lattice against itself moved by half a cell: every point of A has equidistant candidates, the lowest index wins; with
    # duplicated rows of B on top (the same point at two indices)
    ax = np.arange(7, dtype=f32)
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)      # 343 points
    Bl = np.concatenate((lat, lat[:100]))[g.permutation(443)][None]
    Al = np.concatenate((lat + f32(0.5), lat[:100]))[None].astype(f32)
    nl = np.tile(np.array([0.6, 0.0, 0.8], dtype=f32), (1, 443, 1))
    pr = np.array([[0, 0]], dtype=np.int32)
    got, want = _gpu(cuda, Al, Bl, nl, pr, eye, [1.0]), _ref(Al, Bl, nl, pr, eye, [1.0])
    assert _equal(got, want) and (want[3] >= 0).sum() > 400
    d = R.d2(Bl[0], Al[0])
    assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() > 300      # the ties are there
    # rows of B at exactly dmax and one ulp beyond; NaN / inf rows on either side; zero normals; transformed points beyond 512 m
    n = 200
    A = g.uniform(-20, 20, (1, n, 3)).astype(f32)
    B = (A + g.uniform(-5, 5, (1, n, 3))).astype(f32)      # far: only the rows placed below are within dmax
    dm = f32(1.5)
    B[0, :40] = A[0, :40] + np.array([dm, 0, 0], dtype=f32)
    exact = (B[0, :40, 0] - A[0, :40, 0]) == dm      # the sum rounded: keep the rows where the difference is dmax exactly
    B[0, 40:80] = A[0, 40:80]
    B[0, 40:80, 1] = np.nextafter(A[0, 40:80, 1] + dm, f32(1e9))
    B[0, 80:90] = np.nan
    B[0, 90:100, 2] = np.inf
    A[0, 100:110, 0] = np.nan
    A[0, 110:120] = -np.inf
    A[0, 120:130] = [600.0, 0.0, 0.0]
    A[0, 130:140] = [0.0, np.nextafter(f32(512.0), f32(1e9)), 0.0]
    B[0, 140:160] = A[0, 140:160] + f32(0.25)
    nb = g.standard_normal((1, n, 3))
    nb = (nb / np.linalg.norm(nb, axis=2, keepdims=True)).astype(f32)
    nb[0, 150:160] = 0.0
    nb[0, 160:165] = [0.0, -0.0, 0.0]
    got, want = _gpu(cuda, A, B, nb, pr, eye, [float(dm)]), _ref(A, B, nb, pr, eye, [float(dm)])
    assert _equal(got, want)
    nn = want[3][0]
    assert (nn[:40][exact] == np.arange(40)[exact]).sum() > 30      # d2 == dmax * dmax: a correspondence (where no other row is nearer)
    assert (nn[100:140] == -1).all() and (nn[140:150] == np.arange(140, 150)).all() and (nn[150:160] == -1).all()
    assert not np.isin(nn, np.arange(80, 100)).any()
    # a cloud of nothing but NaN on either side: no correspondence at all, empty sums
    for a_, b_ in ((np.full_like(A, np.nan), B), (A, np.full_like(B, np.nan))):
        got = _gpu(cuda, a_, b_, nb, pr, eye, [float(dm)])
        assert (got[3] == -1).all() and not got[2].any() and got[1].tolist() == [[1, 0, 0, 0]]


# ---- 3. guarding -------------------------------------------------------------------------------------------------------------------
def _guarded(dev, arr, dt, fill):
    """a device buffer with GUARD elements of `fill` on both sides of arr -> (whole tensor, pointer to the inside, element count)"""
    flat = np.ascontiguousarray(arr, dtype=dt).reshape(-1)
    whole = torch.from_numpy(np.concatenate((np.full(GUARD, fill, dtype=dt), flat, np.full(GUARD, fill, dtype=dt)))).to(dev)
    return whole, ctypes.c_void_p(whole.data_ptr() + GUARD * flat.itemsize), flat.size


def test_pairs_outside_their_tables_and_guard_rows(cuda):
    g = np.random.default_rng(13)
    N, iters = 300, 2
    A, B = _tables(N, seed=2)
    nB = _device_normals(cuda, B)
    pairs = np.array([[0, 0], [-1, 0], [0, 3], [1, 2], [2, 0], [1, -7], [2147483647, 1], [1, 1]], dtype=np.int32)
    P = len(pairs)
    pose = np.stack([_small_pose(g, 0.03, 0.3) for _ in range(P)])
    lib = _lib.load()
    ins = [_guarded(cuda, A, f32, np.nan), _guarded(cuda, B, f32, np.nan), _guarded(cuda, nB, f32, np.nan), _guarded(cuda, pairs, np.int32, 0)]
    before = [w.clone() for w, _, _ in ins]
    o_pose = _guarded(cuda, pose, np.float64, -77.0)
    o_info = _guarded(cuda, np.full((P, 4), -77), np.int32, -77)
    o_sums = _guarded(cuda, np.full(((iters + 1), P, 32), -77), np.int64, -77)
    o_nn = _guarded(cuda, np.full((P, N), -77), np.int32, -77)
    o_ws = _guarded(cuda, np.zeros(int(lib.lpd_icp_workspace_bytes(P, N, iters))), np.uint8, 0x5A)
    dm = (ctypes.c_float * (iters + 1))(1.0, 0.8, 0.6)
    rc = lib.lpd_icp_pairs(ins[0][1], len(A), None, ins[1][1], len(B), None, ins[2][1], N, ins[3][1], P, dm, iters, 6, o_pose[1], o_info[1],
                           o_sums[1], o_nn[1], o_ws[1], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    for (w, _, _), was in zip(ins, before):
        assert w.cpu().numpy().tobytes() == was.cpu().numpy().tobytes()      # the tables are as they were, guards included
    for (w, _, n), fill in ((o_pose, -77.0), (o_info, -77), (o_sums, -77), (o_nn, -77), (o_ws, 0x5A)):
        h = w.cpu().numpy()
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
    got = [o_pose[0].cpu().numpy()[GUARD:-GUARD].reshape(P, 12), o_info[0].cpu().numpy()[GUARD:-GUARD].reshape(P, 4),
           o_sums[0].cpu().numpy()[GUARD:-GUARD].reshape(iters + 1, P, 32), o_nn[0].cpu().numpy()[GUARD:-GUARD].reshape(P, N)]
    want = R.icp_pairs(A, B, nB, pairs, pose, [1.0, 0.8, 0.6], 6)
    assert _equal(got, want)
    bad = [1, 2, 4, 5, 6]
    assert (got[1][bad] == [-1, 0, 0, 0]).all() and got[0][bad].tobytes() == pose[bad].tobytes() and not got[2][:, bad].any() and (got[3][bad] == -1).all()
    assert (got[1][[0, 3, 7], 1] == iters).all()
    # the argument checks of the library itself
    null = ctypes.c_void_p(0)
    args = [ins[0][1], len(A), None, ins[1][1], len(B), None, ins[2][1], N, ins[3][1], P, dm, iters, 6, o_pose[1], o_info[1], o_sums[1], o_nn[1], o_ws[1], null]
    for pos, val in ((0, null), (6, null), (13, null), (15, null), (17, null), (7, 0), (7, 16385), (9, 0), (11, -1), (11, 65), (12, 5),
                     (10, (ctypes.c_float * 3)(1.0, 0.0, 1.0)), (10, (ctypes.c_float * 3)(1.0, 17.0, 1.0)), (10, (ctypes.c_float * 3)(float("nan"), 1.0, 1.0)),
                     (17, ctypes.c_void_p(o_ws[1].value + 4))):
        bad_args = list(args)
        bad_args[pos] = val
        assert lib.lpd_icp_pairs(*bad_args) != 0, (pos, val)
    assert lib.lpd_icp_workspace_bytes(0, N, 1) == 0 and lib.lpd_icp_workspace_bytes(1, 16385, 1) == 0 and lib.lpd_icp_workspace_bytes(1, N, 65) == 0
    torch.cuda.synchronize()


# ---- 4. the whole chain ------------------------------------------------------------------------------------------------------------
def test_whole_chain_bit_for_bit(cuda):
    g = np.random.default_rng(14)
    A, B = _tables(1024, seed=1)
    nB = _device_normals(cuda, B)
    pairs = np.array([[0, 0], [1, 2], [0, 1], [1, 0], [5, 5]], dtype=np.int32)
    pose = np.stack([_small_pose(g, 0.06, 0.5) for _ in range(5)])
    dmax = [2.0, 1.5, 1.25, 1.0, 0.9, 0.8, 0.7, 0.6, 0.5]      # iters = 8
    got, want = _gpu(cuda, A, B, nB, pairs, pose, dmax, 32), R.icp_pairs(A, B, nB, pairs, pose, dmax, 32)
    for p in range(5):
        print(f"MEASURE icp/chain pair {p} info {want[1][p].tolist()} rms {R.rms(want[2][-1, p]):.4f} m  pose bits equal {got[0][p].tobytes() == want[0][p].tobytes()}")
    assert _equal(got, want)
    assert (want[1][:4] [:, :3] == [1, 8, 0]).all() and want[1][4].tolist() == [-1, 0, 0, 0]
    assert all(got[0][p].tobytes() != pose[p].tobytes() for p in range(4)) and got[0][4].tobytes() == pose[4].tobytes()
    assert len({got[2][s, 0].tobytes() for s in range(9)}) == 9      # every pass saw another pose


def test_refused_steps_leave_the_pose(cuda):
    g = np.random.default_rng(15)
    b, nb = _corner(g, 20)
    keep = nb[:, 2] == 1
    plane, npl = b[keep][None], nb[keep][None]
    pr = np.array([[0, 0]], dtype=np.int32)
    start = _small_pose(g, 0.02, 0.05)[None]
    got = _gpu(cuda, plane, plane, npl, pr, start, [0.5] * 7)      # a single plane: singular at every step
    assert _equal(got, _ref(plane, plane, npl, pr, start, [0.5] * 7))
    assert got[0].tobytes() == start.tobytes() and got[1][0, :3].tolist() == [1, 0, 6] and got[1][0, 3] > 300
    A, B = _tables(500, seed=4)
    nB = _device_normals(cuda, B)
    start = np.stack([_small_pose(g, 0.03, 0.3)] * 2)
    pr = np.array([[0, 0], [1, 1]], dtype=np.int32)
    got = _gpu(cuda, A, B, nB, pr, start, [0.02] * 5, min_inliers=400)      # a dmax of 2 cm: too few inliers
    assert _equal(got, _ref(A, B, nB, pr, start, [0.02] * 5, 400))
    assert got[0].tobytes() == start.tobytes() and (got[1][:, 1:3] == [0, 4]).all() and (got[1][:, 3] < 400).all()


def test_repeatable_and_two_streams(cuda):
    # this module sorts behind tests/test_clean_gpu.py, whose overlapping-scans case depends on no side stream having been made before it
    # (DESIGN.md 13h): the streams are made here, in the suite's process
    g = np.random.default_rng(16)
    A, B = _tables(1000, seed=0)
    nB = _device_normals(cuda, B)
    pairs = np.stack((g.integers(0, 2, 40), g.integers(0, 3, 40)), axis=1).astype(np.int32)
    pose = np.stack([_small_pose(g, 0.04, 0.4) for _ in range(40)])
    dmax = [1.5, 1.0, 0.75, 0.5]
    one = _gpu(cuda, A, B, nB, pairs, pose, dmax)
    two = _gpu(cuda, A, B, nB, pairs, pose, dmax)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    a, b, n_, pr, po = _up(cuda, A, f32), _up(cuda, B, f32), _up(cuda, nB, f32), _up(cuda, pairs, np.int32), _up(cuda, pose, np.float64)
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream(), torch.cuda.Stream()], []
    for s in streams:
        with torch.cuda.stream(s):
            outs.append(ops.icp_pairs(a, b, n_, pr, po, dmax, 6, want_nn=True))      # its own workspace and outputs
    torch.cuda.synchronize()
    for out in outs:
        assert all(x.tobytes() == t.cpu().numpy().tobytes() for x, t in zip(one, out))


# ---- 5. point_normals --------------------------------------------------------------------------------------------------------------
def _normals_gpu(dev, x, idx=None, k=16):
    xt = _up(dev, x, f32)
    B, N = xt.shape[:2]
    rows = xt.view(B * N, 3)
    idx_t = ops.knn_pm(rows, B, N, k) if idx is None else _up(dev, idx, np.int32)
    n, flat = ops.point_normals(rows, idx_t, B, N, want_flatness=True)
    torch.cuda.synchronize()
    return n.cpu().numpy().reshape(B, N, 3), flat.cpu().numpy().reshape(B, N), idx_t.cpu().numpy()


def test_point_normals_against_eigh_and_both_forms(cuda, monkeypatch):
    x = np.stack([_patches(seed, 64, 64) for seed in (20, 21)])      # [2, 4096, 3]
    n, flat, idx = _normals_gpu(cuda, x)
    worst = 0.0
    for b in range(2):
        ref, gap = R.eigh_normals(x[b], idx[b])
        sel = gap >= NORMAL_MIN_GAP
        err = 1.0 - np.abs((n[b].astype(np.float64) * ref).sum(axis=1))
        worst = max(worst, float(err[sel].max()))
        assert sel.mean() > 0.8
        want_n, want_f = R.point_normals(x[b], idx[b])
        print(f"MEASURE icp/normals cloud {b}: bits equal to the restatement {np.array_equal(want_n.view(np.int32), n[b].view(np.int32))}, "
              f"largest difference {np.abs(want_n - n[b]).max():.2e}")
    print(f"MEASURE icp/normals device 1-|n.n_ref| max={worst:.3e} gate={NORMAL_GATE:.1e}")
    assert worst <= NORMAL_GATE
    monkeypatch.setenv("LPD_DEBUG", "normals-l2")      # the library reads it on every call: the L2 form whatever N
    n2, flat2, _ = _normals_gpu(cuda, x, idx=idx)
    assert np.array_equal(n.view(np.int32), n2.view(np.int32)) and np.array_equal(flat.view(np.int32), flat2.view(np.int32))
    monkeypatch.delenv("LPD_DEBUG")
    # a cloud too large for the LDS form, an odd size, and hand-made cases
    big = np.stack([_patches(22, 130, 64)])[:, :8200]
    nb, _, idxb = _normals_gpu(cuda, big)
    refb, gapb = R.eigh_normals(big[0], idxb[0])
    assert (1.0 - np.abs((nb[0].astype(np.float64) * refb).sum(axis=1)))[gapb >= NORMAL_MIN_GAP].max() <= NORMAL_GATE
    g = np.random.default_rng(23)
    flatc = np.column_stack((g.uniform(-5, 5, (300, 2)), np.zeros(300))).astype(f32)[None]
    nf, ff, idxf = _normals_gpu(cuda, flatc, k=12)
    assert np.array_equal(np.abs(nf[0]), np.tile(np.array([0, 0, 1], dtype=f32), (300, 1))) and not ff.any()
    bad = flatc.copy()
    bad[0, 7, 0], bad[0, 9, 2] = np.nan, np.inf
    same = np.zeros((1, 300, 12), dtype=np.int32) + np.arange(300, dtype=np.int32)[None, :, None]
    wild = idxf.copy()
    wild[0, :, 3] = np.where(np.arange(300) % 2 == 0, -5, 10 ** 6)
    for pts, lists in ((bad, idxf), (flatc, same), (flatc, wild)):
        got_n, got_f, _ = _normals_gpu(cuda, pts, idx=lists)
        want_n, want_f = R.point_normals(pts[0], lists[0])
        assert np.array_equal(np.abs(got_n[0]), np.abs(want_n)) and np.array_equal(got_f[0], want_f)
    assert not _normals_gpu(cuda, flatc, idx=same)[0].any()


@pytest.mark.parametrize("N", [4, 5, 17, 63, 64])
def test_point_normals_k_equal_to_n(cuda, N):
    g = np.random.default_rng(N)
    x = np.stack([np.column_stack((g.uniform(-2, 2, (N, 2)), g.normal(0, 0.01, N))) @ R.rot_xyz(0.3, -0.2, 0.5).T for _ in range(3)]).astype(f32)
    idx = np.stack([R.knn_lists(c, N) for c in x])
    n, flat, _ = _normals_gpu(cuda, x, idx=idx)
    used = 0
    for b in range(3):
        ref, gap = R.eigh_normals(x[b], idx[b])
        sel = gap >= NORMAL_MIN_GAP      # four points can be nearly collinear: such a cloud has no normal to compare
        used += int(sel.sum())
        if sel.any():
            assert (1.0 - np.abs((n[b].astype(np.float64) * ref).sum(axis=1)))[sel].max() <= NORMAL_GATE
        assert np.abs(np.linalg.norm(n[b].astype(np.float64), axis=1) - 1.0).max() < 2e-7
    assert used >= N


# (B, N, K): the cases of tests/test_local_features_gpu.py WALK_CASES -- one launch that stages cloud 0 in 16-byte pieces and cloud 1
# (804 bytes in) by the float, K on both sides of the int4 list read, a second tile with one live lane in either form
WALK_CASES = [(2, 67, 4), (2, 67, 5), (2, 67, 7), (2, 67, 8), (1, 513, 8), (1, 257, 8)]


@pytest.mark.parametrize("B,N,K", WALK_CASES)
def test_point_normals_every_read_path_gives_the_same_bits(cuda, monkeypatch, B, N, K):
    """The plain input is held to fp64 eigh (the gate of test_point_normals_k_equal_to_n); every other layout of the same input
    (walk_forms), and all of them again in the L2 form, give its bits in the normals and the flatness."""
    g = np.random.default_rng(1000 * N + K)
    x = np.stack([np.column_stack((g.uniform(-2, 2, (N, 2)), g.normal(0, 0.01, N))) @ R.rot_xyz(0.3, -0.2, 0.5).T for _ in range(B)]).astype(f32)
    idx = np.stack([R.knn_lists(c, K) for c in x])
    rows, idx_t = _up(cuda, x, f32).view(B * N, 3), _up(cuda, idx, np.int32)

    def run(r, i):
        n, flat = ops.point_normals(r, i, B, N, want_flatness=True)
        torch.cuda.synchronize()
        return n.cpu().numpy(), flat.cpu().numpy()
    base, fbase = run(rows, idx_t)
    used = 0
    for b in range(B):
        nb = base.reshape(B, N, 3)[b].astype(np.float64)
        ref, gap = R.eigh_normals(x[b], idx[b])
        sel = gap >= NORMAL_MIN_GAP      # a few neighbours can be nearly collinear: such a point has no normal to compare
        used += int(sel.sum())
        assert (1.0 - np.abs((nb * ref).sum(axis=1)))[sel].max() <= NORMAL_GATE
        assert np.abs(np.linalg.norm(nb, axis=1) - 1.0).max() < 2e-7
    assert 2 * used > B * N
    variants = walk_forms.forms(rows, idx_t)
    for l2 in (False, True):
        if l2:
            monkeypatch.setenv("LPD_DEBUG", "normals-l2")
        for name, r, i in variants + ([("plain", rows, idx_t)] if l2 else []):
            got, fgot = run(r, i)
            assert np.array_equal(got.view(np.int32), base.view(np.int32)) and np.array_equal(fgot.view(np.int32), fbase.view(np.int32)), \
                (name, "L2" if l2 else "LDS")


# ---- 6. the wrapper ----------------------------------------------------------------------------------------------------------------
def test_align_then_refine_on_street_scenes(cuda):
    scenes = [R.tilted_true_pair(s) for s in (0, 3, 7, 9)]
    a = _up(cuda, np.stack([s[0] for s in scenes]), f32)
    b = _up(cuda, np.stack([s[1] for s in scenes]), f32)
    pairs = torch.tensor([[0, 0], [1, 1], [2, 2], [3, 3], [0, 9]], dtype=torch.int64, device=cuda)
    al = verify.align_pairs(a, b, pairs)
    rf = verify.refine_pairs(a, b, pairs, init=al, want_nn=True)
    torch.cuda.synchronize()
    pose = rf.pose.cpu().numpy()
    for i, s in enumerate(scenes):
        M0 = al.matrix()[i].cpu().numpy()
        e0, e1 = R.pose_error(M0[:3].reshape(12), s[2], s[3]), R.pose_error(pose[i].reshape(12), s[2], s[3])
        print(f"MEASURE icp/wrapper scene {i}: alignment {e0[0]:.2f} deg {e0[1]:.3f} m -> refined {e1[0]:.3f} deg {e1[1]:.3f} m "
              f"(gates {QUALITY_GATE_DEG:.3f} deg {QUALITY_GATE_M:.3f} m) share {float(rf.inlier_share[i]):.3f} rms {float(rf.rms[i]):.4f} m")
        assert e1[0] < QUALITY_GATE_DEG and e1[1] < QUALITY_GATE_M and e0[0] > 1.0
    assert rf.valid.tolist() == [True] * 4 + [False] and rf.steps.tolist() == [8] * 4 + [0] and rf.refused.tolist() == [0] * 5
    assert rf.pose.shape == (5, 3, 4) and rf.sums.shape == (5, 9, 32) and rf.nn.shape == (5, 4096) and rf.pose.dtype == torch.float64
    assert torch.equal(rf.inliers, rf.sums[:, -1, 0].to(torch.int32)) and (rf.inlier_share[:4] > 0.8).all() and (rf.rms[:4] < 0.12).all()
    assert float(rf.rms[4]) == 0.0 and int(rf.inliers[4]) == 0 and (rf.nn[4] == -1).all()
    want_rms = [R.rms(rf.sums[i, -1].cpu().numpy()) for i in range(4)]
    assert np.allclose(rf.rms[:4].cpu().numpy(), want_rms, rtol=1e-12)


def test_refinement_matrix_and_init_layouts(cuda):
    g = np.random.default_rng(17)
    A, B = _tables(600, seed=1)
    a, b = _up(cuda, A, f32), _up(cuda, B, f32)
    pairs = torch.tensor([[0, 0], [1, 2], [0, 1]], dtype=torch.int32, device=cuda)
    start = np.stack([_small_pose(g, 0.04, 0.4) for _ in range(3)])
    ca, cb = g.uniform(-100, 100, (2, 3)), g.uniform(-100, 100, (3, 3))
    search = verify.RefineSearch(iterations=3, dmax=[1.5, 1.0, 0.8])
    full = np.concatenate((start.reshape(3, 3, 4), np.tile(np.array([[[0, 0, 0, 1.0]]]), (3, 1, 1))), axis=1)
    outs = [verify.refine_pairs(a, b, pairs, init=_up(cuda, init, np.float64), search=search, center_a=_up(cuda, ca, np.float64),
                                center_b=_up(cuda, cb, np.float64)) for init in (start, start.reshape(3, 3, 4), full)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.pose, outs[0].pose) and torch.equal(o.sums, outs[0].sums)
    want = R.icp_pairs(A, B, _device_normals(cuda, B), pairs.cpu().numpy(), start, list(search.schedule), search.min_inliers)
    assert outs[0].pose.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(outs[0].sums.cpu().numpy(), want[2].transpose(1, 0, 2))
    M = outs[0].matrix().cpu().numpy()
    pr = pairs.cpu().numpy()
    for p in range(3):
        Pm = want[0][p].reshape(3, 4)
        hand = np.eye(4)
        hand[:3, :3] = Pm[:, :3]
        hand[:3, 3] = Pm[:, 3] - Pm[:, :3] @ ca[pr[p, 0]] + cb[pr[p, 1]]
        assert np.abs(M[p] - hand).max() < 1e-12 and M[p, 3].tolist() == [0, 0, 0, 1]
    ident = verify.refine_pairs(a, b, pairs, search=verify.RefineSearch(iterations=0))
    assert ident.pose.cpu().numpy().tobytes() == np.tile(np.eye(3, 4), (3, 1, 1)).tobytes() and ident.nn is None


def test_candidates_with_and_without_refinement(cuda):
    A, B = _tables(1000, TA=2, TB=4, seed=2)
    q, db = _up(cuda, A, f32), _up(cuda, B, f32)
    topk = torch.tensor([[0, 3, -1], [2, -1, 1]], dtype=torch.int64, device=cuda)
    search = verify.AlignSearch(yaw_steps=16, fine_div=2)
    plain = verify.verify_candidates(q, db, topk, search, min_overlap=0.2)
    v = verify.refine_candidates(q, db, topk, search, min_overlap=0.2, refine=verify.RefineSearch(iterations=2))
    torch.cuda.synchronize()
    assert plain.refinement is None
    # verify_candidates does what it did: every field equal to the calls it is made of; refine_candidates adds .refinement to the same
    rows = torch.tensor([[0, 0], [0, 3], [-1, -1], [1, 2], [-1, -1], [1, 1]], dtype=torch.int64, device=cuda)
    al = verify.align_pairs(q, db, rows, search)
    for name in verify.Alignment.__slots__:
        x, y, z = getattr(plain, name), getattr(al, name), getattr(v, name)
        assert (x is None and y is None and z is None) or (torch.equal(x.reshape(y.shape), y) and torch.equal(x, z)), name
    key = torch.where(al.valid, al.score, torch.full_like(al.score, -1)).reshape(2, 3)
    assert torch.equal(plain.order, torch.sort(key, dim=1, descending=True, stable=True).indices) and torch.equal(plain.order, v.order)
    assert torch.equal(plain.accepted, (al.valid & (al.overlap >= 0.2)).reshape(2, 3)) and torch.equal(plain.accepted, v.accepted)
    rf = v.refinement
    assert rf.pose.shape == (2, 3, 3, 4) and rf.valid.shape == (2, 3) and rf.sums.shape == (2, 3, 3, 32) and rf.matrix().shape == (2, 3, 4, 4)
    assert rf.valid.tolist() == [[True, True, False], [True, False, True]] and torch.equal(rf.valid, v.valid)
    assert (rf.steps + rf.refused)[rf.valid].tolist() == [2] * 4 and (rf.steps[~rf.valid] == 0).all() and (rf.inliers[~rf.valid] == 0).all()
    flat = verify.refine_pairs(q, db, rows, init=al, search=verify.RefineSearch(iterations=2))
    assert torch.equal(flat.pose.reshape(2, 3, 3, 4), rf.pose)
