"""lpd_drive_correct / lpd_map_insert / lpd_map_rehash, their ops wrappers and lpdnet_hip/mapping.py on the GPU against tests/map_ref.py.

The corrected poses (bits) and their counters, and -- after the extraction -- the keys, counts, integer sums, fp32 points (bits) and
counters of a map equal the numpy restatement EXACTLY in every case.  Two cases compare with the extended-precision restatement
instead, within the bounds of tests/map_cases.py, and one (a table that is too small) asserts the counters' sum alone, as the
definition does."""
import os

import numpy as np
import pytest
import torch

import drive_ref
import map_cases as C
import map_ref as M
import pgo_ref as R

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
IDENT = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
_REFS = {}


def _ref(name, *args, **kw):
    """the restatement's map of a case, computed once and shared (read-only)"""
    if name not in _REFS:
        _REFS[name] = M.insert(*args, **kw)
    return _REFS[name]


def _device_points(cuda, pts, ld=3, misaligned=False):
    rows = pts.shape[0]
    host = np.full((max(rows, 1), ld), 9.5, dtype=f32)
    host[:rows, :3] = pts
    if not misaligned:
        return torch.from_numpy(host).to(cuda)
    base = torch.empty((host.size + 1,), dtype=torch.float32, device=cuda)
    view = base[1:].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 4
    return view


def _insert(cuda, pts, off, poses, origin, cell, capacity=1 << 13, ld=3, misaligned=False, scans=(0, None), table=None):
    """ops.map_insert into a new (or the given) table -> (keys, acc, info)"""
    from lpdnet_hip import ops
    table = ops.map_table(capacity, cuda) if table is None else table
    ops.map_insert(_device_points(cuda, pts, ld, misaligned), torch.from_numpy(np.asarray(off, dtype=np.int32)).to(cuda),
                   torch.from_numpy(np.ascontiguousarray(poses, dtype=f64).reshape(-1, 12)).to(cuda),
                   torch.from_numpy(np.asarray(origin, dtype=f64)).to(cuda), ops.map_inv_cell(cell), *table, scans[0], scans[1])
    return table


def _extract(table, cell=1.0):
    from lpdnet_hip import mapping
    c = mapping.extract_cells(table[0], table[1], None, cell)
    return dict(keys=c.keys.cpu().numpy(), counts=c.counts.cpu().numpy(), sums=c.sums.cpu().numpy(), points=c.points.cpu().numpy(),
                info=table[2].cpu().numpy())


def _check(got, want, what):
    assert got["info"].tolist() == want.info.tolist(), (what, got["info"], want.info)
    assert np.array_equal(got["keys"], want.keys), what
    assert np.array_equal(got["counts"], want.counts), what
    assert np.array_equal(got["sums"], want.sums), what
    assert got["points"].tobytes() == want.points.tobytes(), what


def _scene(seed, lengths, scale=20.0, origin=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=i64)
    pts, poses = drive_ref.make_drive(rng, lengths, origin=origin, point_scale=scale)
    return pts, M.offsets_of(lengths), poses, poses[0, M.TRA].copy()


# ---- lpd_map_insert ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, M.CHUNK - 1, M.CHUNK, M.CHUNK + 1])
@pytest.mark.parametrize("cell", [0.5, 4.0])
def test_one_scan_of_n_rows(cuda, rows, cell):
    pts, off, poses, origin = _scene(100 + rows, [rows])
    want = _ref(("one", rows, cell), pts, off, poses, origin, cell)
    _check(_extract(_insert(cuda, pts, off, poses, origin, cell)), want, (rows, cell))


def test_4096_rows_in_one_cell_and_in_4096_cells(cuda):
    rng = np.random.default_rng(7)
    off = np.array([0, 1500, 4096], dtype=np.int32)
    poses = np.tile(IDENT, (2, 1))
    one = rng.uniform(0.05, 0.95, (4096, 3)).astype(f32) + f32([3.0, -2.0, 1.0])
    want = _ref("one cell", one, off, poses, np.zeros(3), 1.0)
    assert len(want.keys) == 1 and want.counts.tolist() == [4096]
    _check(_extract(_insert(cuda, one, off, poses, np.zeros(3), 1.0)), want, "one cell")
    g = np.arange(16, dtype=f32)
    many = np.stack(np.meshgrid(g, g - 8, g - 3, indexing="ij"), axis=-1).reshape(-1, 3) + f32(0.25)
    many = many[rng.permutation(4096)]
    want = _ref("4096 cells", many, off, poses, np.zeros(3), 1.0)
    assert len(want.keys) == 4096 and want.counts.max() == 1      # 1024 distinct keys a chunk: the workgroup's table spills
    _check(_extract(_insert(cuda, many, off, poses, np.zeros(3), 1.0, capacity=1 << 14)), want, "4096 cells")


def test_negative_coordinates_cell_boundaries_and_dropped_rows(cuda):
    cell = 0.25
    k = np.arange(-40, 41, dtype=f32)
    b = k * f32(cell)
    edge = np.concatenate((b, np.nextafter(b, f32(np.inf)), np.nextafter(b, f32(-np.inf)), f32([0.0, -0.0])))
    pts = np.stack((edge, edge[::-1], np.roll(edge, 7)), axis=1)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e5, 0, 0], [0, -3e5, 0], [0, 0, 262144.0], [0, 0, -262144.25], [1e30, 1, 1],
                    [np.nan, np.nan, np.nan]], dtype=f32)
    pts = np.concatenate((pts[:100], bad, pts[100:]))
    off = np.array([0, 10, 10, 200, len(pts)], dtype=np.int32)
    poses = np.tile(IDENT, (4, 1))
    want = _ref("edges", pts, off, poses, np.zeros(3), cell)
    assert want.info[1] == 9      # all nine: 262144.0 / 0.25 = 2^20 is the first cell beyond the range, -262144.25 / 0.25 the last below
    _check(_extract(_insert(cuda, pts, off, poses, np.zeros(3), cell), cell), want, "edges")


def test_empty_scans_ld_and_alignment(cuda):
    lengths = [0, 0, 300, 0, 1, 2000, 0, 77, 0]
    pts, off, poses, origin = _scene(3, lengths)
    want = _ref("empty scans", pts, off, poses, origin, 1.0)
    for ld, mis in ((3, False), (3, True), (4, False), (4, True), (6, False)):
        _check(_extract(_insert(cuda, pts, off, poses, origin, 1.0, ld=ld, misaligned=mis)), want, (ld, mis))
    # scans of a handful of rows: more than 64 of them in a chunk
    lengths = np.random.default_rng(4).integers(0, 9, 700)
    pts, off, poses, origin = _scene(5, lengths)
    _check(_extract(_insert(cuda, pts, off, poses, origin, 0.5)), _ref("short scans", pts, off, poses, origin, 0.5), "short scans")


def test_a_broken_offsets_table_is_not_read(cuda):
    lengths = np.full(30, 100)
    pts, off, poses, origin = _scene(6, lengths)
    bad = off.copy()
    bad[12] = bad[13] + 5      # descends inside the second chunk
    want = _ref("broken", pts, bad, poses, origin, 1.0)
    assert 0 < want.info[1] < 3000 and want.info[0] + want.info[1] == 3000
    _check(_extract(_insert(cuda, pts, bad, poses, origin, 1.0)), want, "broken")
    for lo, hi in ((0, 3001), (-1, 3000), (200, 100)):      # the call reads nothing
        worse = off.copy()
        worse[0], worse[-1] = lo, hi
        t = _insert(cuda, pts, worse, poses, origin, 1.0)
        assert t[2].tolist() == [0, 0, 0, 0] and int((t[0] >= 0).sum()) == 0


def test_probe_sequences_wrap_past_the_end_of_the_table(cuda):
    cap = 64
    q = np.stack(np.meshgrid(np.arange(-20, 20), np.arange(-20, 20), np.arange(-2, 3), indexing="ij"), axis=-1).reshape(-1, 3)
    at_end = q[M.slot(M.key(q), cap) >= cap - 2][:12]      # twelve cells that start probing in the last two slots
    assert len(at_end) == 12
    pts = np.repeat(at_end.astype(f32) + f32(0.5), 3, axis=0)
    off = np.array([0, len(pts)], dtype=np.int32)
    want = _ref("wrap", pts, off, IDENT[None], np.zeros(3), 1.0)
    t = _insert(cuda, pts, off, IDENT[None], np.zeros(3), 1.0, capacity=cap)
    _check(_extract(t), want, "wrap")
    keys = t[0].cpu().numpy()
    assert keys[cap - 1] >= 0 and (keys[:10] >= 0).all()      # the run wrapped round into the first slots


def test_a_full_table_loses_rows_and_says_so(cuda):
    g = np.arange(17, dtype=f32)
    pts = np.stack((g, 0 * g, 0 * g), axis=1) + f32(0.5)
    t = _insert(cuda, np.repeat(pts, 2, axis=0), np.array([0, 34], dtype=np.int32), IDENT[None], np.zeros(3), 1.0, capacity=16)
    info = t[2].tolist()
    assert info[2] >= 1 and info[0] + info[1] + info[2] == 34


def test_batches_streams_forms_and_repeats_give_one_map(cuda):
    from lpdnet_hip import ops
    CAP = 1 << 14      # 7177 cells
    lengths = np.random.default_rng(8).integers(0, 400, 40)
    pts, off, poses, origin = _scene(9, lengths, scale=8.0)
    want = _ref("batches", pts, off, poses, origin, 0.5)
    whole = _extract(_insert(cuda, pts, off, poses, origin, 0.5, capacity=CAP), 0.5)
    _check(whole, want, "one call")
    # the same call into a cleared table: the same extracted bits
    again = _extract(_insert(cuda, pts, off, poses, origin, 0.5, capacity=CAP), 0.5)
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    # two calls over halves of the scans
    t = _insert(cuda, pts, off, poses, origin, 0.5, capacity=CAP, scans=(0, 17))
    _check(_extract(_insert(cuda, pts, off, poses, origin, 0.5, scans=(17, 40), table=t), 0.5), want, "two calls")
    # every row straight to the table
    old = os.environ.get("LPD_DEBUG")
    os.environ["LPD_DEBUG"] = (old + "," if old else "") + "map-direct"
    try:
        direct = _extract(_insert(cuda, pts, off, poses, origin, 0.5, capacity=CAP), 0.5)
    finally:
        if old is None:
            del os.environ["LPD_DEBUG"]
        else:
            os.environ["LPD_DEBUG"] = old
    _check(direct, want, "map-direct")
    # two tables on two streams
    tables = [ops.map_table(CAP, cuda), ops.map_table(2 * CAP, cuda)]
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    torch.cuda.synchronize()
    for half in ((0, 17), (17, 40)):
        for s, tb in zip(streams, tables):
            with torch.cuda.stream(s):
                _insert(cuda, pts, off, poses, origin, 0.5, table=tb, scans=half)
    torch.cuda.synchronize()
    for tb in tables:
        _check(_extract(tb, 0.5), want, "two streams")


def test_rows_at_a_utm_origin_stay_within_the_bound_of_extended_precision(cuda):
    points, lengths, poses, origin = C.utm_case()
    off = M.offsets_of(lengths)
    cell = 2.0 ** -6      # most rows have a cell of their own
    want = _ref("utm", points, off, poses, origin, cell)
    got = _extract(_insert(cuda, points, off, poses, origin, cell, capacity=1 << 15), cell)
    _check(got, want, "utm")
    w, _, _ = M.rows_of(points, off, poses, origin)
    k, _, _ = M.keyed(w, M.inv_cell(cell))
    ext = M.rows_ext(points, off, poses, origin)
    at = np.searchsorted(got["keys"], k)
    alone = got["counts"][at] == 1
    assert alone.sum() > len(k) // 2
    # a cell of one row holds rint(w 2^16) / 2^16 rounded to fp32: within 2^-17 + half an fp32 ulp below 128 m (2^-18) of the fp32 row
    err = np.abs(got["points"][at][alone].astype(np.longdouble) - ext[alone]).max()
    assert err <= C.ROWS_BOUND + 1.5 * 2.0 ** -17, err


# ---- lpd_drive_correct ---------------------------------------------------------------------------------------------------------------------
def _correct(cuda, poses, D, ns, X):
    from lpdnet_hip import ops
    out, info = ops.drive_correct(torch.from_numpy(np.ascontiguousarray(poses)).to(cuda), torch.from_numpy(np.asarray(D, dtype=i64)).to(cuda),
                                  torch.from_numpy(np.asarray(ns, dtype=np.int32)).to(cuda), torch.from_numpy(np.ascontiguousarray(X)).to(cuda))
    return out.cpu().numpy(), info.cpu().numpy()


def _same_poses(got, want, what):
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def _moved(rng, poses):
    return np.array([R.mul12(p, R.pose12(R.rot_of(rng.normal(0.0, 0.02, 3)), rng.normal(0.0, 0.5, 3))) for p in poses])


CORRECT = {
    "S1": (1, [0]), "S63 ends": (63, [0, 62]), "S64 one": (64, [10]), "S65 duplicates": (65, [3, 3, 20, 20, 20, 64]),
    "S700 many": (700, sorted(set(range(0, 700, 37)) | {699}) + [699]), "S700 every scan": (700, list(range(700))),
}


@pytest.mark.parametrize("name", list(CORRECT))
def test_corrected_poses_equal_the_restatement(cuda, name):
    S, ns = CORRECT[name]
    rng = np.random.default_rng(S)
    _, poses = drive_ref.make_drive(rng, np.ones(S, dtype=i64), origin=(5.7e6, 6.2e5, 0.0))
    D = drive_ref.distance(drive_ref.steps(poses))
    ns = np.array(sorted(ns), dtype=np.int32)
    X = _moved(rng, poses[ns])
    want, winfo = M.correct(poses, D, ns, X)
    got, info = _correct(cuda, poses, D, ns, X)
    _same_poses(got, want, name)
    assert info.tolist() == winfo.tolist() == [S, 0]


def test_standing_still_nan_poses_and_tables_that_are_not_one(cuda):
    rng = np.random.default_rng(12)
    S = 300
    _, poses = drive_ref.make_drive(rng, np.ones(S, dtype=i64))
    poses[100:120] = poses[100]
    poses[200:230, M.TRA] = poses[200, M.TRA]
    D = drive_ref.distance(drive_ref.steps(poses))
    ns = np.array([0, 100, 119, 150, 200, 229, 299], dtype=np.int32)
    X = _moved(rng, poses[ns])
    for what, p, x, n in (("still", poses, X, ns), ("nan pose", _with(poses, (130, 5), np.nan), X, ns), ("nan node", poses, _with(X, (3, 7), np.nan), ns),
                          ("inf at a node's scan", _with(poses, (200, 3), np.inf), X, ns), ("unsorted", poses, X, ns[[3, 0, 6, 1, 2, 5, 4]]),
                          ("outside", poses, X, np.array([-5, 100, 119, 150, 200, 229, 4000], dtype=np.int32))):
        want, winfo = M.correct(p, D, n, x)
        got, info = _correct(cuda, p, D, n, x)
        _same_poses(got, want, what)
        assert info.tolist() == winfo.tolist() and info.sum() == S, what
        if what not in ("still", "unsorted"):      # an unsorted table may still give every scan a bracket that is one
            assert info[1] > 0, what


def _with(a, at, v):
    a = a.copy()
    a[at] = v
    return a


def test_nodes_that_did_not_move_leave_the_drive_within_the_bound(cuda):
    poses, D, ns = C.unmoved_case()
    got, info = _correct(cuda, poses, D, ns, poses[ns])
    assert info.tolist() == [len(poses), 0]
    assert np.abs(got[:, M.ROT] - poses[:, M.ROT]).max() <= C.CORRECT_ROT_BOUND
    assert np.abs(got[:, M.TRA] - poses[:, M.TRA]).max() <= C.CORRECT_TRANS_BOUND * np.abs(poses[:, M.TRA]).max()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------------
def test_voxel_map_grows_and_is_incremental(cuda):
    from lpdnet_hip import mapping
    lengths = np.random.default_rng(13).integers(50, 400, 30)
    pts, off, poses, origin = _scene(14, lengths, scale=15.0)
    want = _ref("voxel map", pts, off, poses, origin, 0.5)
    tp, tl, tposes = torch.from_numpy(pts).to(cuda), lengths, torch.from_numpy(poses).to(cuda)
    big = mapping.build_map(tp, tl, tposes, cell=0.5)      # origin: the first pose's translation
    small = mapping.VoxelMap(0.5, capacity=256, device=cuda).insert(tp, tl, tposes)
    assert small.grown >= 1 and big.grown == 0 and small.capacity >= 2 * len(want.keys) > 512
    for m in (big, small):
        c = m.cells()
        got = dict(keys=c.keys.cpu().numpy(), counts=c.counts.cpu().numpy(), sums=c.sums.cpu().numpy(), points=c.points.cpu().numpy(),
                   info=m.info.cpu().numpy())
        _check(got, want, "VoxelMap")
        assert m.occupied == len(want.keys) and m.inserted == want.info[0] and m.dropped == 0 and c.cell == 0.5
        assert c.origin.cpu().numpy().tobytes() == origin.tobytes() and c.points.dtype == torch.float32 and c.points.device == tposes.device
    # incremental, growing from a copy in the second call
    inc = mapping.VoxelMap(0.5, origin=origin, capacity=1 << 10, device=cuda)
    inc.insert(tp, tl, tposes, scans=(0, 2))
    first_cap = inc.capacity
    inc.insert(tp, tl, tposes, scans=range(2, 30))
    assert inc.capacity > first_cap
    c = inc.cells()
    got = dict(keys=c.keys.cpu().numpy(), counts=c.counts.cpu().numpy(), sums=c.sums.cpu().numpy(), points=c.points.cpu().numpy(), info=inc.info.cpu().numpy())
    _check(got, want, "incremental")


def test_corrected_poses_go_back_into_the_drive_step(cuda):
    from lpdnet_hip import drive, mapping
    rng = np.random.default_rng(15)
    lengths = rng.integers(20, 60, 120)
    pts, poses = drive_ref.make_drive(rng, lengths, step=1.0)
    tp, tposes = torch.from_numpy(pts).to(cuda), torch.from_numpy(poses).to(cuda)
    plan = drive.plan_windows(tposes, 20.0, 10.0, lengths=lengths)
    ref = plan.ref.cpu().numpy()
    assert (ref >= 0).all() and len(ref) >= 5
    nodes = _moved(rng, poses[ref])
    fixed = mapping.correct_scan_poses(plan, tposes, torch.from_numpy(nodes).to(cuda).reshape(-1, 3, 4))
    assert fixed.dtype == torch.float64 and fixed.device == tposes.device and tuple(fixed.shape) == (120, 12)
    want, _ = M.correct(poses, plan.distance.cpu().numpy(), ref, nodes)
    _same_poses(fixed.cpu().numpy(), want, "correct_scan_poses")
    rows = drive.accumulate(tp, lengths, poses=fixed)
    assert rows.points.dtype == torch.float32 and rows.points.device == tposes.device and rows.points.shape[0] > 0


def test_argument_errors_name_their_function(cuda):
    from lpdnet_hip import drive, mapping, ops
    p = torch.zeros((4, 12), dtype=torch.float64, device=cuda)
    D = torch.zeros(4, dtype=torch.int64, device=cuda)
    ns = torch.zeros(1, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="drive_correct: D"):
        ops.drive_correct(p, D[:3], ns, p[:1])
    with pytest.raises(ValueError, match="drive_correct: node_scan"):
        ops.drive_correct(p, D, torch.zeros(5, dtype=torch.int32, device=cuda), p[:1])
    with pytest.raises(ValueError, match="drive_correct: node_pose"):
        ops.drive_correct(p, D, ns, p[:2])
    with pytest.raises(TypeError, match="node_scan"):
        ops.drive_correct(p, D, ns.to(torch.int64), p[:1])
    keys, acc, info = ops.map_table(16, cuda)
    pts = torch.zeros((5, 3), device=cuda)
    off = torch.tensor([0, 1, 2, 3, 5], dtype=torch.int32, device=cuda)
    org = torch.zeros(3, dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError, match="map_insert: scans"):
        ops.map_insert(pts, off, p, org, 1.0, keys, acc, info, 2, 2)
    with pytest.raises(ValueError, match="map_insert: inv_cell"):
        ops.map_insert(pts, off, p, org, 4096.0, keys, acc, info)
    with pytest.raises(ValueError, match="map_insert: keys"):
        ops.map_insert(pts, off, p, org, 1.0, keys[:12], acc, info)
    with pytest.raises(ValueError, match="map_insert: acc"):
        ops.map_insert(pts, off, p, org, 1.0, keys, acc[:, :3], info)
    with pytest.raises(ValueError, match="map_insert: origin"):
        ops.map_insert(pts, off, p, org[:2], 1.0, keys, acc, info)
    with pytest.raises(ValueError, match="map_rehash: the new table"):
        ops.map_rehash(keys, acc, keys, acc, info)
    with pytest.raises(ValueError, match="VoxelMap.insert: scans"):
        mapping.VoxelMap(1.0, device=cuda).insert(pts, [1, 1, 1, 2], p, scans=(3, 9))
    with pytest.raises(ValueError, match="VoxelMap: origin"):
        mapping.VoxelMap(1.0, origin=[0.0, 1.0], device=cuda)
    with pytest.raises(ValueError, match="VoxelMap: capacity"):
        mapping.VoxelMap(1.0, capacity=100, device=cuda)
    plan = drive.plan_windows(torch.from_numpy(drive_ref.make_drive(np.random.default_rng(1), np.ones(50, dtype=i64))[1]).to(cuda), 10.0, 5.0)
    with pytest.raises(ValueError, match="correct_scan_poses: one pose per window"):
        mapping.correct_scan_poses(plan, plan.poses, p)
    with pytest.raises(TypeError, match="correct_scan_poses: result"):
        mapping.correct_scan_poses(plan, plan.poses, p.float())
    # every wrapper of the map and its localisation through every check they share: ONE wrong argument a call, the exception and the
    # words "<wrapper>: <argument>" (tests/test_odometry_gpu.py has the table of map_crop, map_touch and map_surface_touched)
    k2, a2, _ = ops.map_table(32, cuda)
    surf = torch.zeros((16, 8), device=cuda)
    surf_off = torch.zeros((16 * 8 + 1,), device=cuda)[1:].view(16, 8)      # one float off a 16-byte boundary
    assert surf_off.is_contiguous() and surf_off.data_ptr() % 16 == 4
    good = dict(drive_correct=dict(poses=p, D=D, node_scan=ns, node_pose=p[:1]),
                map_insert=dict(points=pts, offsets=off, poses=p, origin=org, inv_cell=1.0, keys=keys, acc=acc, info=info),
                map_rehash=dict(keys_in=k2, acc_in=a2, keys=keys, acc=acc, info=info),
                map_surface=dict(keys=keys, acc=acc),
                map_localize=dict(points=pts, offsets=off, poses=p, origin=org, inv_cell=1.0, keys=keys, surf=surf, dmax=(1.0, 1.0)))
    wrong = [("map_insert", dict(keys=keys[:12]), "keys"), ("map_rehash", dict(keys=keys[:12]), "keys"), ("map_rehash", dict(keys_in=k2[:12]), "keys"),
             ("map_surface", dict(keys=keys[:12]), "keys"), ("map_localize", dict(keys=keys[:12]), "keys"),
             ("map_insert", dict(acc=acc[:, :3]), "acc"), ("map_rehash", dict(acc=acc[:, :3]), "acc"), ("map_rehash", dict(acc_in=a2[:, :3]), "acc"),
             ("map_surface", dict(acc=acc[:, :3]), "acc"),
             ("map_localize", dict(surf=surf_off), "surf"),
             ("map_insert", dict(scan0=2, scan1=2), "scans"), ("map_localize", dict(scan0=2, scan1=2), "scans"),
             ("map_insert", dict(inv_cell=4096.0), "inv_cell"), ("map_localize", dict(inv_cell=4096.0), "inv_cell"),
             ("map_insert", dict(origin=org[:2]), "origin"), ("map_localize", dict(origin=org[:2]), "origin"),
             ("map_rehash", dict(keys_in=keys, acc_in=acc), "the new table"),
             ("drive_correct", dict(info=torch.zeros(3, dtype=torch.int32, device=cuda)), "info"), ("map_insert", dict(info=info[:3]), "info"),
             ("map_rehash", dict(info=info[:3]), "info"), ("map_surface", dict(info=torch.zeros(3, dtype=torch.int64, device=cuda)), "info")]
    for name, args in good.items():
        getattr(ops, name)(**args)      # the table's calls are good ones but for the one argument
    for name, bad, arg in wrong:
        with pytest.raises(ValueError, match=f"{name}: {arg}"):
            getattr(ops, name)(**dict(good[name], **bad))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_closing_the_loops_on_the_device_brings_the_laps_together_in_the_map(cuda):
    """pgo_ref.two_laps(1, 64), three scans to a node: PoseGraph.optimize, correct_scan_poses, build_map.  The occupied cells satisfy the
    condition of test_map_cpu.py and equal the restatement's for the device's own poses.  (V = 64 is the smallest of 48 / 64 at which
    the restatement meets the condition for the seeds 1, 2, 3: 0.61, 0.59, 0.54; at V = 48 seed 3 gives 0.46.)"""
    from lpdnet_hip import drive, mapping, posegraph
    c = C.lap_case(1, 64)
    g = c["graph"]
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)      # noqa: E731
    res = posegraph.PoseGraph(dev(g["start"]), (dev(g["edge"]), dev(g["meas"]), dev(g["weight"]))).optimize(**R.QUALITY_SOLVER)
    start = dev(c["start"])
    plan = drive.DrivePlan()      # the nodes are every third scan: a plan whose windows' reference scans are the nodes
    plan.ref = dev(c["node_scan"])
    plan.first, plan.poses, plan.distance = plan.ref, start, None
    fixed = mapping.correct_scan_poses(plan, dev(c["start"].copy()), res)
    pts = dev(c["points"])
    counts = [mapping.build_map(pts, c["lengths"], p, cell=1.0).occupied for p in (dev(c["gt"]), start, fixed)]
    m_true, m_start, m_solved = counts
    assert m_start > m_solved and (m_start - m_solved) / (m_start - m_true) >= 0.5, counts
    assert counts == list(M.quality(c["points"], c["lengths"], c["gt"], c["start"], fixed.cpu().numpy(), cell=1.0)[:3])
