"""lpd_map_surface / lpd_map_localize, their ops wrappers and lpdnet_hip/mapping.py's localisation on the GPU against tests/loc_ref.py.

Two kinds of equality with the restatement: per key, after a sort by key, the bits of the surf rows; and EXACTLY the sums, info, cell and
the bits of the poses of a localisation -- at every table size and slot placement.  The end-to-end case also stays within the bounds
that tests/test_localize_cpu.py measured on the restatement (tests/loc_cases.py)."""
import numpy as np
import pytest
import torch

import icp_ref as I
import loc_cases as C
import loc_ref as L
import map_ref as M

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
_REFS = {}


def _ref(name, make):
    """a restatement's result, computed once and shared (read-only)"""
    if name not in _REFS:
        _REFS[name] = make()
    return _REFS[name]


# ---- a small world: a floor and two walls ----------------------------------------------------------------------------------------------------
def _world(rng, n):
    kind = rng.integers(0, 4, n)
    a, b, h, e = rng.uniform(-10.0, 10.0, n), rng.uniform(-10.0, 10.0, n), rng.uniform(0.0, 5.0, n), rng.normal(0.0, 0.02, n)
    floor = np.stack((a, b, 0.4 + e), axis=1)      # inside one layer of 1 m cells
    wall_x = np.stack((7.3 + e, b, h), axis=1)
    wall_y = np.stack((a, -5.6 + e, h), axis=1)
    return np.where((kind < 2)[:, None], floor, np.where((kind == 2)[:, None], wall_x, wall_y))


def _pose(rng, origin, tilt=0.02, spread=2.0):
    R = I.rot_xyz(rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(0.0, 2.0 * np.pi))
    return R, np.asarray(origin, dtype=f64) + np.array([rng.uniform(-spread, spread), rng.uniform(-spread, spread), 1.5])


def _scan(rng, n, R, t, origin):
    return ((_world(rng, n) + np.asarray(origin, dtype=f64) - t) @ R).astype(f32)


def _map_case(origin=(0.0, 0.0, 0.0), cell=1.0, seed=50, scans=4, rows=4000):
    """-> (points, offsets, poses, origin, cell, Cells) of the map scans at their true poses"""
    def make():
        rng = np.random.default_rng(seed)
        poses, pts = [], []
        for _ in range(scans):
            R, t = _pose(rng, origin)
            poses.append(C.pose12(R, t))
            pts.append(_scan(rng, rows, R, t, origin))
        pts, poses, off, org = np.concatenate(pts), np.array(poses), M.offsets_of([rows] * scans), np.asarray(origin, dtype=f64)
        return pts, off, poses, org, cell, M.insert(pts, off, poses, org, cell)
    return _ref(("map", tuple(origin), cell, seed, scans, rows), make)


def _query_case(seed, lengths, origin=(0.0, 0.0, 0.0), rot=0.02, shift=0.2):
    """-> (points, offsets, start poses [S, 12]): fresh scans of the same world, started a little off"""
    rng = np.random.default_rng(seed)
    pts, start = [], []
    for n in lengths:
        R, t = _pose(rng, origin)
        pts.append(_scan(rng, int(n), R, t, origin))
        dR = I.rot_xyz(*rng.uniform(-rot, rot, 3))
        start.append(C.pose12(dR @ R, t + rng.uniform(-shift, shift, 3)))
    return np.concatenate(pts) if len(pts) else np.zeros((0, 3), dtype=f32), M.offsets_of(lengths), np.array(start)


# ---- to the device and back ------------------------------------------------------------------------------------------------------------------
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


def _t(cuda, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def _table(cuda, mp, capacity, scans=(0, None), table=None):
    from lpdnet_hip import ops
    pts, off, poses, origin, cell, _ = mp
    table = ops.map_table(capacity, cuda) if table is None else table
    ops.map_insert(_device_points(cuda, pts), _t(cuda, off, np.int32), _t(cuda, poses, f64), _t(cuda, origin, f64), ops.map_inv_cell(cell), *table,
                   scans[0], scans[1])
    return table


def _by_key(keys, surf):
    keys, surf = keys.cpu().numpy(), surf.cpu().numpy()
    live = keys >= 0
    order = np.argsort(keys[live])
    return keys[live][order], surf[live][order], surf[~live]


def _surface(cuda, table, want, reach=1, min_cells=5):
    """ops.map_surface, checked per key against the restatement's Surface -> surf on the device"""
    from lpdnet_hip import ops
    surf, info = ops.map_surface(table[0], table[1], reach, min_cells)
    k, rows, empty = _by_key(table[0], surf)
    assert np.array_equal(k, want.keys)
    assert rows.tobytes() == want.rows().tobytes(), np.argwhere(rows.view(np.uint32) != want.rows().view(np.uint32))[:4]
    assert not empty.any() and empty.view(np.uint32).max(initial=0) == 0
    bare = (want.normals == 0).all(axis=1)
    assert info.tolist() == [int((~bare).sum()), int(bare.sum())]
    return surf


def _localize(cuda, table, surf, pts, off, poses, origin, cell, dmax, min_inliers=50, max_flat=0.3, scans=(0, None), ld=3, misaligned=False,
              points=None):
    from lpdnet_hip import ops
    points = _device_points(cuda, pts, ld, misaligned) if points is None else points
    pose, info, sums, cells = ops.map_localize(points, _t(cuda, off, np.int32), _t(cuda, poses, f64), _t(cuda, origin, f64), ops.map_inv_cell(cell),
                                               table[0], surf, dmax, min_inliers, max_flat, scans[0], scans[1], want_cells=True)
    return dict(pose=pose.cpu().numpy(), info=info.cpu().numpy(), sums=sums.cpu().numpy(), cell=cells.cpu().numpy())


def _check(got, want, what, rows=None):
    assert got["info"].tolist() == want["info"].tolist(), (what, got["info"][:8], want["info"][:8])
    assert np.array_equal(got["sums"], want["sums"]), (what, np.argwhere(got["sums"] != want["sums"])[:4])
    n = len(want["cell"]) if rows is None else rows
    assert np.array_equal(got["cell"][:n], want["cell"][:n]), (what, np.argwhere(got["cell"][:n] != want["cell"][:n])[:4])
    a, b = got["pose"], want["pose"]
    bad = a.view(np.uint64) != b.view(np.uint64)
    bad &= ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), (what, np.argwhere(bad)[:4], a[bad][:4], b[bad][:4])


DMAX3 = (1.0, 1.0, 0.5)


def _std(cuda, capacity=1 << 12):
    """the standard map at 1 m cells: (map case, its table at `capacity`, checked surf, Surface)"""
    mp = _map_case()
    want = _ref(("surface", 1, 5), lambda: L.surface(mp[5]))
    table = _table(cuda, mp, capacity)
    return mp, table, _surface(cuda, table, want), want


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach,min_cells", [(1, 5), (2, 5), (1, 9), (1, 10), (2, 30), (2, 31), (1, 27), (2, 125)])
def test_surface_rows_equal_the_restatement_per_key(cuda, reach, min_cells):
    mp = _map_case()
    want = _ref(("surface", reach, min_cells), lambda: L.surface(mp[5], reach, min_cells))
    if min_cells in (9, 30):      # min_cells at k and at k + 1: the cells that see exactly k keep their normal, then lose it
        k = min_cells
        at_k = want.used == k
        more = _ref(("surface", reach, k + 1), lambda: L.surface(mp[5], reach, k + 1))
        assert at_k.sum() > 0 and (want.normals[at_k] != 0).any(axis=1).all() and (more.normals[at_k] == 0).all()
    _surface(cuda, _table(cuda, mp, 1 << 12), want, reach, min_cells)


def test_one_map_at_two_capacities_and_from_two_streams_reads_the_same(cuda):
    from lpdnet_hip import ops
    mp = _map_case()
    want = _ref(("surface", 1, 5), lambda: L.surface(mp[5]))
    pts, off, start = _query_case(7, [700, 300])
    ref = _ref("two capacities", lambda: L.localize(want, pts, off, start, mp[3], 1.0, DMAX3))
    assert ref["info"][:, 1].tolist() == [2, 2] and ref["info"][:, 3].min() > 50
    outs = []
    for cap in (1 << 10, 1 << 13):      # 556 cells: a load of 0.54 and of 0.07 -- probe chains of up to nine slots, and hardly any
        assert len(want.keys) == 556
        table = _table(cuda, mp, cap)
        surf = _surface(cuda, table, want)
        outs.append(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3))
        _check(outs[-1], ref, cap)
    assert all(outs[0][k].tobytes() == outs[1][k].tobytes() for k in outs[0])
    # a table made by two inserts on two streams at once: the slots depend on timing, the answers do not
    table = ops.map_table(1 << 11, cuda)
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    torch.cuda.synchronize()
    for s, half in zip(streams, ((0, 2), (2, 4))):
        with torch.cuda.stream(s):
            _table(cuda, mp, None, scans=half, table=table)
    torch.cuda.synchronize()
    _check(_localize(cuda, table, _surface(cuda, table, want), pts, off, start, mp[3], 1.0, DMAX3), ref, "two streams")


def test_a_full_table_of_16_slots(cuda):
    """16 cells in 16 slots: every lookup of an absent key ends after 16 probes"""
    g = np.arange(4, dtype=f64)
    centres = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), axis=-1).reshape(-1, 3) + 0.5
    rng = np.random.default_rng(3)
    world = np.repeat(centres, 30, axis=0) + np.concatenate((rng.uniform(-0.45, 0.45, (480, 2)), rng.normal(0.0, 0.01, (480, 1))), axis=1)
    ident = C.pose12(np.eye(3), np.zeros(3))
    mp = (world.astype(f32), M.offsets_of([480]), ident[None], np.zeros(3), 1.0, None)
    cells = M.insert(*mp[:5])
    assert len(cells.keys) == 16
    want = L.surface(cells, 1, 4)
    table = _table(cuda, mp, 16)
    assert table[2].tolist() == [480, 0, 0, 16] and int((table[0] >= 0).sum()) == 16
    surf = _surface(cuda, table, want, 1, 4)
    q = np.concatenate((world + [0.0, 0.0, 0.03], rng.uniform(-3.0, 7.0, (400, 3)))).astype(f32)      # on the slab, and all around it
    off = M.offsets_of([len(q)])
    start = C.pose12(I.rot_xyz(0.0, 0.0, 0.01), [0.05, -0.05, 0.0])[None]
    ref = L.localize(want, q, off, start, np.zeros(3), 1.0, (1.0,), 6, 1.0)      # one pass: a single sheet does not fix a pose
    assert ref["info"][0, 3] > 400 and (ref["cell"] < 0).sum() > 100
    _check(_localize(cuda, table, surf, q, off, start, np.zeros(3), 1.0, (1.0,), 6, 1.0), ref, "full table")


def test_cells_at_the_index_border(cuda):
    """cell = 1/64 m: the last cell index 2^20 - 1 ends at 16384 m.  A floor, a wall IN the last column of cells and a second wall, each
    through the middle of its cells and apart from the others; rows beyond the border have no cell."""
    cell = 2.0 ** -6
    t = np.array([16383.0, 0.0, 0.0])
    u = (np.arange(96, dtype=f64) + 0.5) / 256.0      # four points a cell; world x = 16384 - u lies in the last 24 cells

    def sheet(a, b):
        A, B = np.meshgrid(a, b, indexing="ij")
        return A.ravel(), B.ravel()
    fx, fy = sheet(1.0 - u, u)
    ay, az = sheet(u, u[8:])
    bx, bz = sheet(1.0 - u[12:], u[8:])
    mid = 2.0 / 256.0
    local = np.concatenate((np.stack((fx, fy, np.full(fx.size, mid)), axis=1), np.stack((np.full(ay.size, 1.0 - mid), ay, az), axis=1),
                            np.stack((bx, np.full(bx.size, mid), bz), axis=1)))
    ident = C.pose12(np.eye(3), t)
    mp = (local.astype(f32), M.offsets_of([len(local)]), ident[None], np.zeros(3), cell, None)
    cells = M.insert(*mp[:5])
    q = M.unkey(cells.keys)
    assert q[:, 0].max() == M.QLIM - 1 and len(cells.keys) == 24 * 24 + 24 * 22 + 21 * 22 and np.all(cells.counts == 16)
    want = L.surface(cells, 2, 5)
    table = _table(cuda, mp, 1 << 11)
    _surface(cuda, table, want, 2, 5)
    want = L.surface(cells)
    surf = _surface(cuda, table, want)
    rng = np.random.default_rng(5)
    rows = np.concatenate((local + rng.normal(0.0, 0.001, local.shape), local + [0.2, 0.0, 0.0]))[rng.permutation(2 * len(local))[:5000]].astype(f32)
    off = M.offsets_of([len(rows)])
    start = C.pose12(I.rot_xyz(0.0, 0.0, 0.002), t + [0.003, -0.002, 0.001])[None]
    dmax = (cell, cell, cell / 2)
    ref = L.localize(want, rows, off, start, np.zeros(3), cell, dmax, 6, 1.0)
    assert ref["info"][0, 1] == 2 and ref["info"][0, 3] > 1000 and (ref["cell"] < 0).sum() > 1000
    edge = M.unkey(ref["cell"][ref["cell"] >= 0])[:, 0] == M.QLIM - 1
    assert edge.sum() > 20      # rows that correspond to cells of the last column
    _check(_localize(cuda, table, surf, rows, off, start, np.zeros(3), cell, dmax, 6, 1.0), ref, "border")


# ---- the pass: scan lengths, chunks, layouts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, M.CHUNK - 1, M.CHUNK, M.CHUNK + 1, 2 * M.CHUNK + 1])
def test_one_scan_of_n_rows(cuda, rows):
    mp, table, surf, want = _std(cuda)
    pts, off, start = _query_case(100 + rows, [rows])
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, 6)
    assert rows < 63 or ref["info"][0].tolist()[:3] == [1, 2, 0]
    _check(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3, 6), ref, rows)


def test_short_scans_empty_scans_ld_and_alignment(cuda):
    mp, table, surf, want = _std(cuda)
    lengths = [3] * 70 + [500, 0, 700, 0, 0, 40]      # a chunk that spans 70 scans: more than the 64 staged poses; an empty scan between two
    pts, off, start = _query_case(11, lengths)
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, 6)
    assert (ref["info"][:70, 2] == 2).all() and ref["info"][70, 1] == 2 and ref["info"][71].tolist() == [1, 0, 2, 0] and ref["sums"][:, :70, 0].sum() > 70
    for ld, mis in ((3, False), (3, True), (4, False), (4, True), (6, False)):
        _check(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3, 6, ld=ld, misaligned=mis), ref, (ld, mis))
    # more than 64 scans in every chunk
    lengths = np.random.default_rng(4).integers(0, 9, 700)
    pts, off, start = _query_case(12, lengths)
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, 6)
    _check(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3, 6), ref, "700 short scans")


def test_a_sub_range_of_scans_leaves_the_others_bit_for_bit(cuda):
    mp, table, surf, want = _std(cuda)
    pts, off, start = _query_case(13, [300, 900, 0, 1100, 200, 500])
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, scan0=1, scan1=4)
    got = _localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3, scans=(1, 4))
    _check(got, ref, "sub-range")
    for i in (0, 4, 5):
        assert got["pose"][i].tobytes() == start[i].tobytes() and got["info"][i].tolist() == [0, 0, 0, 0] and not got["sums"][:, i].any()
    assert (got["cell"][:300] == -1).all() and (got["cell"][off[4]:] == -1).all() and (got["cell"][off[1]:off[4]] >= 0).sum() > 500
    assert got["info"][1].tolist()[:3] == [1, 2, 0] and np.abs(got["pose"][1] - start[1]).max() > 1e-3


def test_a_broken_offsets_table_is_not_read(cuda):
    """48 scans of 64 rows: the scans 16 .. 31 are exactly the second chunk, and offsets[20] = offsets[21] + 5 descends inside it.  That
    chunk alone is refused -- its rows get no correspondence, its scans no step -- and every other scan comes out as on the intact
    table: 1349 and 1280 lie on the same side of every row of the other chunks, so the binary search answers there as before."""
    S, n, iters = 48, 64, 2
    mp, table, surf, want = _std(cuda)
    pts, off, start = _query_case(21, [n] * S)
    bad = off.copy()
    bad[20] = bad[21] + 5
    second = np.arange(M.CHUNK, 2 * M.CHUNK)
    # the chunk rule of the restatement: the second chunk is not read, every other row is, by the scan it belongs to
    g, scan, not_read = M.row_scans(bad, 0, S, S * n)
    assert not_read == M.CHUNK and np.array_equal(g, np.delete(np.arange(S * n), second)) and np.array_equal(scan, g // n)
    whole = _ref("broken: intact", lambda: L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, 6))
    assert (whole["info"][:, 1] == iters).all() and whole["info"][:, 3].min() > 6
    got = _localize(cuda, table, surf, pts, bad, start, mp[3], 1.0, DMAX3, 6)
    others = np.r_[0:16, 32:S]
    for k in ("pose", "info"):
        assert got[k][others].tobytes() == whole[k][others].tobytes(), k
    assert np.array_equal(got["sums"][:, others], whole["sums"][:, others])
    assert got["info"][20, 0] == -1
    for i in range(16, 32):
        assert i == 20 or got["info"][i].tolist() == [1, 0, iters, 0], (i, got["info"][i])
        assert not got["sums"][:, i].any() and got["pose"][i].tobytes() == start[i].tobytes(), i
    assert (got["cell"][second] == -1).all()
    assert np.array_equal(np.delete(got["cell"], second), np.delete(whole["cell"], second))
    _check(got, _ref("broken", lambda: L.localize(want, pts, bad, start, mp[3], 1.0, DMAX3, 6)), "the restatement on the broken table")
    for lo, hi in ((0, S * n + 1), (-1, S * n), (200, 100)):      # the call reads nothing
        worse = off.copy()
        worse[0], worse[-1] = lo, hi
        got = _localize(cuda, table, surf, pts, worse, start, mp[3], 1.0, DMAX3, 6)
        assert got["pose"].tobytes() == start.tobytes() and not got["sums"].any() and (got["cell"] == -1).all(), (lo, hi)


def test_nan_rows_a_nan_pose_and_a_scan_of_more_than_2_to_20_rows(cuda):
    mp, table, surf, want = _std(cuda)
    pts, off, start = _query_case(14, [400, 600, 500])
    pts = pts.copy()
    pts[5::40, 0] = np.nan
    pts[7::40, 1] = np.inf
    pts[9::40, 2] = f32(3e7)
    start = start.copy()
    start[1, 6] = np.nan
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3)
    assert ref["info"][:, 0].tolist() == [1, -1, 1] and not ref["sums"][:, 1].any() and (ref["cell"][400:1000] == -1).all()
    got = _localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3)
    _check(got, ref, "nan")
    assert got["pose"][1].tobytes() == start[1].tobytes()
    # a forged offsets table: the middle scan claims 2^20 + 1 rows that nobody wrote -- invalid, never read
    big = L.MAX_SCAN_ROWS + 1
    a, _, b = _query_case(15, [400, 500])
    forged = np.array([0, 400, 400 + big, 900 + big], dtype=np.int32)
    points = torch.empty((900 + big, 3), dtype=torch.float32, device=cuda)
    points[:400].copy_(torch.from_numpy(a[:400]))
    points[400 + big:].copy_(torch.from_numpy(a[400:]))
    start3 = np.stack((b[0], b[0], b[1]))
    host = np.zeros((900 + big, 3), dtype=f32)
    host[:400], host[400 + big:] = a[:400], a[400:]
    ref = L.localize(want, host, forged, start3, mp[3], 1.0, DMAX3)
    assert ref["info"][:, 0].tolist() == [1, -1, 1] and ref["info"][0, 1] == 2 and ref["info"][2, 1] == 2
    got = _localize(cuda, table, surf, None, forged, start3, mp[3], 1.0, DMAX3, points=points)
    _check(got, ref, "forged")
    assert (got["cell"][400:400 + big] == -1).all() and got["pose"][1].tobytes() == start3[1].tobytes()


def test_a_refused_step_and_no_step_at_all(cuda):
    mp, table, surf, want = _std(cuda)
    pts, off, start = _query_case(16, [800, 30])
    ref = L.localize(want, pts, off, start, mp[3], 1.0, DMAX3, 200)      # the second scan has 30 rows: fewer than min_inliers
    assert ref["info"][0].tolist()[:3] == [1, 2, 0] and ref["info"][1].tolist()[:3] == [1, 0, 2] and 6 < ref["info"][1, 3] <= 30
    got = _localize(cuda, table, surf, pts, off, start, mp[3], 1.0, DMAX3, 200)
    _check(got, ref, "refused")
    assert got["pose"][1].tobytes() == start[1].tobytes()
    ref = L.localize(want, pts, off, start, mp[3], 1.0, (1.0,))      # iters = 0: one pass, no step
    got = _localize(cuda, table, surf, pts, off, start, mp[3], 1.0, (1.0,))
    _check(got, ref, "iters = 0")
    assert got["sums"].shape == (1, 2, 32) and got["pose"].tobytes() == start.tobytes() and got["info"][:, 1:3].tolist() == [[0, 0], [0, 0]]
    # flatness and distance trim for real: a tight max_flat and a small dmax
    ref = L.localize(want, pts, off, start, mp[3], 1.0, (0.3, 0.2, 0.1), 6, 0.02)
    _check(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, (0.3, 0.2, 0.1), 6, 0.02), ref, "trimmed")


def test_eight_steps_at_a_utm_origin_repeat_bit_for_bit_on_two_streams(cuda):
    utm = (5.7e6, 6.2e5, 120.0)
    mp = _map_case(origin=utm)
    want = _ref(("surface utm", 1, 5), lambda: L.surface(mp[5]))
    table = _table(cuda, mp, 1 << 12)
    surf = _surface(cuda, table, want)
    pts, off, start = _query_case(17, [1500, 900, 2100], origin=utm, rot=0.04, shift=0.4)
    dmax = L.schedule(1.0)
    ref = _ref("utm chain", lambda: L.localize(want, pts, off, start, mp[3], 1.0, dmax))
    assert ref["info"][:, 1].tolist() == [8, 8, 8]
    truth_moved = np.abs(ref["pose"] - start)[:, M.TRA].max()
    assert 0.05 < truth_moved < 1.0
    outs = [_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, dmax) for _ in range(3)]
    for o in outs:
        _check(o, ref, "utm")
    assert all(outs[0][k].tobytes() == o[k].tobytes() for o in outs[1:] for k in o)
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    torch.cuda.synchronize()
    res = []
    for s in streams:
        with torch.cuda.stream(s):
            res.append(_localize(cuda, table, surf, pts, off, start, mp[3], 1.0, dmax))
    torch.cuda.synchronize()
    for o in res:
        _check(o, ref, "two streams")


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------------
def test_voxel_map_surface_is_cached_and_dropped_by_an_insert_that_grows_the_table(cuda):
    from lpdnet_hip import mapping
    mp = _map_case()
    pts, off, poses, origin, cell, cells = mp
    tp, tposes = torch.from_numpy(pts).to(cuda), torch.from_numpy(poses).to(cuda)
    vm = mapping.VoxelMap(cell, origin=origin, capacity=1 << 11, device=cuda)      # 556 cells: no growth yet
    vm.insert(tp, [4000] * 4, tposes)
    s1 = vm.surface()
    assert vm.capacity == 1 << 11 and vm.surface() is s1 and vm.surface(2, 5) is not s1 and tuple(s1.shape) == (vm.capacity, 8)

    def same(sc, w):
        assert np.array_equal(sc.keys.cpu().numpy(), w.keys) and sc.normals.cpu().numpy().tobytes() == w.normals.tobytes()
        assert sc.flatness.cpu().numpy().tobytes() == w.flatness.tobytes() and np.array_equal(sc.used.cpu().numpy(), w.used)
        assert sc.points.cpu().numpy().tobytes() == w.points.tobytes() and len(sc) == len(w.keys)
    same(vm.surface_cells(), _ref(("surface", 1, 5), lambda: L.surface(cells)))
    # the same scans 100 m further on: twice the cells, more than half of the slots -- the table doubles, the cached rows are dropped
    moved = poses.copy()
    moved[:, 3] += 100.0
    vm.insert(tp, [4000] * 4, torch.from_numpy(moved).to(cuda))
    both = M.insert(pts, off, moved, origin, cell, into=cells)
    assert vm.capacity == 1 << 12 and vm._surface is None and vm.occupied == len(both.keys) > 1 << 10
    s2 = vm.surface()
    assert s2 is not s1 and tuple(s2.shape) == (vm.capacity, 8)
    same(vm.surface_cells(), L.surface(both))


def test_localize_scans_end_to_end_and_back_into_the_map(cuda):
    from lpdnet_hip import mapping
    seed, cell = 1, 1.0
    case, cells, surf = C.street_map(seed, cell)
    vm = mapping.build_map(torch.from_numpy(case["points_map"]).to(cuda), case["lengths_map"], torch.from_numpy(case["poses_map"]).to(cuda), cell=cell)
    assert vm.occupied == len(cells.keys) and vm.origin.cpu().numpy().tobytes() == case["origin"].tobytes()
    tp = torch.from_numpy(case["points"]).to(cuda)
    loc = mapping.localize_scans(vm, tp, case["lengths"], torch.from_numpy(case["start"]).to(cuda), want_cells=True)
    ref = _ref("street", lambda: L.localize(surf, case["points"], M.offsets_of(case["lengths"]), case["start"], case["origin"], cell, L.schedule(cell)))
    got = dict(pose=loc.poses.cpu().numpy(), info=np.stack((np.where(loc.valid.cpu().numpy(), 1, -1), loc.steps.cpu().numpy(), loc.refused.cpu().numpy(),
                                                            ref["info"][:, 3]), axis=1), sums=loc.sums.cpu().numpy(), cell=loc.cells.cpu().numpy())
    _check(got, ref, "localize_scans")
    assert loc.poses.dtype == torch.float64 and tuple(loc.poses.shape) == (3, 12) and loc.poses.device == tp.device and len(loc) == 3
    share = loc.inliers.cpu().numpy()
    assert np.array_equal(share, ref["info"][:, 3] / case["lengths"]) and share.min() > 0.3
    assert np.allclose(loc.rms.cpu().numpy(), [I.rms(s) for s in ref["sums"][-1]], rtol=1e-12, atol=0)
    e0, e1 = C.errors(case["start"], case["truth"]), C.errors(got["pose"], case["truth"])
    assert all(b[0] < a[0] and b[1] < a[1] for a, b in zip(e0, e1))
    assert max(e[0] for e in e1) <= C.FINAL_ROT_DEG[cell] and max(e[1] for e in e1) <= C.FINAL_TRANS_M[cell]
    far = mapping.localize_scans(vm, tp, case["lengths"], torch.from_numpy(case["far"]).to(cuda))
    assert far.inliers.max().item() < share.min() and far.cells is None
    # only the middle scan, with another search
    one = mapping.localize_scans(vm, tp, case["lengths"], case["start"], search=mapping.LocalizeSearch(iters=2, dmax=1.0), scans=(1, 2))
    assert one.valid.tolist() == [False, True, False] and one.steps.tolist() == [0, 2, 0]
    assert one.poses[0].cpu().numpy().tobytes() == case["start"][0].tobytes() and one.poses[2].cpu().numpy().tobytes() == case["start"][2].tobytes()
    # lap two into the same map: the localised poses go straight back into insert
    before = vm.occupied
    vm.insert(tp, case["lengths"], loc.poses)
    both = M.insert(case["points"], M.offsets_of(case["lengths"]), ref["pose"], case["origin"], cell, into=cells)
    assert vm.occupied == len(both.keys) > before and vm._surface is None
    assert np.array_equal(vm.cells().keys.cpu().numpy(), both.keys) and np.array_equal(vm.cells().sums.cpu().numpy(), both.sums)
