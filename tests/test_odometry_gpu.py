"""lpd_odom_predict / lpd_odom_accept / lpd_map_crop / lpd_map_touch / lpd_map_surface_touched, their ops wrappers and
lpdnet_hip/odometry.py on the GPU against tests/odom_ref.py.

Everything is exact: the bits of the poses, the integers of the counters, per key after a sort by key the sums of a cropped table, and
the bits of surf after insert + touch + refresh against a full lpd_map_surface of the same table.  The end-to-end case also stays
within the ratio that tests/test_odometry_cpu.py measured on the restatement (tests/odom_cases.py)."""
import numpy as np
import pytest
import torch

import loc_ref as L
import map_ref as M
import odom_cases as C
import odom_ref as O

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
_REFS = {}


def _ref(name, make):
    """a restatement's result, computed once and shared (read-only)"""
    if name not in _REFS:
        _REFS[name] = make()
    return _REFS[name]


def _t(cuda, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=f64), np.ascontiguousarray(want, dtype=f64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


# ---- predict and accept: the CPU file's cases on the device -------------------------------------------------------------------------------------
def test_predict_equals_the_restatement_bit_for_bit(cuda):
    from lpdnet_hip import ops
    for name, P, t, motion in C.predict_cases():
        pose, pred = _t(cuda, P, f64), torch.full((4, 12), 7.0, dtype=torch.float64, device=cuda)
        before = pose.clone()
        ops.odom_predict(pose, pred, t, None if motion is None else _t(cuda, motion, f64))
        want = O.predict(P, t, motion)
        _same(pred[t].cpu().numpy(), want, name)
        _same(pose[t].cpu().numpy(), want, name + ": pose[t] is the start of the localisation")
        other = [i for i in range(4) if i != t]
        _same(pose[other].cpu().numpy(), before[other].cpu().numpy(), name + ": the other poses are not touched")
        assert (pred[other] == 7.0).all(), name


def test_accept_equals_the_restatement_bit_for_bit(cuda):
    from lpdnet_hip import ops
    S = 6
    for name, pred_t, pose_t, info_t, n, t, sq, mj, want in C.accept_cases():
        n = int(n)
        pred, pose = np.full((S, 12), 3.0), np.full((S, 12), 4.0)
        info = np.full((S, 4), 9, dtype=np.int32)
        pred[t], pose[t], info[t] = pred_t, pose_t, info_t
        lengths = np.full(S, 5, dtype=i64)
        lengths[t] = n
        off = np.concatenate(([0], np.cumsum(lengths)))
        d_pred, d_pose, d_ins = _t(cuda, pred, f64), _t(cuda, pose, f64), torch.full((S, 12), 5.0, dtype=torch.float64, device=cuda)
        state = torch.full((S,), -7, dtype=torch.int32, device=cuda)
        ops.odom_accept(d_pred, d_pose, _t(cuda, info, np.int32), _t(cuda, off, np.int32), t, sq, mj, d_ins, state)
        st, p, ins = O.accept(pred_t, pose_t, info_t, n, t, sq, mj)
        assert st == want
        got_state = state.cpu().numpy()
        assert got_state[t] == st and (np.delete(got_state, t) == -7).all(), (name, got_state)
        _same(d_pose[t].cpu().numpy(), p, name)
        _same(d_ins[t].cpu().numpy(), ins, name)
        other = [i for i in range(S) if i != t]
        assert (d_pose[other] == 4.0).all() and (d_ins[other] == 5.0).all(), name


# ---- the crop -------------------------------------------------------------------------------------------------------------------------------------
def _cell_rows(seed, n_cells, span, per_cell=3):
    """rows that fall into n_cells distinct 1 m cells of [-span, span)^3, the cell (0, -1, 0) of CENTRE among them, a few each ->
    (points [n, 3] fp32, shuffled)"""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*(np.arange(-span, span),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = grid[(grid != np.array([0, -1, 0])).any(axis=1)]
    q = np.concatenate((grid[rng.choice(len(grid), n_cells - 1, replace=False)], [[0, -1, 0]]))
    pts = np.repeat(q, per_cell, axis=0) + rng.uniform(0.1, 0.9, (n_cells * per_cell, 3))
    return pts[rng.permutation(len(pts))].astype(f32)


def _insert(cuda, pts, capacity, poses=None, lengths=None, table=None, scans=(0, None), origin=(0.0, 0.0, 0.0), cell=1.0):
    """ops.map_insert of rows under the identity (or `poses`) -> (keys, acc, info)"""
    from lpdnet_hip import ops
    lengths = [len(pts)] if lengths is None else lengths
    poses = np.tile(O.IDENTITY, (len(lengths), 1)) if poses is None else poses
    table = ops.map_table(capacity, cuda) if table is None else table
    ops.map_insert(_t(cuda, pts, f32), _t(cuda, M.offsets_of(lengths), np.int32), _t(cuda, poses, f64), _t(cuda, origin, f64),
                   ops.map_inv_cell(cell), *table, scans[0], scans[1])
    return table


def _mapping(keys, acc):
    """a table -> (keys ascending, sums [M, 3], counts [M])"""
    keys, acc = keys.cpu().numpy(), acc.cpu().numpy()
    live = keys >= 0
    order = np.argsort(keys[live])
    return keys[live][order], acc[live][order][:, :3], acc[live][order][:, 3]


def _crop(cuda, table, centre, keep_cells, capacity, origin=(0.0, 0.0, 0.0), cell=1.0):
    from lpdnet_hip import ops
    keys, acc, info, info5 = ops.map_crop_table(capacity, cuda)
    ops.map_crop(table[0], table[1], _t(cuda, centre, f64), _t(cuda, origin, f64), ops.map_inv_cell(cell), keep_cells, keys, acc, info5)
    return keys, acc, info, info5


def _check_crop(cuda, pts, cap_in, cap_out, centre, keep_cells):
    table = _insert(cuda, pts, cap_in)
    cells = M.insert(pts, M.offsets_of([len(pts)]), O.IDENTITY[None, :], np.zeros(3), 1.0)
    assert int(table[2][2]) == 0 and np.array_equal(_mapping(table[0], table[1])[0], cells.keys)
    want, left = O.crop(cells, centre, np.zeros(3), 1.0, keep_cells)
    keys, acc, info, info5 = _crop(cuda, table, centre, keep_cells, cap_out)
    k, s, m = _mapping(keys, acc)
    assert np.array_equal(k, want.keys) and np.array_equal(s, want.sums) and np.array_equal(m, want.counts), (cap_in, cap_out, keep_cells)
    assert info5.tolist() == [int(want.counts.sum()), 0, 0, len(want.keys), left], (info5.tolist(), left)
    assert info.data_ptr() == info5.data_ptr() and info.tolist() == info5.tolist()[:4]
    return want, left


CENTRE = np.concatenate((np.eye(3), [[0.5], [-0.5], [0.5]]), axis=1).reshape(12)      # the cell (0, -1, 0)


@pytest.mark.parametrize("cap_in,cap_out,n_cells,span,keep", [(16, 16, 12, 2, 1), (64, 16, 60, 2, 0), (64, 64, 60, 2, 1), (64, 4096, 60, 2, 9),
                                                              (4096, 16, 400, 6, 1), (4096, 64, 900, 6, 1), (4096, 4096, 900, 6, 3),
                                                              (4096, 4096, 900, 6, 0), (16, 4096, 16, 2, 5)])
def test_crop_keeps_the_cells_around_the_centre_at_every_capacity(cuda, cap_in, cap_out, n_cells, span, keep):
    """64 slots holding 60 cells is a table near its probe limit: its chains wrap around the end"""
    want, left = _check_crop(cuda, _cell_rows(cap_in + n_cells, n_cells, span), cap_in, cap_out, CENTRE, keep)
    assert len(want.keys) > 0 and (left == 0) == (keep >= 5)      # keep 5 and 9 are larger than the map
    if keep == 0:
        assert want.keys.tolist() == M.key(np.array([[0, -1, 0]])).tolist()


def test_crop_does_not_depend_on_slot_placement(cuda):
    pts = _cell_rows(5, 60, 2)
    a = _insert(cuda, pts, 64)
    b = _insert(cuda, pts[::-1].copy(), 64)
    ka, kb = a[0].cpu().numpy(), b[0].cpu().numpy()
    assert np.array_equal(np.sort(ka), np.sort(kb))
    outs = [_mapping(*_crop(cuda, t, CENTRE, 1, 64)[:2]) for t in (a, b)]
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    assert 0 < len(outs[0][0]) < 60


def test_crop_with_a_centre_that_is_not_finite_or_has_no_cell_keeps_everything(cuda):
    pts = _cell_rows(6, 200, 4)
    nan = CENTRE.copy()
    nan[5] = np.nan
    far = CENTRE.copy()
    far[3] = 4.0e6
    for centre in (nan, far):
        want, left = _check_crop(cuda, pts, 1024, 512, centre, 0)
        assert left == 0 and len(want.keys) == 200


def test_crop_into_a_table_that_is_too_small_counts_the_lost_rows(cuda):
    pts = _cell_rows(7, 60, 2)
    table = _insert(cuda, pts, 64)
    keys, acc, info, info5 = _crop(cuda, table, CENTRE, 9, 16)
    c = info5.tolist()
    assert c[0] + c[2] == len(pts) and c[2] > 0 and c[3] == 16 and c[4] == 0


def test_rehash_and_crop_are_one_copy(cuda):
    """600 cells in 2^10 slots into 2^11 slots by lpd_map_rehash, by a crop around a centre that is not finite and by a crop that keeps
    more cells than the map is wide: the same cells bit for bit and the same first four counters.  Into 16 slots WHICH keys are lost
    depends on timing; that the counters add up does not."""
    from lpdnet_hip import mapping, ops
    pts = _cell_rows(8, 600, 6)
    table = _insert(cuda, pts, 1 << 10)
    assert table[2].tolist() == [len(pts), 0, 0, 600]
    nan = CENTRE.copy()
    nan[5] = np.nan

    def rehash(capacity):
        keys, acc, info = ops.map_table(capacity, cuda)
        ops.map_rehash(table[0], table[1], keys, acc, info)
        return keys, acc, info, None

    def three_ways(capacity):
        return rehash(capacity), _crop(cuda, table, nan, 0, capacity), _crop(cuda, table, CENTRE, 64, capacity)
    outs = []
    for keys, acc, info, info5 in three_ways(1 << 11):
        c = mapping.extract_cells(keys, acc, None, 1.0)
        outs.append([x.cpu().numpy().tobytes() for x in (c.keys, c.counts, c.sums, c.points)] + [info.tolist()])
        assert info.tolist() == [len(pts), 0, 0, 600]
        assert info5 is None or int(info5[4]) == 0
    assert outs[0] == outs[1] == outs[2]
    want = mapping.extract_cells(table[0], table[1], None, 1.0)
    assert outs[0][0] == want.keys.cpu().numpy().tobytes() and outs[0][2] == want.sums.cpu().numpy().tobytes()
    for keys, acc, info, info5 in three_ways(16):
        c, occupied = info.tolist(), int((keys >= 0).sum())
        assert c[0] + c[2] == len(pts) and c[1] == 0 and c[3] == occupied <= 16, c
        assert int(acc[:, 3].sum()) == c[0] and (info5 is None or int(info5[4]) == 0)


# ---- touch + refresh against the full surface ----------------------------------------------------------------------------------------------------------
def _scan_rows(rng, n, box, z=2.0):
    """n rows in [-box, box]^2 x [0, z): most on a floor and a wall, so that cells get normals"""
    kind = rng.integers(0, 3, n)
    a, b, h = rng.uniform(-box, box, n), rng.uniform(-box, box, n), rng.uniform(0.0, z, n)
    e = rng.normal(0.0, 0.02, n)
    floor = np.stack((a, b, 0.4 + e), axis=1)
    wall = np.stack((0.3 * box + e, b, h), axis=1)
    free = np.stack((a, b, h), axis=1)
    return np.where((kind == 0)[:, None], floor, np.where((kind == 1)[:, None], wall, free)).astype(f32)


class _Touched:
    """one table with its surf and dirty, fed scan after scan: insert, touch, refresh, and the comparison with the full surface"""

    def __init__(self, cuda, capacity, reach, min_cells=5):
        from lpdnet_hip import ops
        self.cuda, self.reach, self.min_cells = cuda, reach, min_cells
        self.table = ops.map_table(capacity, cuda)
        self.surf = torch.zeros((capacity, ops.LOC_SURF), dtype=torch.float32, device=cuda)
        self.dirty = torch.zeros((capacity,), dtype=torch.uint8, device=cuda)

    def add(self, pts, lengths, poses, scans, offsets=None, ld=3):
        from lpdnet_hip import ops
        host = np.full((max(len(pts), 1), ld), 9.5, dtype=f32)
        host[:len(pts), :3] = pts
        args = (_t(self.cuda, host, f32), _t(self.cuda, M.offsets_of(lengths) if offsets is None else offsets, np.int32), _t(self.cuda, poses, f64),
                _t(self.cuda, np.zeros(3), f64), ops.map_inv_cell(1.0), self.table[0])
        ops.map_insert(*args[:5], *self.table, scans[0], scans[1])
        ops.map_touch(*args, self.dirty, self.reach, scans[0], scans[1])
        marked = self.dirty.cpu().numpy().astype(bool)
        info = ops.map_surface_touched(self.table[0], self.table[1], self.surf, self.dirty, self.reach, self.min_cells)
        assert int(info.sum()) == int(marked.sum())
        self.check()
        return marked

    def check(self):
        from lpdnet_hip import ops
        assert int(self.table[2][2]) == 0
        full, _ = ops.map_surface(self.table[0], self.table[1], self.reach, self.min_cells)
        a, b = self.surf.cpu().numpy().view(np.uint32), full.cpu().numpy().view(np.uint32)
        assert np.array_equal(a, b), np.argwhere(a != b)[:4]
        assert not self.dirty.any()


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 3000])
def test_touch_and_refresh_equal_the_full_surface(cuda, rows, reach):
    rng = np.random.default_rng(100 * reach + rows)
    lengths = [700, rows, 300]
    pts = np.concatenate([_scan_rows(rng, n, 12.0) for n in lengths])
    poses = np.tile(O.IDENTITY, (3, 1))
    poses[1, M.TRA] = (1.5, -0.5, 0.0)
    poses[2, M.TRA] = (-2.0, 3.0, 0.25)
    t = _Touched(cuda, 1 << 14, reach)
    for i in range(3):      # three successive inserts
        marked = t.add(pts, lengths, poses, (i, i + 1))
        if i == 1:      # the marked slots are the restatement's touched set, and not the whole table
            keys = t.table[0].cpu().numpy()
            cells = M.insert(pts, M.offsets_of(lengths), poses, np.zeros(3), 1.0, 0, 2)
            want = O.touched(cells.keys, O.row_keys(pts, M.offsets_of(lengths), poses, np.zeros(3), 1.0, 1, 2), reach)
            assert np.array_equal(np.sort(keys[marked]), cells.keys[want])
            assert rows > 1 or marked.sum() < 0.2 * len(cells.keys)


@pytest.mark.parametrize("reach", [1, 2])
def test_touch_on_a_small_table_at_high_load_with_wrap_around(cuda, reach):
    rng = np.random.default_rng(30 + reach)
    lengths = [150, 120]
    pts = rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 3.9], (270, 3)).astype(f32)      # 4 x 4 x 4 = 64 cells at the most: no row can be lost
    t = _Touched(cuda, 64, reach)
    t.add(pts, lengths, np.tile(O.IDENTITY, (2, 1)), (0, 1))
    t.add(pts, lengths, np.tile(O.IDENTITY, (2, 1)), (1, 2))
    assert int(t.table[2][3]) > 55      # more than 55 of the 64 slots hold a cell: every chain is long and wraps around


def test_touch_of_scans_that_insert_nothing_marks_nothing(cuda):
    from lpdnet_hip import ops
    rng = np.random.default_rng(40)
    lengths = [600, 0, 500, 400]
    pts = np.concatenate([_scan_rows(rng, n, 8.0) for n in lengths])
    poses = np.tile(O.IDENTITY, (4, 1))
    poses[2, 6] = np.nan      # scan 2: a NaN pose
    t = _Touched(cuda, 1 << 12, 1)
    assert t.add(pts, lengths, poses, (0, 1)).sum() > 100
    before = [x.clone() for x in t.table[:2]]
    assert t.add(pts, lengths, poses, (1, 2)).sum() == 0      # an empty scan
    assert t.add(pts, lengths, poses, (2, 3)).sum() == 0      # the NaN pose: the insert drops its rows, the touch marks nothing
    assert t.table[2].tolist()[:2] == [600, 500]
    assert all(torch.equal(a, b) for a, b in zip(before, t.table[:2]))
    assert t.add(pts, lengths, poses, (3, 4), ld=4).sum() > 100      # ... and the table goes on as before, rows of four floats


def test_touch_walks_a_broken_offsets_table_as_the_insert_does(cuda):
    rng = np.random.default_rng(41)
    lengths = np.full(30, 100)
    pts = _scan_rows(rng, 3000, 10.0)
    poses = np.tile(O.IDENTITY, (30, 1))
    bad = M.offsets_of(lengths).copy()
    bad[12] = bad[13] + 5      # descends inside the second chunk: that chunk is not read
    cells = M.insert(pts, bad, poses, np.zeros(3), 1.0)
    assert 0 < cells.info[1] < 3000
    t = _Touched(cuda, 1 << 12, 1)
    marked = t.add(pts, lengths, poses, (0, 30), offsets=bad)
    assert t.table[2].tolist() == cells.info.tolist()
    want = O.touched(cells.keys, O.row_keys(pts, bad, poses, np.zeros(3), 1.0), 1)
    assert np.array_equal(np.sort(t.table[0].cpu().numpy()[marked]), cells.keys[want])
    for lo, hi in ((0, 3001), (-1, 3000), (200, 100)):      # the call reads nothing
        worse = M.offsets_of(lengths).copy()
        worse[0], worse[-1] = lo, hi
        assert t.add(pts, lengths, poses, (0, 30), offsets=worse).sum() == 0
    assert t.table[2].tolist() == cells.info.tolist()


def test_touch_after_a_crop_and_on_two_streams(cuda):
    from lpdnet_hip import ops
    rng = np.random.default_rng(50)
    lengths = [900, 800]
    pts = np.concatenate([_scan_rows(rng, n, 12.0) for n in lengths])
    poses = np.tile(O.IDENTITY, (2, 1))
    poses[1, M.TRA] = (2.5, 1.0, 0.0)
    t = _Touched(cuda, 1 << 12, 1)
    t.add(pts, lengths, poses, (0, 1))
    keys, acc, info, info5 = _crop(cuda, t.table, poses[1], 5, 1 << 12)
    assert int(info5[4]) > 0 and int(info5[3]) > 0
    t.table = (keys, acc, info)
    t.surf = ops.map_surface(keys, acc, 1, 5)[0]      # a new table: the full surface once
    t.add(pts, lengths, poses, (1, 2))
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    twins = []
    torch.cuda.synchronize(cuda)
    for s in streams:
        with torch.cuda.stream(s):
            u = _Touched(cuda, 1 << 12, 1)
            args = (_t(cuda, pts, f32), _t(cuda, M.offsets_of(lengths), np.int32), _t(cuda, poses, f64), _t(cuda, np.zeros(3), f64), ops.map_inv_cell(1.0))
            for i in range(2):
                ops.map_insert(*args, *u.table, i, i + 1)
                ops.map_touch(*args, u.table[0], u.dirty, 1, i, i + 1)
                ops.map_surface_touched(u.table[0], u.table[1], u.surf, u.dirty, 1, 5)
            twins.append(u)
    torch.cuda.synchronize(cuda)
    for u in twins:
        u.check()
    a, b = (_mapping(u.table[0], u.table[1]) for u in twins)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------
KEEP_M, REFRESH, LOST = 20.0, 2, 3


def _chain_drive():
    return _ref("drive", lambda: C.street_drive(1, S=6, rows=2000))


def _chain_ref(lost=False):
    def make():
        d = _chain_drive()
        pts, lengths = C.with_lost_scan(d, LOST) if lost else (d["points"], d["lengths"])
        return pts, lengths, O.estimate(pts, lengths, d["truth"][0], 1.0, keep_m=KEEP_M, refresh=REFRESH)
    return _ref(("chain", lost), make)


def _estimate(cuda, pts, lengths, **kw):
    from lpdnet_hip import odometry
    search = odometry.OdometrySearch(**dict(dict(cell=1.0, keep=KEEP_M, refresh=REFRESH, capacity=1 << 14), **kw))
    return odometry.estimate_poses(torch.from_numpy(pts).to(cuda), lengths, _chain_drive()["truth"][0], search)


def _check_chain(odo, want, what):
    _same(odo.poses.cpu().numpy(), want["poses"], what)
    assert odo.valid.cpu().numpy().tolist() == want["valid"].tolist(), what
    assert odo.steps.cpu().numpy().tolist() == want["info"][:, 1].tolist() and odo.refused.cpu().numpy().tolist() == want["info"][:, 2].tolist(), what
    _same(odo.inliers.cpu().numpy(), want["inliers"], what)
    k, s, m = _mapping(odo.keys, odo.acc)
    cells = want["cells"]
    assert np.array_equal(k, cells.keys) and np.array_equal(s, cells.sums) and np.array_equal(m, cells.counts), what
    assert odo.lost == int((~want["valid"]).sum()) and odo.left_behind == sum(want["left"]), what
    mc = odo.cells()
    assert mc.points.cpu().numpy().tobytes() == cells.points.tobytes(), what


@pytest.mark.parametrize("surface", ["touched", "full"])
def test_estimate_poses_equals_the_restatement_bit_for_bit(cuda, surface):
    pts, lengths, want = _chain_ref()
    assert want["valid"].all() and len(want["left"]) == 2 and min(want["left"]) > 0      # the crops really left cells behind
    assert want["info"][1:, 1].tolist() == [8] * 5
    odo = _estimate(cuda, pts, lengths, surface=surface)
    _check_chain(odo, want, surface)
    assert odo.capacity == 1 << 14 and len(odo) == 6 and (odo.rms.cpu().numpy()[1:] > 0).all()
    e = C.errors(odo.poses.cpu().numpy(), _chain_drive()["truth"])
    assert max(x[1] for x in e) < 0.1, e


def test_a_capacity_that_is_too_small_ends_in_the_same_bits_after_doubling(cuda):
    pts, lengths, want = _chain_ref()
    odo = _estimate(cuda, pts, lengths, capacity=256)
    assert odo.capacity > 256 and odo.capacity >= len(want["cells"].keys)
    _check_chain(odo, want, "doubled")


def test_a_lost_scan_on_the_device(cuda):
    pts, lengths, want = _chain_ref(lost=True)
    assert want["valid"].tolist() == [True, True, True, False, True, True]
    odo = _estimate(cuda, pts, lengths)
    _check_chain(odo, want, "lost")
    _same(odo.poses[LOST].cpu().numpy(), want["pred"][LOST], "the lost scan keeps its prediction")


def test_estimated_poses_go_into_the_map_and_the_submaps_without_a_copy_back(cuda):
    from lpdnet_hip import drive, mapping, odometry
    d = _ref("quality drive", lambda: C.street_drive(2))      # the seed with the worst ratio on the restatement
    pts = torch.from_numpy(d["points"]).to(cuda)
    search = odometry.OdometrySearch(cell=1.0, keep=C.KEEP_M, refresh=C.REFRESH, min_share=C.MIN_SHARE)
    odo = odometry.estimate_poses(pts, d["lengths"], d["truth"][0], search)
    assert odo.poses.is_cuda and odo.lost == 0
    e = C.errors(odo.poses.cpu().numpy(), d["truth"])
    assert max(x[0] for x in e) <= C.WORST_ROT_DEG[1.0] and max(x[1] for x in e) <= C.WORST_TRANS_M[1.0]
    origin = d["truth"][0, M.TRA]
    est = mapping.VoxelMap(1.0, origin=origin, device=cuda).insert(pts, d["lengths"], odo.poses)
    true = mapping.VoxelMap(1.0, origin=origin, device=cuda).insert(pts, d["lengths"], d["truth"])
    ratio = est.occupied / true.occupied
    print(f"MEASURE odometry: occupied cells at the estimated over the true poses {est.occupied} / {true.occupied} = {ratio:.4f}")
    assert ratio <= C.OCCUPIED_BOUND
    sub, positions = drive.submaps_from_drive(pts, d["lengths"], odo.poses, length=6.0, stride=3.0, num_points=256)
    assert positions.is_cuda and positions.shape[0] >= 2 and torch.isfinite(positions).all()      # 11 m of drive: two windows at the least


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments(cuda):
    from lpdnet_hip import odometry, ops
    P = torch.zeros((3, 12), dtype=torch.float64, device=cuda)
    info, off, state = torch.zeros((3, 4), dtype=torch.int32, device=cuda), torch.zeros(4, dtype=torch.int32, device=cuda), torch.zeros(3, dtype=torch.int32, device=cuda)
    for bad in (lambda: ops.odom_predict(P, P, 1), lambda: ops.odom_predict(P, P.clone(), 3), lambda: ops.odom_predict(P, P.clone(), -1),
                lambda: ops.odom_predict(P, P.clone()[:2], 1), lambda: ops.odom_predict(P, P.clone(), 1, torch.zeros(11, dtype=torch.float64, device=cuda)),
                lambda: ops.odom_accept(P, P.clone(), info, off, 3, 100, 5.0, P.clone(), state),
                lambda: ops.odom_accept(P, P.clone(), info, off, 1, 1025, 5.0, P.clone(), state),
                lambda: ops.odom_accept(P, P.clone(), info, off, 1, 100, -1.0, P.clone(), state),
                lambda: ops.odom_accept(P, P.clone(), info, off, 1, 100, float("nan"), P.clone(), state),
                lambda: ops.odom_accept(P, P, info, off, 1, 100, 5.0, P.clone(), state),
                lambda: ops.odom_accept(P, P.clone(), info[:2], off, 1, 100, 5.0, P.clone(), state),
                lambda: ops.odom_accept(P, P.clone(), info, off[:3], 1, 100, 5.0, P.clone(), state)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.odom_predict(P.float(), P.clone(), 1)
    keys, acc, tinfo, info5 = ops.map_crop_table(64, cuda)
    k2, a2, _, i2 = ops.map_crop_table(16, cuda)
    centre, origin = P[0], torch.zeros(3, dtype=torch.float64, device=cuda)
    for bad in (lambda: ops.map_crop(keys, acc, centre, origin, 1.0, 1, keys, acc, info5), lambda: ops.map_crop(keys, acc, centre, origin, 1.0, -1, k2, a2, i2),
                lambda: ops.map_crop(keys, acc, centre, origin, 1.0, (1 << 21) + 1, k2, a2, i2), lambda: ops.map_crop(keys, acc, centre, origin, 4096.0, 1, k2, a2, i2),
                lambda: ops.map_crop(keys, acc, centre[:11], origin, 1.0, 1, k2, a2, i2), lambda: ops.map_crop(keys, acc, centre, origin, 1.0, 1, k2, a2, i2[:4]),
                lambda: ops.map_crop(keys[:48], acc[:48], centre, origin, 1.0, 1, k2, a2, i2)):
        with pytest.raises(ValueError):
            bad()
    pts, poff = torch.zeros((10, 3), device=cuda), torch.tensor([0, 10], dtype=torch.int32, device=cuda)
    dirty, surf = torch.zeros(64, dtype=torch.uint8, device=cuda), torch.zeros((64, 8), device=cuda)
    for bad in (lambda: ops.map_touch(pts, poff, P[:1], origin, 1.0, keys, dirty[:32]), lambda: ops.map_touch(pts, poff, P[:1], origin, 1.0, keys, dirty, 3),
                lambda: ops.map_touch(pts, poff, P[:1], origin, 1.0, keys, dirty, 1, 1, 1), lambda: ops.map_touch(pts, poff, P[:1], origin, 0.01, keys, dirty),
                lambda: ops.map_surface_touched(keys, acc, surf[:32], dirty), lambda: ops.map_surface_touched(keys, acc, surf, dirty, 1, 3),
                lambda: ops.map_surface_touched(keys, acc, surf, dirty[:63]), lambda: ops.map_surface_touched(keys, acc[:32], surf, dirty)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.map_touch(pts, poff, P[:1], origin, 1.0, keys, dirty.to(torch.int32))
    # the three wrappers of this file through every check they share with the map's (tests/test_map_gpu.py has the others): ONE wrong
    # argument a call, the exception and the words "<wrapper>: <argument>".  map_crop names a wrong origin under centre_pose's message.
    surf_off = torch.zeros((64 * 8 + 1,), device=cuda)[1:].view(64, 8)      # one float off a 16-byte boundary
    assert surf_off.is_contiguous() and surf_off.data_ptr() % 16 == 4
    good = dict(map_crop=dict(keys_in=keys, acc_in=acc, centre_pose=centre, origin=origin, inv_cell=1.0, keep_cells=1, keys=k2, acc=a2, info5=i2),
                map_touch=dict(points=pts, offsets=poff, poses=P[:1], origin=origin, inv_cell=1.0, keys=keys, dirty=dirty),
                map_surface_touched=dict(keys=keys, acc=acc, surf=surf, dirty=dirty))
    wrong = [("map_crop", dict(keys=k2[:12]), "keys"), ("map_crop", dict(keys_in=keys[:48]), "keys"), ("map_touch", dict(keys=keys[:48]), "keys"),
             ("map_surface_touched", dict(keys=keys[:48]), "keys"),
             ("map_crop", dict(acc=a2[:, :3]), "acc"), ("map_crop", dict(acc_in=acc[:, :3]), "acc"), ("map_surface_touched", dict(acc=acc[:, :3]), "acc"),
             ("map_surface_touched", dict(surf=surf_off), "surf"),
             ("map_touch", dict(dirty=dirty[:32]), "dirty"), ("map_surface_touched", dict(dirty=dirty[:32]), "dirty"),
             ("map_touch", dict(scan0=1, scan1=1), "scans"),
             ("map_crop", dict(inv_cell=4096.0), "inv_cell"), ("map_touch", dict(inv_cell=4096.0), "inv_cell"),
             ("map_crop", dict(origin=origin[:2]), "centre_pose"), ("map_touch", dict(origin=origin[:2]), "origin"),
             ("map_crop", dict(keys=keys, acc=acc), "the new table"),
             ("map_crop", dict(info5=i2[:4]), "info5"), ("map_surface_touched", dict(info=torch.zeros(3, dtype=torch.int64, device=cuda)), "info")]
    for name, args in good.items():
        getattr(ops, name)(**args)      # the table's calls are good ones but for the one argument
    for name, bad, arg in wrong:
        with pytest.raises(ValueError, match=f"{name}: {arg}"):
            getattr(ops, name)(**dict(good[name], **bad))
    with pytest.raises(ValueError):
        odometry.estimate_poses([torch.zeros((0, 3), device=cuda)], None)
    with pytest.raises(ValueError):
        odometry.estimate_poses([pts], None, start=np.zeros(11))
