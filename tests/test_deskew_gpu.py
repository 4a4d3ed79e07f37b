"""lpd_scan_deskew / lpd_drive_motions / lpd_odom_motion, their ops wrappers, odometry.deskew_scans and odometry.estimate_poses with
times on the GPU against tests/deskew_ref.py.

Everything is exact: the bits of the rows and of the motions and the integers of the counters; the chain with times equals the
restatement's in the bits of its poses, of its deskewed rows and of its final map."""
import numpy as np
import pytest
import torch

import deskew_cases as C
import deskew_ref as D
import map_ref as M
import odom_cases as OC
import odom_ref as O

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
CANARY = 777.25
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


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def _placed(cuda, a, ld, shift):
    """the rows of `a` [n, 3] in a device buffer with rows `ld` floats apart that starts `shift` floats behind a 16-byte boundary; the
    other floats are 9.5 -> the [n, ld] view"""
    n = a.shape[0]
    host = np.full((n, ld), 9.5, dtype=f32)
    host[:, :3] = a
    flat = torch.full((n * ld + 8,), 9.5, dtype=torch.float32, device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = flat[shift:shift + n * ld].view(n, ld)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return view


def _out(cuda, n, shift=0):
    flat = torch.full((3 * n + 8,), CANARY, dtype=torch.float32, device=cuda)
    return flat[shift:shift + 3 * n].view(n, 3)


LENGTHS = [0, 1, 3, 1023, 1024, 1025, 2049]      # 5125 rows: six chunks, scans that end one row before, at and one row behind a chunk


def _table(name="lengths"):
    def make():
        if name == "lengths":
            pts, lengths, tm, mo = C.random_table(21, LENGTHS)
        elif name == "tiny":      # 900 scans of 1 .. 4 rows: every chunk of 1024 rows holds more scans than the 64 of the staged table
            pts, lengths, tm, mo = C.random_table(22, np.random.default_rng(22).integers(1, 5, 900))
        else:
            pts, lengths, tm, mo = C.boundary_table()
        off = M.offsets_of(lengths)
        return pts, lengths, tm, mo, off, D.deskew(pts, off, tm, mo)
    return _ref(("table", name), make)


def _run(cuda, pts, off, tm, mo, ld=3, shift=0, out=None, **kw):
    from lpdnet_hip import ops
    points = _placed(cuda, pts, ld, shift)
    out = _out(cuda, len(pts)) if out is None else out
    got, info = ops.scan_deskew(points, _t(cuda, off, np.int32), _t(cuda, tm, f32), _t(cuda, mo, f64), out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy(), info.cpu().numpy(), points


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,shift", [(3, 0), (3, 3), (4, 0), (4, 1), (5, 0)])
def test_rows_equal_the_restatement_at_every_layout(cuda, ld, shift):
    """ld 3 from a base 12 bytes behind a 16-byte boundary, ld 4 aligned (one 16-byte load a row) and misaligned, ld 5"""
    pts, lengths, tm, mo, off, (want, winfo) = _table()
    got, info, points = _run(cuda, pts, off, tm, mo, ld, shift)
    _bits(got, want, (ld, shift))
    assert info.tolist() == winfo.tolist() == [len(pts), 0]
    assert (points[:, 3:] == 9.5).all() and np.array_equal(points[:, :3].cpu().numpy(), pts)      # the input is only read
    assert np.abs(got - pts).max() > 0.5      # the rows really moved


def test_out_misaligned_and_out_in_place(cuda):
    from lpdnet_hip import ops
    pts, lengths, tm, mo, off, (want, winfo) = _table()
    for shift in (1, 2, 3):
        out = _out(cuda, len(pts), shift)
        got, info, _ = _run(cuda, pts, off, tm, mo, out=out)
        _bits(got, want, ("out", shift))
        flat = out.storage_offset()
        assert flat == shift and info.tolist() == winfo.tolist()
    points = _placed(cuda, pts, 3, 1)
    got, info = ops.scan_deskew(points, _t(cuda, off, np.int32), _t(cuda, tm, f32), _t(cuda, mo, f64), out=points)      # out is points
    _bits(got.cpu().numpy(), want, "in place")
    assert got.data_ptr() == points.data_ptr() and info.tolist() == winfo.tolist()


def test_more_scans_in_a_chunk_than_the_staged_table_holds(cuda):
    pts, lengths, tm, mo, off, (want, winfo) = _table("tiny")
    assert len(lengths) == 900 and len(pts) > 2048 and (np.searchsorted(off, [1024, 2048]) - np.searchsorted(off, [0, 1024]) > 64).all()
    got, info, _ = _run(cuda, pts, off, tm, mo)
    _bits(got, want, "tiny scans")
    assert info.tolist() == winfo.tolist()
    got4, _, _ = _run(cuda, pts, off, tm, mo, 4, 0)
    _bits(got4, want, "tiny scans, ld 4")


@pytest.mark.parametrize("scans", [(3, 5), (4, 7), (0, 3), (6, 7), (1, 2)])
def test_a_sub_range_of_the_scans_leaves_every_other_row_alone(cuda, scans):
    pts, lengths, tm, mo, off, _ = _table()
    canary = np.full((len(pts), 3), CANARY, dtype=f32)
    want, winfo = D.deskew(pts, off, tm, mo, 0.5, scans[0], scans[1], out=canary)
    got, info, _ = _run(cuda, pts, off, tm, mo, scan0=scans[0], scan1=scans[1])
    _bits(got, want, scans)
    n = int(off[scans[1]] - off[scans[0]])
    assert info.tolist() == winfo.tolist() == [n, 0] and int((got == CANARY).all(axis=1).sum()) == len(pts) - n


def test_a_broken_offsets_table(cuda):
    pts, lengths, tm, mo = C.random_table(23, np.full(30, 100))
    canary = np.full((len(pts), 3), CANARY, dtype=f32)
    bad = M.offsets_of(lengths).copy()
    bad[12] = bad[13] + 5      # descends inside the second chunk: that chunk is neither read nor written
    want, winfo = D.deskew(pts, bad, tm, mo, out=canary)
    assert 0 < winfo[0] < 3000 and (want[1024:2048] == CANARY).all() and not (want[:1024] == CANARY).any()
    got, info, _ = _run(cuda, pts, bad, tm, mo)
    _bits(got, want, "broken")
    assert info.tolist() == winfo.tolist()
    for lo, hi in ((0, 3001), (-1, 3000), (200, 100)):      # the call reads nothing
        worse = M.offsets_of(lengths).copy()
        worse[0], worse[-1] = lo, hi
        got, info, _ = _run(cuda, pts, worse, tm, mo)
        assert (got == CANARY).all() and info.tolist() == [0, 0]


@pytest.mark.parametrize("ref", [0.5, 0.0, 1.0])
def test_the_boundary_rows(cuda, ref):
    pts, lengths, tm, mo, off, _ = _table("boundary")
    want, winfo = D.deskew(pts, off, tm, mo, ref)
    got, info, _ = _run(cuda, pts, off, tm, mo, ref=ref)
    _bits(got, want, ref)
    assert info.tolist() == winfo.tolist() and winfo[1] == 3 * 15 + 2 * 36
    n0 = int(lengths[0])
    assert np.array_equal(got[:n0], pts[:n0])      # the identity motion: every row compares equal to its input
    with np.errstate(invalid="ignore"):
        stay = np.tile(~((tm[:n0] >= 0) & (tm[:n0] <= 1)), len(lengths)) | np.repeat(~np.isfinite(mo).all(axis=1), n0)
    _bits(got[stay], pts[stay], "passed through: bit copies")


def test_two_streams_and_two_launches_give_the_same_bits(cuda):
    from lpdnet_hip import ops
    pts, lengths, tm, mo, off, (want, winfo) = _table()
    args = (_placed(cuda, pts, 3, 0), _t(cuda, off, np.int32), _t(cuda, tm, f32), _t(cuda, mo, f64))
    outs, infos = [], []
    torch.cuda.synchronize(cuda)
    for s in [torch.cuda.Stream(device=cuda) for _ in range(2)]:
        with torch.cuda.stream(s):
            for _ in range(2):
                o, i = ops.scan_deskew(*args, out=_out(cuda, len(pts)))
                outs.append(o)
                infos.append(i)
    torch.cuda.synchronize(cuda)
    for o, i in zip(outs, infos):
        _bits(o.cpu().numpy(), want, "streams")
        assert i.tolist() == winfo.tolist()
    total = torch.zeros(2, dtype=torch.int64, device=cuda)
    for _ in range(3):
        ops.scan_deskew(*args, out=_out(cuda, len(pts)), info=total)      # a given info is added to
    assert total.tolist() == [3 * len(pts), 0]


# ---- the two motion rules ---------------------------------------------------------------------------------------------------------------------------
def test_motions_equal_the_restatement(cuda):
    from lpdnet_hip import ops
    d = _drive()
    P = d["truth"].copy()
    bad = P.copy()
    bad[2, 3], bad[4, 0] = np.nan, np.inf
    for poses in (P, bad, P[:1], P[:2], np.tile(P, (60, 1))):      # 360 scans: more than one workgroup
        got = ops.drive_motions(_t(cuda, poses, f64)).cpu().numpy()
        _same(got, D.drive_motions(poses), len(poses))
    got = ops.drive_motions(_t(cuda, bad, f64)).cpu().numpy()
    assert np.isfinite(got).all(axis=1).tolist() == [True, False, False, False, False, False]      # every motion that a bad pose is part of, and the last one's copy
    first = C.nominal_motion(1.5, 2.5)
    for poses in (P, bad):
        for fm in (None, first):
            motion = torch.full((6, 12), 7.0, dtype=torch.float64, device=cuda)
            for t in range(6):
                ops.odom_motion(_t(cuda, poses, f64), t, motion, None if fm is None else _t(cuda, fm, f64))
                _same(motion[t].cpu().numpy(), D.odom_motion(poses, t, fm), (t, fm is None))
                assert (motion[t + 1:] == 7.0).all()


# ---- odometry.deskew_scans ------------------------------------------------------------------------------------------------------------------------------
def _drive():
    return _ref("drive", lambda: C.skewed_drive(1, 1.5, 2.5, S=6, rows=2000))


def test_deskew_scans_from_poses_and_from_motions(cuda):
    from lpdnet_hip import odometry
    d = _drive()
    pts, tm = torch.from_numpy(d["points"]).to(cuda), torch.from_numpy(d["times"]).to(cuda)
    rows, info = odometry.deskew_scans(pts, d["lengths"], tm, motions=d["motions"])
    want, winfo = D.deskew_drive(d["points"], d["lengths"], d["times"], motions=d["motions"])
    assert rows.is_cuda and info.is_cuda and info.tolist() == winfo.tolist() == [12000, 0]
    _bits(rows.cpu().numpy(), want, "motions")
    res = float(np.linalg.norm(want.astype(f64) - d["clean"].astype(f64), axis=1).max())
    assert res <= C.RESIDUAL_BOUND * d["skew"], (res, d["skew"])
    poses = d["truth"].copy()
    poses[4, 7] = np.nan      # the motions of scans 3 and 4 are not finite, and scan 5 repeats scan 4's: their rows pass through and are counted
    rows, info = odometry.deskew_scans([pts[2000 * k:2000 * (k + 1)] for k in range(6)], None, [tm[2000 * k:2000 * (k + 1)] for k in range(6)],
                                       poses=torch.from_numpy(poses).to(cuda), ref=0.25)
    want, winfo = D.deskew_drive(d["points"], d["lengths"], d["times"], poses=poses, ref=0.25)
    _bits(rows.cpu().numpy(), want, "poses")
    assert info.tolist() == winfo.tolist() == [6000, 6000]
    _bits(rows[6000:].cpu().numpy(), d["points"][6000:], "passed through")
    rows, info = odometry.deskew_scans(pts, d["lengths"], tm, motions=d["motions"], scans=(2, 4))
    want, winfo = D.deskew(d["points"], M.offsets_of(d["lengths"]), d["times"], d["motions"], 0.5, 2, 4, out=d["points"])
    _bits(rows.cpu().numpy(), want, "scans 2 .. 4: the others are the input's")
    assert info.tolist() == winfo.tolist() == [4000, 0] and rows.data_ptr() != pts.data_ptr()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------------
KEEP_M, REFRESH, LOST = 20.0, 3, 3


def _chain_ref(lost=False):
    def make():
        d = _drive()
        pts, lengths = OC.with_lost_scan(d, LOST) if lost else (d["points"], d["lengths"])
        return pts, lengths, D.estimate(pts, lengths, d["times"], d["truth"][0], 1.0, keep_m=KEEP_M, refresh=REFRESH, first_motion=C.nominal_motion(1.5, 2.5))
    return _ref(("chain", lost), make)


def _estimate(cuda, pts, lengths, times, **kw):
    from lpdnet_hip import odometry
    search = odometry.OdometrySearch(**dict(dict(cell=1.0, keep=KEEP_M, refresh=REFRESH, capacity=1 << 14, first_motion=C.nominal_motion(1.5, 2.5)), **kw))
    return odometry.estimate_poses(torch.from_numpy(pts).to(cuda), lengths, _drive()["truth"][0], search, times=times)


def _mapping(keys, acc):
    keys, acc = keys.cpu().numpy(), acc.cpu().numpy()
    live = keys >= 0
    order = np.argsort(keys[live])
    return keys[live][order], acc[live][order][:, :3], acc[live][order][:, 3]


def _check_chain(odo, want, what):
    _same(odo.poses.cpu().numpy(), want["poses"], what)
    assert odo.valid.cpu().numpy().tolist() == want["valid"].tolist(), what
    assert odo.steps.cpu().numpy().tolist() == want["info"][:, 1].tolist() and odo.refused.cpu().numpy().tolist() == want["info"][:, 2].tolist(), what
    _same(odo.inliers.cpu().numpy(), want["inliers"], what)
    k, s, m = _mapping(odo.keys, odo.acc)
    cells = want["cells"]
    assert np.array_equal(k, cells.keys) and np.array_equal(s, cells.sums) and np.array_equal(m, cells.counts), what
    assert odo.lost == int((~want["valid"]).sum()) and odo.left_behind == sum(want["left"]), what


@pytest.mark.parametrize("surface", ["touched", "full"])
def test_estimate_poses_with_times_equals_the_restatement_bit_for_bit(cuda, surface):
    pts, lengths, want = _chain_ref()
    assert want["valid"].all() and len(want["left"]) == 1 and want["info"][1:, 1].tolist() == [8] * 5 and want["passed"] == 0
    odo = _estimate(cuda, pts, lengths, torch.from_numpy(_drive()["times"]).to(cuda), surface=surface)
    _check_chain(odo, want, surface)
    assert odo.points.is_cuda and odo.passed == 0
    _bits(odo.points.cpu().numpy(), want["points"], "the deskewed rows")
    plain = _ref("plain", lambda: O.estimate(pts, lengths, _drive()["truth"][0], 1.0, keep_m=KEEP_M, refresh=REFRESH, first_motion=C.nominal_motion(1.5, 2.5)))
    e, e0 = C.errors(want["poses"], _drive()["truth"]), C.errors(plain["poses"], _drive()["truth"])
    print(f"MEASURE deskew chain: worst {max(x[0] for x in e):.4f} degrees {max(x[1] for x in e):.4f} m with times, "
          f"{max(x[0] for x in e0):.4f} degrees {max(x[1] for x in e0):.4f} m without")
    assert max(x[1] for x in e) < max(x[1] for x in e0)


def test_a_lost_scan_and_rows_without_a_time(cuda):
    pts, lengths, want = _chain_ref(lost=True)
    assert want["valid"].tolist() == [True, True, True, False, True, True]
    odo = _estimate(cuda, pts, lengths, _drive()["times"])      # a host array is uploaded
    _check_chain(odo, want, "lost")
    _same(odo.poses[LOST].cpu().numpy(), want["pred"][LOST], "the lost scan keeps its prediction")
    _bits(odo.points.cpu().numpy(), want["points"], "the deskewed rows")
    tm = _drive()["times"].copy()
    tm[[5, 2500, 11999]] = (np.nan, 1.5, -0.25)
    want = _ref("no time", lambda: D.estimate(_drive()["points"], lengths, tm, _drive()["truth"][0], 1.0, keep_m=KEEP_M, refresh=REFRESH,
                                              first_motion=C.nominal_motion(1.5, 2.5)))
    odo = _estimate(cuda, _drive()["points"], lengths, [tm[2000 * k:2000 * (k + 1)] for k in range(6)])      # one array a scan
    _check_chain(odo, want, "no time")
    assert odo.passed == want["passed"] == 3
    _bits(odo.points[[5, 2500, 11999]].cpu().numpy(), _drive()["points"][[5, 2500, 11999]], "passed through")


def test_estimate_poses_without_times_is_the_call_it_was(cuda):
    from lpdnet_hip import odometry
    d = _drive()
    want = _ref("plain", lambda: O.estimate(d["points"], d["lengths"], d["truth"][0], 1.0, keep_m=KEEP_M, refresh=REFRESH,
                                            first_motion=C.nominal_motion(1.5, 2.5)))
    search = odometry.OdometrySearch(cell=1.0, keep=KEEP_M, refresh=REFRESH, capacity=1 << 14, first_motion=C.nominal_motion(1.5, 2.5))
    odo = odometry.estimate_poses(torch.from_numpy(d["points"]).to(cuda), d["lengths"], d["truth"][0], search)
    _check_chain(odo, want, "no times")
    assert odo.points is None and odo.passed == 0
    launches = {}
    from lpdnet_hip import ops
    ops.PROFILE = launches
    try:
        odometry.estimate_poses(torch.from_numpy(d["points"]).to(cuda), d["lengths"], d["truth"][0], search)
    finally:
        ops.PROFILE = None
    assert "odom_predict" in launches and not {"scan_deskew", "odom_motion", "drive_motions"} & set(launches)      # no new launch


def test_the_deskewed_rows_go_into_the_submaps_and_the_map_without_a_copy_back(cuda):
    from lpdnet_hip import drive, mapping
    pts, lengths, want = _chain_ref()
    odo = _estimate(cuda, pts, lengths, torch.from_numpy(_drive()["times"]).to(cuda))
    assert odo.points.is_cuda and odo.poses.is_cuda
    origin = _drive()["truth"][0, M.TRA]
    vmap = mapping.build_map(odo.points, lengths, odo.poses, cell=1.0, origin=origin)
    cells = M.insert(want["points"], M.offsets_of(lengths), want["poses"], origin, 1.0)
    assert vmap.occupied == len(cells.keys) and vmap.inserted == int(cells.info[0])
    raw = mapping.build_map(torch.from_numpy(pts).to(cuda), lengths, odo.poses, cell=1.0, origin=origin)
    print(f"MEASURE deskew map: occupied 1 m cells {vmap.occupied} from the deskewed rows, {raw.occupied} from the rows as they came")
    assert vmap.occupied < raw.occupied      # a sharper map
    sub, positions = drive.submaps_from_drive(odo.points, lengths, odo.poses, length=4.0, stride=2.0, num_points=256)
    assert positions.is_cuda and positions.shape[0] >= 2 and torch.isfinite(positions).all()
    loc = mapping.localize_scans(vmap, odo.points, lengths, odo.poses, scans=(4, 6))
    assert loc.poses.is_cuda


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments(cuda):
    from lpdnet_hip import odometry, ops
    pts, off = torch.zeros((10, 3), device=cuda), torch.tensor([0, 4, 10], dtype=torch.int32, device=cuda)
    tm, mo = torch.zeros(10, device=cuda), torch.zeros((2, 12), dtype=torch.float64, device=cuda)
    good = dict(points=pts, offsets=off, times=tm, motion=mo)
    ops.scan_deskew(**good)
    wide = torch.zeros((10, 4), device=cuda)
    flat = torch.zeros(40, device=cuda)
    wrong = [(dict(times=tm[:9]), "times"), (dict(times=torch.zeros(20, device=cuda)[::2]), "times"), (dict(motion=mo[:1]), "offsets"),
             (dict(motion=torch.zeros((2, 11), dtype=torch.float64, device=cuda)), "poses"), (dict(offsets=off[:2]), "offsets"),
             (dict(ref=1.5), "ref"), (dict(ref=float("nan")), "ref"), (dict(out=torch.zeros((9, 3), device=cuda)), "out"),
             (dict(out=torch.zeros((10, 4), device=cuda)[:, :3]), "out"), (dict(points=wide, out=wide[:, :3]), "out"),
             (dict(points=flat[:30].view(10, 3), out=flat[3:33].view(10, 3)), "out overlaps"), (dict(scan0=1, scan1=1), "scans"), (dict(scan1=3), "scans"),
             (dict(info=torch.zeros(3, dtype=torch.int64, device=cuda)), "info"), (dict(points=torch.zeros((10, 2), device=cuda)), "points")]
    for bad, arg in wrong:
        with pytest.raises(ValueError, match=f"scan_deskew: {arg}"):
            ops.scan_deskew(**dict(good, **bad))
    for bad in (dict(times=tm.double()), dict(motion=mo.float()), dict(out=torch.zeros((10, 3), dtype=torch.float64, device=cuda)), dict(points=None),
                dict(times=None), dict(info=torch.zeros(2, dtype=torch.int32, device=cuda))):
        with pytest.raises(TypeError):
            ops.scan_deskew(**dict(good, **bad))
    P = torch.zeros((3, 12), dtype=torch.float64, device=cuda)
    for bad in (lambda: ops.odom_motion(P, 3, P.clone()), lambda: ops.odom_motion(P, -1, P.clone()), lambda: ops.odom_motion(P, 1, P),
                lambda: ops.odom_motion(P, 1, P.clone()[:2]), lambda: ops.odom_motion(P, 1, P.clone(), torch.zeros(11, dtype=torch.float64, device=cuda)),
                lambda: ops.drive_motions(P[:, :11]), lambda: ops.drive_motions(P[:0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.drive_motions(P.float())
    with pytest.raises(TypeError):
        ops.odom_motion(P, 1, P.clone().float())
    for bad in (lambda: odometry.deskew_scans(pts, [4, 6], tm), lambda: odometry.deskew_scans(pts, [4, 6], tm, poses=mo, motions=mo),
                lambda: odometry.deskew_scans(pts, [4, 6], tm[:9], motions=mo), lambda: odometry.deskew_scans(pts, [4, 6], tm.double(), motions=mo),
                lambda: odometry.deskew_scans(pts, [4, 5], tm, motions=mo), lambda: odometry.deskew_scans(pts, [4, 6], tm, motions=mo, ref=-0.5),
                lambda: odometry.deskew_scans(pts, [4, 6], tm, motions=mo, scans=(1, 3)), lambda: odometry.deskew_scans(pts, [4, 6, 0], tm, motions=mo),
                lambda: odometry.estimate_poses(pts, [4, 6], times=tm[:9]), lambda: odometry.estimate_poses(pts, [4, 6], times=tm, time_ref=2.0),
                lambda: odometry.estimate_poses(pts, [4, 6], times=tm.double())):
        with pytest.raises(ValueError):
            bad()
