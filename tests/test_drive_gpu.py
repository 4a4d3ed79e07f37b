"""lpd_drive_steps / lpd_drive_plan / lpd_drive_rows, their ops wrappers and lpdnet_hip/drive.py on the GPU against tests/drive_ref.py.

`q`, `D`, `plan`, `position` (bits), the offsets and the rows (bits) equal the numpy restatement EXACTLY in every case: there is no
tolerance and no case is excluded.  Every result is computed twice, the second time on another stream, and the two are torch.equal.
The output always lies between guard rows, which must keep their fill."""
import ctypes

import numpy as np
import pytest
import torch

import clean_ref
import drive_ref as R
import places_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD, FILL = 64, -77.25
_REFS = {}


def _ref(key, pts, lengths, P, length, stride, frame):
    """the restatement's result, computed once per case and shared (read-only)"""
    if key not in _REFS:
        _REFS[key] = R.drive(pts, lengths, P, length, stride, frame)
    return _REFS[key]


def _bits32(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_points(cuda, pts, ld, misaligned=False):
    """[rows, 3] -> a device tensor whose rows are ld floats apart; misaligned: the table starts 4 bytes behind a 16-byte boundary"""
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


def _run(cuda, pts, lengths, P, length, stride, frame, ld=3, misaligned=False, max_len=None, stream=None):
    """steps, cumsum, plan, rows through ops -> dict of host arrays; the rows between guard rows"""
    from lpdnet_hip import ops
    S = len(lengths)
    L, T = ops.drive_units(length, "length"), ops.drive_units(stride, "stride")
    dp = _device_points(cuda, pts, ld, misaligned)
    off = torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)).to(cuda)
    poses = torch.from_numpy(np.ascontiguousarray(P)).to(cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        q, D = ops.drive_distance(poses)
        W = R.window_count(int(D[-1].item()), L, T)
        res = dict(q=q.cpu().numpy(), D=D.cpu().numpy(), W=W)
        if W:
            plan, position = ops.drive_plan(D, off, poses, L, T, 0, W)
            n = plan[:, 3].cpu().numpy().astype(np.int64)
            out_off = torch.from_numpy(np.concatenate(([0], np.cumsum(n))).astype(np.int32)).to(cuda)
            total = int(n.sum())
            big = torch.full((total + 2 * GUARD, 3), FILL, dtype=torch.float32, device=cuda)
            if total:
                ops.drive_rows(dp, off, poses, plan, out_off, int(n.max()) if max_len is None else max_len, total, frame, big[GUARD:GUARD + total])
            torch.cuda.synchronize()
            big = big.cpu().numpy()
            assert (big[:GUARD] == f32(FILL)).all() and (big[GUARD + total:] == f32(FILL)).all()      # the guard rows are untouched
            res.update(plan=plan.cpu().numpy(), position=position.cpu().numpy(), out=big[GUARD:GUARD + total], out_off=out_off.cpu().numpy())
    torch.cuda.synchronize()
    return res


def _twice(cuda, *a, **kw):
    """the same bits in every launch: the default stream, then a second stream"""
    one = _run(cuda, *a, **kw)
    two = _run(cuda, *a, stream=torch.cuda.Stream(device=cuda), **kw)
    assert one.keys() == two.keys()
    for k in one:
        x, y = np.asarray(one[k]), np.asarray(two[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    return one


def _same(got, want):
    assert np.array_equal(got["q"], want["q"]), np.nonzero(got["q"] != want["q"])
    assert np.array_equal(got["D"], want["D"]) and got["W"] == want["W"]
    if want["W"] == 0:
        return
    assert np.array_equal(got["plan"], want["plan"]), (got["plan"], want["plan"])
    assert np.array_equal(_bits64(got["position"]), _bits64(want["position"]))
    assert np.array_equal(got["out_off"], want["out_off"])
    assert got["out"].shape == want["out"].shape
    bad = np.nonzero((_bits32(got["out"]) != _bits32(want["out"])).any(1))[0]
    assert bad.size == 0, (bad[:8], got["out"][bad[:4]], want["out"][bad[:4]])


def _case(seed, lengths, step=(0.5, 1.5), origin=(5.7e6, 6.2e5, 80.0)):
    g = np.random.default_rng(seed)
    S = len(lengths)
    return R.make_drive(g, lengths, step=g.uniform(step[0], step[1], max(S - 1, 0)), heading_noise=0.05, origin=origin)


# (S, length, stride): the smallest drives get windows short enough to have some
SIZES = [(1, 0.5, 0.25), (2, 0.5, 0.25), (63, 4.0, 2.0), (64, 4.0, 2.0), (65, 4.0, 2.0), (300, 10.0, 2.5)]


@pytest.mark.parametrize("S,length,stride", SIZES)
def test_short_scans_equal_the_restatement(cuda, S, length, stride):
    """scan lengths 1 .. 7 drawn at random: many scans per 1024-row chunk, chunk boundaries inside and between scans; more scans in a chunk
    than the workgroup keeps relative poses for (S = 300), and fewer (the others); both frames; ld 3 and 4"""
    lengths = np.random.default_rng(S).integers(1, 8, S).tolist()
    pts, P = _case(100 + S, lengths, step=(0.05, 0.15) if S == 300 else (0.5, 1.5))      # S = 300: about a hundred scans per window
    for frame in (0, 1):
        want = _ref(("short", S, frame), pts, lengths, P, length, stride, frame)
        _same(_twice(cuda, pts, lengths, P, length, stride, frame), want)
        _same(_run(cuda, pts, lengths, P, length, stride, frame, ld=4), want)
    assert want["W"] == (0 if S == 1 else want["W"]) and (S < 3 or want["W"] >= 3)
    if S == 300:
        assert (want["plan"][:, 1] - want["plan"][:, 0]).max() > 64 and want["plan"][:, 3].max() < 1024      # a chunk of more than 64 scans


@pytest.mark.parametrize("S", [1, 2, 65])
def test_pushbroom_scans_of_541_rows(cuda, S):
    lengths = [541] * S
    pts, P = _case(200 + S, lengths)
    length, stride = (0.5, 0.25) if S < 3 else (8.0, 4.0)
    for frame in (0, 1):
        want = _ref(("push", S, frame), pts, lengths, P, length, stride, frame)
        _same(_twice(cuda, pts, lengths, P, length, stride, frame), want)
    _same(_run(cuda, pts, lengths, P, length, stride, 1, ld=4), want)
    _same(_run(cuda, pts, lengths, P, length, stride, 1, ld=4, misaligned=True), want)
    _same(_run(cuda, pts, lengths, P, length, stride, 1, ld=3, misaligned=True), want)
    _same(_run(cuda, pts, lengths, P, length, stride, 1, ld=7), want)


def test_scans_over_several_chunks_and_a_scan_of_no_rows(cuda):
    """1, 1023, 1024, 1025 and 3000 rows: one scan over several chunks; a zero-length scan in the middle of a window and at its ends;
    scans of 16 rows: 64 or 65 scans in a chunk, either side of the relative-pose table's size"""
    for key, lengths in (("chunks", [1, 1023, 1024, 1025, 3000, 1, 1024, 3000, 1025, 1023] * 2),
                         ("empty", [5, 0, 7, 300, 0, 0, 1100, 3, 0, 2, 0, 900, 40, 0] * 2 + [0]),
                         ("sixteen", [16] * 100 + ([16] * 63 + [15]) * 2 + [15] * 72)):
        pts, P = _case(len(lengths), lengths, step=(0.05, 0.1) if key == "sixteen" else (0.5, 1.5))
        for frame in (0, 1):
            want = _ref((key, frame), pts, lengths, P, 6.0, 3.0, frame)
            assert want["W"] >= 3 and (key != "sixteen" or want["plan"][:, 3].min() > 1024)
            _same(_twice(cuda, pts, lengths, P, 6.0, 3.0, frame), want)
        _same(_run(cuda, pts, lengths, P, 6.0, 3.0, 1, ld=4), want)


def _line(steps):
    x = np.concatenate(([0.0], np.cumsum(np.asarray(steps, dtype=np.float64))))
    P = np.zeros((len(x), 12))
    P[:, [0, 5, 10]] = 1.0
    P[:, 3] = x
    return P


HAND_MADE = {      # tests/test_drive_cpu.py writes the same windows down
    "unit steps, stride 2": ([1] * 10, 4.0, 2.0, [(0, 4, 2), (2, 6, 4), (4, 8, 6), (6, 10, 8)]),
    "unit steps, stride 4": ([1] * 10, 4.0, 4.0, [(0, 4, 2), (4, 8, 6)]),
    "stride > length": ([1] * 10, 2.0, 5.0, [(0, 2, 1), (5, 7, 6)]),
    "stride = length / 3": ([1] * 10, 3.0, 1.0, [(w, w + 3, w + 2) for w in range(8)]),
    "stationary stretch": ([1, 1, 0, 0, 0, 1, 1, 1, 1], 2.0, 1.0, [(0, 2, 1), (1, 6, 2), (2, 7, 6), (6, 8, 7), (7, 9, 8)]),
    "a step longer than length": ([1, 1, 10, 1, 1], 2.0, 2.0, [(0, 2, 1), (2, 3, 2), (3, 3, -1), (3, 3, -1), (3, 3, -1), (3, 3, -1), (3, 5, 4)]),
    "one scan": ([], 2.0, 1.0, []),
}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_drives(cuda, name):
    steps, length, stride, windows = HAND_MADE[name]
    P = _line(steps)
    S = len(P)
    lengths = [3 + (i % 4) for i in range(S)]
    pts = (np.random.default_rng(S).uniform(-30, 30, (sum(lengths), 3))).astype(f32)
    for frame in (0, 1):
        got = _twice(cuda, pts, lengths, P, length, stride, frame)
        _same(got, _ref(("hand", name, frame), pts, lengths, P, length, stride, frame))
        assert got["W"] == len(windows)
        if windows:
            assert [tuple(r[:3]) for r in got["plan"].tolist()] == windows
            off = np.concatenate(([0], np.cumsum(lengths)))
            assert got["plan"][:, 3].tolist() == [int(off[e] - off[f]) for f, e, _ in windows]
            assert got["position"][:, 0].tolist() == [float(P[r, 3]) if r >= 0 else 0.0 for _, _, r in windows]


def test_reference_scan_rows_are_bit_copies_under_signed_permutations(cuda):
    g = np.random.default_rng(9)
    S, n = 24, 5
    P = np.zeros((S, 12))
    for i in range(S):
        M = np.zeros((3, 3))
        M[np.arange(3), g.permutation(3)] = g.choice([-1.0, 1.0], 3)
        P[i] = np.concatenate((M, np.array([[5.7e6 + 0.9 * i], [6.2e5 - 0.3 * i], [70.0]])), 1).reshape(12)
    pts = (g.uniform(-1, 1, (S * n, 3)) * 50.0).astype(f32)
    got = _twice(cuda, pts, [n] * S, P, 4.0, 2.0, 1)
    _same(got, _ref(("perm",), pts, [n] * S, P, 4.0, 2.0, 1))
    assert got["W"] >= 3
    for w, (first, end, ref, _) in enumerate(got["plan"]):
        at = int(got["out_off"][w]) + (ref - first) * n
        assert np.array_equal(_bits32(got["out"][at:at + n]), _bits32(pts[ref * n:(ref + 1) * n]))


def _drive_tensors(cuda, pts, lengths, P):
    dp = torch.from_numpy(pts).to(cuda)
    off = torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)).to(cuda)
    return dp, off, torch.from_numpy(np.ascontiguousarray(P)).to(cuda)


def test_window_batches(cuda):
    """w0 > 0; W beyond the drive's end gives empty windows; two batches equal one -- the plan and the rows"""
    from lpdnet_hip import ops
    lengths = np.random.default_rng(5).integers(1, 40, 150).tolist()
    pts, P = _case(31, lengths)
    want = _ref(("batch",), pts, lengths, P, 6.0, 2.0, 1)
    W, S, L, T = want["W"], len(lengths), want["L"], want["T"]
    assert W >= 8
    dp, off, poses = _drive_tensors(cuda, pts, lengths, P)
    _, D = ops.drive_distance(poses)
    one, pos_one = ops.drive_plan(D, off, poses, L, T, 0, W + 3)
    assert np.array_equal(one.cpu().numpy()[:W], want["plan"]) and one.cpu().numpy()[W:].tolist() == [[S, S, -1, 0]] * 3
    assert np.array_equal(_bits64(pos_one.cpu().numpy()[:W]), _bits64(want["position"])) and not pos_one[W:].any()
    k = W // 3
    a, pos_a = ops.drive_plan(D, off, poses, L, T, 0, k)
    b, pos_b = ops.drive_plan(D, off, poses, L, T, k, W + 3 - k)
    assert torch.equal(torch.cat((a, b)), one) and torch.equal(torch.cat((pos_a, pos_b)).view(torch.int64), pos_one.view(torch.int64))
    total = int(want["out_off"][-1])
    out_off = torch.from_numpy(np.concatenate((want["out_off"], [total] * 3)).astype(np.int32)).to(cuda)
    longest = int(want["plan"][:, 3].max())
    whole = ops.drive_rows(dp, off, poses, one, out_off, longest, total, 1)
    split = torch.full((total, 3), FILL, dtype=torch.float32, device=cuda)
    ops.drive_rows(dp, off, poses, b, out_off[k:], longest, total, 1, split)      # the second batch first: its rows only
    at = int(want["out_off"][k])
    assert (split[:at] == FILL).all() and torch.equal(split[at:].view(torch.int32), whole[at:].view(torch.int32))
    ops.drive_rows(dp, off, poses, a, out_off[:k + 1], longest, total, 1, split)
    assert torch.equal(split.view(torch.int32), whole.view(torch.int32))
    assert np.array_equal(_bits32(whole.cpu().numpy()), _bits32(want["out"]))


def test_a_window_longer_than_max_len_is_not_written(cuda):
    lengths = np.random.default_rng(6).integers(1, 60, 120).tolist()
    pts, P = _case(32, lengths)
    want = _ref(("maxlen",), pts, lengths, P, 6.0, 3.0, 1)
    n = want["plan"][:, 3]
    max_len = int(np.sort(n)[len(n) // 2])
    long = n > max_len
    assert long.any() and (~long).any() and long[1:-1].any()
    got = _run(cuda, pts, lengths, P, 6.0, 3.0, 1, max_len=max_len)
    for w in range(want["W"]):
        a, b = int(want["out_off"][w]), int(want["out_off"][w + 1])
        if long[w]:
            assert (got["out"][a:b] == f32(FILL)).all()
        else:
            assert np.array_equal(_bits32(got["out"][a:b]), _bits32(want["out"][a:b]))


def test_a_plan_or_offsets_that_are_not_what_they_should_be_write_nothing_outside(cuda):
    """plan lines and output offsets that break the definition: those windows are not written, the others are, the guards stay"""
    from lpdnet_hip import ops
    lengths = [20] * 60
    pts, P = _case(33, lengths)
    want = _ref(("broken",), pts, lengths, P, 6.0, 3.0, 0)
    W, S = want["W"], len(lengths)
    assert W >= 8
    dp, off, poses = _drive_tensors(cuda, pts, lengths, P)
    plan = want["plan"].copy()
    plan[0] = (-1, plan[0, 1], plan[0, 2], plan[0, 3])           # first < 0
    plan[1] = (plan[1, 0], S + 1, plan[1, 2], plan[1, 3])        # end > S
    plan[2] = (plan[2, 0], plan[2, 1], plan[2, 1], plan[2, 3])   # ref == end
    plan[3] = (plan[3, 0], plan[3, 1], plan[3, 2], plan[3, 3] + 1)      # rows that are not the offsets' difference
    plan[4] = (plan[4, 1], plan[4, 0], plan[4, 2], plan[4, 3])   # first > end
    out_off = want["out_off"].astype(np.int32).copy()
    total = int(out_off[-1])
    big = torch.full((total + 2 * GUARD, 3), FILL, dtype=torch.float32, device=cuda)
    ops.drive_rows(dp, off, poses, torch.from_numpy(plan).to(cuda), torch.from_numpy(out_off).to(cuda), int(plan[:, 3].max()), total, 0,
                   big[GUARD:GUARD + total])
    got = big.cpu().numpy()
    assert (got[:GUARD] == f32(FILL)).all() and (got[GUARD + total:] == f32(FILL)).all()
    got = got[GUARD:GUARD + total]
    for w in range(W):
        a, b = int(out_off[w]), int(out_off[w + 1])
        if w < 5:
            assert (got[a:b] == f32(FILL)).all(), w
        else:
            assert np.array_equal(_bits32(got[a:b]), _bits32(want["out"][a:b])), w


def test_poses_that_hold_nan(cuda):
    """NaN and inf in rotations and translations: q = 0 for such a step, the plan and the positions equal the restatement, the rows
    equal it where they are numbers and are NaN where it is NaN (the sign and payload of a NaN are the machine's).  The guards
    stay untouched (checked in _run)."""
    lengths = np.random.default_rng(7).integers(1, 30, 100).tolist()
    pts, P = _case(34, lengths, origin=(0.0, 0.0, 0.0))
    P[10, 3] = np.nan
    P[30, 0] = np.nan
    P[50, 7] = np.inf
    P[51, :] = np.nan
    P[70, 5] = -np.inf
    for frame in (0, 1):
        want = _ref(("nan", frame), pts, lengths, P, 6.0, 3.0, frame)
        got = _twice(cuda, pts, lengths, P, 6.0, 3.0, frame)
        assert np.array_equal(got["q"], want["q"]) and want["q"][[10, 11, 50, 51, 52]].tolist() == [0] * 5
        assert np.array_equal(got["plan"], want["plan"]) and np.array_equal(got["out_off"], want["out_off"])
        assert np.array_equal(got["position"], want["position"], equal_nan=True)
        assert np.isnan(want["out"]).any() and not np.isnan(want["out"]).all()
        assert np.array_equal(np.isnan(got["out"]), np.isnan(want["out"]))
        ok = ~np.isnan(want["out"])
        assert np.array_equal(_bits32(got["out"])[ok], _bits32(want["out"])[ok])


def test_argument_errors_return_err_arg(cuda):
    from lpdnet_hip import _lib
    lib = _lib.load()
    ERR = _lib.DEFINES["LPD_ERR_ARG"]
    t = torch.zeros((4096,), dtype=torch.float64, device=cuda)
    p = ctypes.c_void_p(t.data_ptr())
    o = ctypes.c_void_p(t.data_ptr() + 8192)
    big = 1 << 22
    assert lib.lpd_drive_steps(None, 4, p, None) == ERR and lib.lpd_drive_steps(p, 4, None, None) == ERR
    assert lib.lpd_drive_steps(p, 0, o, None) == ERR and lib.lpd_drive_steps(p, big + 1, o, None) == ERR
    assert b"lpd_drive_steps" in lib.lpd_last_error()
    good = dict(D=p, S=4, offsets=p, poses=p, L=65536, T=65536, w0=0, W=1, plan=o, position=o)
    for bad in (dict(D=None), dict(offsets=None), dict(poses=None), dict(plan=None), dict(position=None), dict(S=0), dict(S=big + 1), dict(L=0),
                dict(T=0), dict(L=(1 << 40) + 1), dict(T=-5), dict(W=0), dict(W=65536), dict(w0=-1), dict(w0=big)):
        a = dict(good, **bad)
        assert lib.lpd_drive_plan(a["D"], a["S"], a["offsets"], a["poses"], a["L"], a["T"], a["w0"], a["W"], a["plan"], a["position"], None) == ERR, bad
    assert b"lpd_drive_plan" in lib.lpd_last_error()
    good = dict(points=p, ld=3, rows=8, offsets=p, poses=p, S=4, plan=p, W=1, out_off=p, frame=1, max_len=8, out=o)
    for bad in (dict(points=None), dict(offsets=None), dict(poses=None), dict(plan=None), dict(out_off=None), dict(out=None), dict(ld=2),
                dict(rows=0), dict(S=0), dict(S=big + 1), dict(W=0), dict(W=65536), dict(frame=2), dict(frame=-1), dict(max_len=0),
                dict(max_len=(1 << 20) + 1), dict(out=p)):
        a = dict(good, **bad)
        assert lib.lpd_drive_rows(a["points"], a["ld"], a["rows"], a["offsets"], a["poses"], a["S"], a["plan"], a["W"], a["out_off"], a["frame"],
                                  a["max_len"], a["out"], None) == ERR, bad
    assert b"lpd_drive_rows" in lib.lpd_last_error()
    torch.cuda.synchronize()


def _ground_drive():
    """200 scans of 300 rows with labelled ground (tests/clean_ref.py scenes), half a metre apart"""
    S, n = 200, 300
    pts = np.concatenate([clean_ref.scene(n, 900 + i)[0] for i in range(S)])
    g = np.random.default_rng(12)
    _, P = R.make_drive(g, [n] * S, step=g.uniform(0.4, 0.6, S - 1), heading_noise=0.01, origin=(5.7e6, 6.2e5, 80.0))
    return pts, [n] * S, P


def test_plan_windows_and_accumulate(cuda):
    from lpdnet_hip import drive
    pts, lengths, P = _ground_drive()
    for frame, code in (("reference", 1), ("world", 0)):
        want = _ref(("ground", code), pts, lengths, P, 20.0, 10.0, code)
        plan = drive.plan_windows(P, 20.0, 10.0, device=cuda, lengths=lengths)
        assert len(plan) == want["W"] >= 6
        table = torch.stack((plan.first, plan.end, plan.ref, plan.rows), 1).cpu().numpy()
        assert np.array_equal(table, want["plan"]) and np.array_equal(plan.offsets.cpu().numpy(), want["out_off"])
        assert np.array_equal(plan.row_counts, want["plan"][:, 3])
        assert np.array_equal(_bits64(plan.positions.cpu().numpy()), _bits64(want["position"][:, :2]))
        got = drive.accumulate(pts, lengths, plan=plan, frame=frame)
        assert np.array_equal(_bits32(got.points.cpu().numpy()), _bits32(want["out"])) and got.lengths() == want["plan"][:, 3].tolist()
        part = drive.accumulate(torch.from_numpy(pts).to(cuda), lengths, plan=plan, frame=frame, windows=(2, 5))
        a, b = int(want["out_off"][2]), int(want["out_off"][5])
        assert np.array_equal(_bits32(part.points.cpu().numpy()), _bits32(want["out"][a:b]))
        assert np.array_equal(part.offsets.cpu().numpy(), want["out_off"][2:6] - a)
        alone = drive.accumulate([pts[i * 300:(i + 1) * 300] for i in range(len(lengths))], None, P.reshape(-1, 3, 4), length=20.0, stride=10.0,
                                 frame=frame, device=cuda)
        assert torch.equal(alone.points.view(torch.int32), got.points.view(torch.int32)) and torch.equal(alone.offsets, got.offsets)
    onerow = drive.plan_windows(P, 20.0, 10.0, device=cuda)      # no lengths: one row per scan
    assert torch.equal(onerow.rows, onerow.end - onerow.first)


def test_submaps_from_drive_end_to_end(cuda):
    """equal to the public make_submaps(clean=) fed with the restatement's rows and lengths; the positions feed the place lists"""
    from lpdnet_hip import drive, places, submap
    pts, lengths, P = _ground_drive()
    want = _ref(("ground", 1), pts, lengths, P, 20.0, 10.0, 1)
    clean = submap.RoadRemoval(r_max=50.0, H=64, seed=3)
    sub, positions = drive.submaps_from_drive(pts, lengths, P, 20.0, 10.0, num_points=256, clean=clean, device=cuda)
    ref = submap.make_submaps(want["out"], want["plan"][:, 3].tolist(), num_points=256, clean=clean, device=cuda)
    assert sub.x.shape == (want["W"], 1, 256, 3) and torch.equal(sub.x.view(torch.int32), ref.x.view(torch.int32))
    for name in ("level", "cells", "n_raw"):
        assert torch.equal(getattr(sub, name), getattr(ref, name)), name
    assert torch.equal(sub.center.view(torch.int32), ref.center.view(torch.int32)) and torch.equal(sub.scale.view(torch.int32), ref.scale.view(torch.int32))
    assert torch.equal(sub.cleaned.info, ref.cleaned.info) and torch.equal(sub.cleaned.offsets, ref.cleaned.offsets)
    assert (sub.cleaned.info[:, 1] >= 0).any() and int(sub.n_raw.sum()) < int(want["out_off"][-1])      # a road was found and removed
    assert positions.shape == (want["W"], 2) and np.array_equal(_bits64(positions.cpu().numpy()), _bits64(want["position"][:, :2]))
    assert np.array_equal(sub.plan.ref.cpu().numpy(), want["plan"][:, 2])
    # two window batches: without a cleaning the batches do not matter
    plain = drive.submaps_from_drive(pts, lengths, P, 20.0, 10.0, num_points=256, device=cuda)[0]
    split = drive.submaps_from_drive(pts, lengths, P, 20.0, 10.0, num_points=256, device=cuda, window_batch=4)[0]
    direct = submap.make_submaps(want["out"], want["plan"][:, 3].tolist(), num_points=256, device=cuda)
    assert torch.equal(plain.x.view(torch.int32), direct.x.view(torch.int32)) and torch.equal(split.x.view(torch.int32), direct.x.view(torch.int32))
    assert torch.equal(split.level, direct.level) and torch.equal(split.n_raw, direct.n_raw)
    # the positions go straight into the place lists (radii that give both lists members on a 90 m drive)
    lists = places.training_lists(positions, pos_radius=15.0, near_radius=35.0)
    pos, near = lists.to_lists()
    rp, rn = places_ref.training_lists(positions.cpu().numpy(), 15.0, 35.0)
    assert len(pos) == want["W"] and all(np.array_equal(a, b) for a, b in zip(pos, rp)) and all(np.array_equal(a, b) for a, b in zip(near, rn))
    assert sum(len(a) for a in pos) > 0


def test_measure_fp32_error_of_the_kernels_rows_at_utm_scale(cuda):
    """The error is bounded by the arithmetic: coordinates below 256 m after the subtraction, an fp32 ulp there is 1.5e-5 m, three
    products and three sums plus the rounding of M and u.  Asserted at 1e-3 m on the GPU's own output."""
    g = np.random.default_rng(10)
    S, n = 120, 40
    pts, P = R.make_drive(g, [n] * S, step=g.uniform(0.2, 1.2, S - 1), heading_noise=0.05, origin=(5.7e6, 6.2e5, 80.0), point_scale=60.0)
    for frame in (0, 1):
        got = _run(cuda, pts, [n] * S, P, 20.0, 10.0, frame)
        off = np.concatenate(([0], np.cumsum([n] * S)))
        ext = R.rows_extended(pts, off, P, got["plan"], frame)
        err = float(np.abs(got["out"].astype(np.longdouble) - ext).max())
        print(f"MEASURE drive rows on the GPU vs extended precision, frame {frame}: max |error| = {err:.3e} m over {len(ext)} rows")
        assert float(np.abs(ext).max()) < 256.0 and err < 1e-3
