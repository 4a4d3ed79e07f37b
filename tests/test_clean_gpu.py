"""lpd_road_planes / lpd_clean_count / lpd_clean_fill, ops.road_planes / ops.clean_scans and submap's clean= on the GPU against
tests/clean_ref.py.

`mask`, `out` (bit-copies of the kept rows), `out_offsets`, `info` and `plane` equal the numpy restatement EXACTLY in every case:
there is no tolerance and no case is excluded.  Every result is also computed twice and the two are torch.equal."""
import ctypes

import numpy as np
import pytest
import torch

import clean_ref as R

pytestmark = pytest.mark.gpu
CHUNK = R.CHUNK      # LPD_CLEAN_CHUNK: rows of one workgroup
_REFS = {}


def _removal(P):
    from lpdnet_hip import submap
    return submap.RoadRemoval(**{k: (float(v) if k in R.FLOATS else int(v)) for k, v in P.items()})


def _ref(key, points, offsets, P, max_len):
    """the restatement's result, computed once per case and shared (read-only)"""
    if key not in _REFS:
        _REFS[key] = R.clean_batch(points[:, :3], offsets, P, max_len)
    return _REFS[key]


def _gpu(cuda, points, offsets, P, max_len):
    from lpdnet_hip import ops
    pts = torch.from_numpy(np.array(points, order="C")).to(cuda)      # a writable copy
    off = torch.tensor([int(v) for v in offsets], dtype=torch.int32, device=cuda)
    prm, B = _removal(P).c_params(), len(offsets) - 1
    res = []
    for _ in range(2):
        plane, info = ops.road_planes(pts, off, B, max_len, prm)
        road = (plane, info) if P["H"] > 0 else (None, None)
        out, out_off, mask = ops.clean_scans(pts, off, B, max_len, prm, *road, want_mask=True)
        res.append((plane, info, out, out_off, mask))
    torch.cuda.synchronize()
    a, b = res
    total = int(a[3][-1])
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])      # the same bits in every launch
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[2][:total].view(torch.int32), b[2][:total].view(torch.int32))
    assert a[2].shape == (points.shape[0], 3) and a[3].dtype == torch.int32 and a[4].dtype == torch.uint8 and a[3].is_cuda
    return dict(plane=a[0].cpu().numpy(), info=a[1].cpu().numpy(), out=a[2][:total].cpu().numpy(), out_offsets=a[3].cpu().numpy(),
                mask=a[4].cpu().numpy())


def _same(got, want):
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    assert np.array_equal(got["plane"].view(np.uint32), want["plane"].view(np.uint32)), (got["plane"], want["plane"])
    assert np.array_equal(got["out_offsets"], want["out_offsets"]), (got["out_offsets"], want["out_offsets"])
    assert np.array_equal(got["mask"], want["mask"])
    assert got["out"].shape == want["out"].shape and np.array_equal(got["out"].view(np.uint32), want["out"].view(np.uint32))


SIZES = [1, 2, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17]


@pytest.mark.parametrize("n", SIZES)
def test_one_scan_equals_the_restatement(cuda, n):
    """sizes around a wave and around a workgroup's chunk; refine 0 and 1; min_inliers = 2 so that the smallest scans can have a road"""
    pts, _ = R.scene(n, 30 + n, (0.04, -0.02))
    removed = []
    for refine in (0, 1):
        P = R.params(H=64, min_inliers=2, refine=refine, seed=n)
        got = _gpu(cuda, pts, [0, n], P, n)
        _same(got, _ref(("one", n, refine), pts, [0, n], P, n))
        removed.append(n - int(got["out_offsets"][1]))
        assert got["info"][0, 0] == n
    if n >= 63:
        assert got["info"][0, 1] >= 0 and 0.3 * n < removed[1] < 0.8 * n      # a road was found and about half the scene went with it
    if n < 3:
        assert got["info"][0, 1] == -1 and removed == [0, 0]      # no triple of distinct rows


@pytest.mark.parametrize("H", [1, 7, 256, 1024])
def test_hypothesis_counts(cuda, H):
    n = 2 * CHUNK + 452
    pts, _ = R.scene(n, 41)
    for refine in (0, 1):
        P = R.params(H=H, refine=refine, seed=(7 << 32) | 5)      # both words of the seed are used
        got = _gpu(cuda, pts, [0, n], P, n)
        _same(got, _ref(("H", H, refine), pts, [0, n], P, n))
    if H >= 256:
        assert got["info"][0, 1] >= 0 and got["info"][0, 2] > n // 3 and got["info"][0, 3] > n // 3      # half the scene is road


def _ragged():
    """scans: a scene; one the crop empties (60 m away); all NaN; a scene in a tilted road; then, by the offsets, an empty one
    (broken), one longer than max_len (broken) and a short one"""
    a, _ = R.scene(1500, 51)
    far = a[:300] + np.array([60.0, 0.0, 0.0], dtype=np.float32)
    far = far[far[:, 0] > 25.0]
    nan = np.full((70, 3), np.nan, dtype=np.float32)
    nan[::3, 1] = np.inf
    b, _ = R.scene(CHUNK + 333, 52, (-0.06, 0.08))
    c, _ = R.scene(2000, 53)
    d, _ = R.scene(200, 54)
    pts = np.concatenate((a, far, nan, b, c, d), 0)
    lens = [len(a), len(far), len(nan), len(b), 0, len(c), len(d)]
    return pts, np.concatenate(([0], np.cumsum(lens))), lens


def test_ragged_batch_with_emptied_nan_and_broken_scans(cuda):
    pts, off, lens = _ragged()
    max_len = 1500      # the 2000-row scan is longer: not read
    P = R.params(H=128, r_max=25.0, seed=3)
    got = _gpu(cuda, pts, off, P, max_len)
    want = _ref("ragged", pts, off, P, max_len)
    _same(got, want)
    info = got["info"]
    assert info[1].tolist() == [0, -1, 0, 0] and info[2].tolist() == [0, -1, 0, 0]                  # emptied by the crop; all NaN
    assert info[4].tolist() == [-1, -1, 0, 0] and info[5].tolist() == [-1, -1, 0, 0]              # broken: empty, too long
    assert info[0, 1] >= 0 and info[3, 1] >= 0 and info[6, 0] > 0
    kept = np.diff(got["out_offsets"])
    assert kept[1] == kept[2] == kept[4] == kept[5] == 0 and kept[0] > 0 and kept[3] > 0
    assert not got["mask"][off[5]:off[6]].any()
    # offsets that start below zero or end behind the table: those scans are not read, their neighbours are
    for o, broken in (([-5, 10, 300], 0), ([0, 200, len(pts) + 5], 1), ([0, 300, 200, 900], 1)):
        g = _gpu(cuda, pts, o, P, max_len)
        _same(g, R.clean_batch(pts, o, P, max_len))
        assert g["info"][broken].tolist() == [-1, -1, 0, 0] and (g["info"][:, 0] >= 0).sum() == len(o) - 2


def test_row_stride_four_with_junk(cuda):
    n = CHUNK + 77
    pts, _ = R.scene(n, 61)
    four = np.full((n, 4), np.nan, dtype=np.float32)      # the fourth column is never read
    four[::2, 3] = 1e30
    four[:, :3] = pts
    P = R.params(H=32, seed=1)
    got = _gpu(cuda, four, [0, n], P, n)
    _same(got, _ref("ld4", pts, [0, n], P, n))
    assert got["out"].shape[1] == 3 and got["info"][0, 1] >= 0


def test_crop_that_removes_everything_and_crop_only(cuda):
    n = CHUNK + 5
    pts, _ = R.scene(n, 62)
    P = R.params(H=16, z_lo=100.0, z_hi=200.0)
    two = np.concatenate((pts, pts))
    got = _gpu(cuda, two, [0, n, 2 * n], P, n)
    _same(got, R.clean_batch(two, [0, n, 2 * n], P, n))
    assert got["out_offsets"].tolist() == [0, 0, 0] and got["info"].tolist() == [[0, -1, 0, 0]] * 2 and not got["mask"].any()
    P = R.params(H=0, r_min=5.0, r_max=30.0, z_hi=1.0)      # H = 0: no road step
    got = _gpu(cuda, pts, [0, n], P, n)
    _same(got, R.clean_batch(pts, [0, n], P, n))
    assert got["info"][0, 1:].tolist() == [-1, 0, 0] and 0 < got["out_offsets"][1] == got["info"][0, 0] < n


def test_no_road_scan(cuda):
    """wall only, and the seed band set so that no triple is valid: the road rule removes nothing, the crop still applies"""
    pts, lab = R.scene(4 * CHUNK, 63)
    wall = np.ascontiguousarray(pts[lab == 1])
    n = len(wall)
    P = R.params(H=64, seed_z_lo=100.0, seed_z_hi=200.0, z_hi=4.0)
    got = _gpu(cuda, wall, [0, n], P, n)
    _same(got, R.clean_batch(wall, [0, n], P, n))
    live = int((wall[:, 2] <= 4.0).sum())
    assert got["info"][0].tolist() == [live, -1, 0, 0] and got["out_offsets"][1] == live and 0 < live < n and not got["plane"].any()
    P = R.params(H=64, z_hi=4.0)      # without the band the wall offers no plane within the slope limit either, or too few inliers
    got = _gpu(cuda, wall, [0, n], P, n)
    _same(got, R.clean_batch(wall, [0, n], P, n))


def test_mask_does_not_depend_on_the_row_order(cuda):
    """for a GIVEN plane (the plane itself depends on the order by definition: the triples are drawn by row number)"""
    from lpdnet_hip import ops
    n = 2 * CHUNK + 99
    pts, _ = R.scene(n, 64, (0.03, 0.03))
    perm = np.random.default_rng(64).permutation(n)
    prm = _removal(R.params(H=64, r_max=40.0)).c_params()
    a = torch.from_numpy(pts.copy()).to(cuda)
    b = torch.from_numpy(np.ascontiguousarray(pts[perm])).to(cuda)
    off = torch.tensor([0, n], dtype=torch.int32, device=cuda)
    plane, info = ops.road_planes(a, off, 1, n, prm)
    out_a, off_a, mask_a = ops.clean_scans(a, off, 1, n, prm, plane, info, want_mask=True)
    out_b, off_b, mask_b = ops.clean_scans(b, off, 1, n, prm, plane, info, want_mask=True)
    assert int(info[0, 1]) >= 0 and torch.equal(off_a, off_b) and 0 < int(off_a[1]) < n
    ma, mb = mask_a.cpu().numpy().astype(bool), mask_b.cpu().numpy().astype(bool)
    assert np.array_equal(ma[perm], mb)
    assert np.array_equal(out_b[:int(off_b[1])].cpu().numpy(), pts[perm][mb])      # stable: the permuted order is kept


def test_argument_errors_launch_nothing(cuda):
    from lpdnet_hip import LpdHipError, _lib, ops, submap
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    pts = torch.zeros((64, 3), device=cuda)
    off = torch.tensor([0, 64], dtype=torch.int32, device=cuda)
    plane = torch.full((1, 4), 7.0, device=cuda)
    info = torch.full((1, 4), 7, dtype=torch.int32, device=cuda)
    counts = torch.full((1,), 7, dtype=torch.int32, device=cuda)
    boff = torch.zeros((2,), dtype=torch.int32, device=cuda)
    out = torch.full((64, 3), 7.0, device=cuda)
    ooff = torch.full((2,), 7, dtype=torch.int32, device=cuda)
    ws = torch.zeros((int(lib.lpd_road_planes_workspace_bytes(1, 1024)),), dtype=torch.uint8, device=cuda)
    assert ws.numel() >= 1024 * 20 and lib.lpd_road_planes_workspace_bytes(0, 4) == 0 and lib.lpd_road_planes_workspace_bytes(1, 1025) == 0

    def calls(prm, ld=3, rows=64, B=1, max_len=64, points=True, offsets=True):
        head = (p(pts) if points else None, ld, rows, p(off) if offsets else None, B, max_len, ctypes.byref(prm) if prm is not None else None)
        return [("lpd_road_planes", lib.lpd_road_planes(*head, p(plane), p(info), p(ws), None), lib.lpd_last_error().decode()),
                ("lpd_clean_count", lib.lpd_clean_count(*head, p(plane), p(info), p(counts), None), lib.lpd_last_error().decode()),
                ("lpd_clean_fill", lib.lpd_clean_fill(*head, p(plane), p(info), p(boff), p(out), p(ooff), None, None), lib.lpd_last_error().decode())]

    def prm(**kw):
        c = submap.RoadRemoval().c_params()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    nan, inf = float("nan"), float("inf")
    bad_prm = [dict(r_max=512.5), dict(r_min=-1.0), dict(r_min=30.0, r_max=20.0), dict(r_max=nan), dict(r_min=nan), dict(H=1025), dict(H=-1),
               dict(tau=-0.1), dict(tau=inf), dict(tau=nan), dict(min_det=-1.0), dict(min_det=nan), dict(max_slope=-0.1), dict(max_slope=inf),
               dict(clearance=nan), dict(clearance=inf), dict(min_inliers=-1), dict(refine=2), dict(z_lo=nan), dict(z_hi=nan), dict(seed_z_lo=nan),
               dict(seed_z_hi=nan)]
    for kw in bad_prm:
        for name, rc, msg in calls(prm(**kw)):
            assert rc == -1 and msg.startswith(name + ":"), (kw, name, rc, msg)
    for kw in (dict(ld=2), dict(rows=0), dict(rows=-4), dict(B=0), dict(B=65536), dict(max_len=0), dict(max_len=(1 << 20) + 1), dict(points=False),
               dict(offsets=False)):
        for name, rc, msg in calls(prm(), **kw):
            assert rc == -1 and msg.startswith(name + ":"), (kw, name, rc, msg)
    for name, rc, msg in calls(None):
        assert rc == -1 and msg.startswith(name + ":")
    good = prm()
    head = (p(pts), 3, 64, p(off), 1, 64, ctypes.byref(good))
    assert lib.lpd_road_planes(*head, None, p(info), p(ws), None) == -1 and lib.lpd_road_planes(*head, p(plane), p(info), None, None) == -1
    assert lib.lpd_clean_count(*head, p(plane), None, p(counts), None) == -1 and lib.lpd_clean_count(*head, None, None, None, None) == -1
    assert lib.lpd_clean_fill(*head, None, None, None, p(out), p(ooff), None, None) == -1
    assert lib.lpd_clean_fill(*head, None, None, p(boff), p(pts), p(ooff), None, None) == -1      # out must not alias points
    torch.cuda.synchronize()
    assert (plane == 7).all() and (info == 7).all() and (counts == 7).all() and (out == 7).all() and (ooff == 7).all()      # nothing ran
    # the wrappers
    c = submap.RoadRemoval().c_params()
    for call in (lambda: ops.road_planes(pts, off, 2, 64, c), lambda: ops.road_planes(pts, off, 1, 0, c), lambda: ops.road_planes(pts[:, :2], off, 1, 64, c),
                 lambda: ops.clean_scans(pts, off, 1, 64, c, plane, None), lambda: ops.clean_scans(pts, off, 1, 64, c, plane[:, :3], info),
                 lambda: ops.road_planes(pts, off, 1, (1 << 20) + 1, c)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.road_planes(pts, off.long(), 1, 64, c)
    with pytest.raises(TypeError):
        ops.road_planes(pts, off, 1, 64, submap.RoadRemoval())
    with pytest.raises(LpdHipError):
        ops.clean_scans(pts.cpu(), off, 1, 64, c)
    # a block_off that is not the scan of the counts writes nothing outside out
    wrong = torch.tensor([60, 64], dtype=torch.int32, device=cuda)
    small = torch.full((70, 3), 7.0, device=cuda)
    one = torch.ones((64, 3), device=cuda)
    crop = prm(H=0)
    assert lib.lpd_clean_fill(p(one), 3, 64, p(off), 1, 64, ctypes.byref(crop), None, None, p(wrong), p(small), p(ooff), None, None) == 0
    torch.cuda.synchronize()
    assert (small[:60] == 7).all() and (small[60:64] == 1).all() and (small[64:] == 7).all() and ooff.tolist() == [60, 64]


@pytest.fixture(scope="module")
def model(cuda):
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad
    m = PointNetVlad(num_points=1024, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=1024), strict=True)
    return m.to(cuda).eval()


LENS = [3000, 5000, 1500]


def _scans():
    scans = [np.array(R.scene(n, 70 + i, (0.02 * i, -0.01))[0]) for i, n in enumerate(LENS)]
    scans[1][17] = np.nan      # rows that are not finite are dropped, not rejected
    scans[1][4000, 2] = np.inf
    return scans


def test_make_submaps_with_clean_and_scan_input(cuda, model):
    """make_submaps(clean=...) = make_submaps on the restatement's kept rows, exactly; an emptied scan is the zero submap"""
    from lpdnet_hip import submap
    scans = _scans()
    clean = submap.RoadRemoval(r_max=45.0, H=128, seed=9)
    P = R.params(r_max=45.0, H=128, seed=9)
    cat = np.concatenate(scans, 0)
    want = _ref("submaps", cat, np.concatenate(([0], np.cumsum(LENS))), P, max(LENS))
    kept = [want["out"][want["out_offsets"][b]:want["out_offsets"][b + 1]] for b in range(3)]
    sub = submap.make_submaps(scans, num_points=1024, clean=clean, want_counts=True)
    ref = submap.make_submaps(kept, num_points=1024, want_counts=True)
    assert sub.x.shape == (3, 1, 1024, 3) and torch.equal(sub.x, ref.x) and torch.equal(sub.counts, ref.counts)
    assert torch.equal(sub.level, ref.level) and torch.equal(sub.cells, ref.cells) and sub.n_raw.tolist() == [len(k) for k in kept]
    assert ref.cleaned is None and isinstance(sub.cleaned, submap.CleanedScans) and sub.cleaned.mask is None
    assert sub.cleaned.lengths() == [len(k) for k in kept] and np.array_equal(sub.cleaned.info.cpu().numpy(), want["info"])
    assert np.array_equal(sub.cleaned.plane.cpu().numpy().view(np.uint32), want["plane"].view(np.uint32)) and (want["info"][:, 1] >= 0).all()
    with pytest.raises(ValueError):
        submap.make_submaps(scans, num_points=1024)      # without clean= the NaN row is rejected by check_finite
    # clean_scans alone, with the mask; a concatenated tensor with lengths; ld = 4
    four = np.concatenate((cat, np.full((len(cat), 1), np.nan, dtype=np.float32)), 1)
    res = submap.clean_scans(torch.from_numpy(four).to(cuda), LENS, clean, want_mask=True)
    assert np.array_equal(res.mask.cpu().numpy(), want["mask"]) and np.array_equal(res.offsets.cpu().numpy(), want["out_offsets"])
    assert np.array_equal(res.points[:int(res.offsets[-1])].cpu().numpy(), want["out"]) and res.lengths() == [len(k) for k in kept]
    # a scan that the cleaning empties: the zero submap, marked
    empty = submap.make_submaps([scans[0], scans[2] + np.array([100.0, 0, 0], dtype=np.float32)], num_points=1024, clean=clean)
    assert empty.level.tolist()[1] == -1 and empty.cells.tolist()[1] == 0 and empty.n_raw.tolist()[1] == 0 and not empty.x[1].any()
    assert torch.equal(empty.x[0], sub.x[0]) and empty.cleaned.info[1].tolist() == [0, -1, 0, 0]
    with torch.no_grad():
        direct = model(sub.x)
        wrapped = submap.ScanInput(model, num_points=1024, clean=clean)(scans)
        plain = submap.ScanInput(model, num_points=1024)(scans[:1])
    assert torch.equal(direct, wrapped) and torch.isfinite(direct).all() and direct.shape == (3, 256)
    assert (plain[0] - wrapped[0]).abs().max() > 1e-3      # the road is gone: another descriptor


def test_scan_stream_with_clean(cuda, model, tmp_path):
    from lpdnet_hip import ingest, submap
    scans = _scans()
    names = []
    for i, s in enumerate(scans):
        a = np.full((len(s), 4), 55.0, dtype=np.float32)
        a[:, :3] = s
        names.append(f"s{i}.bin")
        a.tofile(tmp_path / names[-1])
    clean = submap.RoadRemoval(r_max=45.0, H=128, seed=9)
    got = ingest.get_latent_vectors_from_scans(model, names, 2, str(tmp_path), num_points=1024, dtype=np.float32, columns=4, clean=clean)
    with torch.no_grad():
        want = [model(submap.make_submaps(scans[i:i + 2], num_points=1024, clean=clean).x).cpu().numpy() for i in (0, 2)]
    assert got.shape == (3, 256) and np.isfinite(got).all() and np.array_equal(got, np.concatenate(want, 0))
    stream = ingest.ScanStream(names, 3, str(tmp_path), cuda, 1024, np.float32, 4, clean=clean)
    batches = list(stream)
    assert len(batches) == 1 and batches[0].shape == (3, 1, 1024, 3) and stream.last.cleaned is not None
    assert (stream.last.cleaned.info[:, 1] >= 0).all()


def test_planes_against_the_generating_plane(cuda):
    """MEASURE lines: the distance of the device's plane to the plane the scene was made with (the assertion is the exact equality
    with the restatement above; the conditions on the restatement are tests/test_clean_cpu.py's)"""
    from lpdnet_hip import submap
    for n, tilt in ((5000, (0.0, 0.0)), (5000, (0.05, -0.03)), (3 * CHUNK + 17, (0.05, -0.03))):
        pts, lab = R.scene(n, 11, tilt)
        res = submap.clean_scans([pts], clean=submap.RoadRemoval(), want_mask=True)
        a, b, c, _ = res.plane[0].tolist()
        kept = res.mask.cpu().numpy().astype(bool)
        high = R.height_above_road(pts, tilt) > 0.5
        print(f"MEASURE clean/gpu/n{n}/tilt{tilt[0]:g} slope error {np.hypot(a - tilt[0], b - tilt[1]):.2e} offset error {abs(c - R.ROAD_Z) * 1e3:.2f} mm "
              f"road removed {1 - kept[lab == 0].mean():.4f} high removed {1 - kept[high].mean():.4f} info {res.info[0].tolist()}")
        want = R.clean_batch(pts, [0, n], R.params(), n)
        assert np.array_equal(res.plane.cpu().numpy().view(np.uint32), want["plane"].view(np.uint32)) and np.array_equal(kept, want["mask"].astype(bool))
