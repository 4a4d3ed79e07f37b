"""lpd_make_submaps on the GPU against tests/submap_ref.py: (a) the numpy restatement of the definition -- info and counts exact,
values within one fp32 rounding -- and (b) an independent fp64 grid average; order independence, repeatability, row stride,
argument errors, and the way from raw scans to descriptors (submap.make_submaps, submap.ScanInput, ingest.ScanStream).

Gates (derived, not tuned): cell rows 2^-22 * (max|mn| + E) per coordinate against (a) -- the only operation whose rounding may
differ from numpy's is the division; normalised output 2^-22 absolute; xform 2^-22 relative per component; against (b)
2^-20 * E + 4 * 2^-24 * max|x|: the half-step quantisation plus fp32 rounding.  Fill rows are bit-equal to the raw points.

The entry point takes no workspace (the 64-bit sums fit in LDS), so there is no "workspace too small" error to test.  N < 128 is
an argument error (-1); N > 4096 is outside the kernel's scope and returns LPD_ERR_UNSUPPORTED (-3), as include/lpd_hip.h says.
"Unit norm" of a descriptor is asserted on the NetVLAD head's L2-normalised vector (test_a_finished_submap_goes_through says why).

Measured on an MI355X (MEASURE lines of this file): see DESIGN.md section 13c."""
import ctypes
import os

import numpy as np
import pytest
import torch

import submap_ref as R

pytestmark = pytest.mark.gpu

# name -> (clouds as (generator name, n), N)
LAUNCHES = {
    "ragged": ((("scan", 300), ("scan", 1), ("scan", 129), ("scan", 5000)), 128),
    "short": ((("scan", 100),), 128),
    "rung0": ((("scan", 4097),), 4096),
    "trips": ((("scan", 20000),), 1024),
    "odd": ((("scan", 70001),), 4096),
    "lattice": ((("lattice", 0),), 1024),
    "degenerate": ((("identical", 0), ("plane", 0), ("two_points", 0), ("translated", 0)), 128),
}
_GOT = {}


def _launch(clouds, N, normalize, ld=3, dev="cuda:0"):
    from lpdnet_hip import ops
    pts = np.concatenate(clouds, 0)
    if ld > 3:
        wide = np.full((pts.shape[0], ld), -12345.0, dtype=np.float32)      # junk behind the coordinates
        wide[:, :3] = pts
        pts = wide
    off = np.zeros(len(clouds) + 1, dtype=np.int32)
    np.cumsum([c.shape[0] for c in clouds], out=off[1:])
    out, info, xform, counts = ops.make_submaps(torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), len(clouds), N, normalize,
                                                want_counts=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy(), xform.cpu().numpy(), counts.cpu().numpy()


def _got(name, normalize):
    """one launch per (case, normalize) for the whole module"""
    key = (name, normalize)
    if key not in _GOT:
        spec, N = LAUNCHES[name]
        _GOT[key] = _launch([R.cloud(g, n) for g, n in spec], N, normalize)
    return _GOT[key]


def _ref(name, b, normalize):
    spec, N = LAUNCHES[name]
    g, n = spec[b]
    return R.cached_submap(g, n, N, normalize)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_discrete_parity_is_exact(cuda, name):
    spec, N = LAUNCHES[name]
    for normalize in (False, True):
        out, info, xform, counts = _got(name, normalize)
        for b in range(len(spec)):
            ref = _ref(name, b, normalize)
            assert tuple(info[b]) == ref["info"], (name, b, info[b], ref["info"])
            assert np.array_equal(counts[b], ref["counts"]), (name, b)
            assert np.isfinite(out[b]).all() and np.isfinite(xform[b]).all()


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_values_against_the_restatement(cuda, name):
    spec, N = LAUNCHES[name]
    raw, _, xf0, _ = _got(name, False)
    nrm, _, xf1, _ = _got(name, True)
    worst = [0.0, 0.0, 0.0]
    for b, (g, n) in enumerate(spec):
        x = R.cloud(g, n)
        ref0, ref1 = _ref(name, b, False), _ref(name, b, True)
        M = ref0["info"][1]
        assert np.array_equal(raw[b][M:], x[ref0["fill"]]), (name, b)            # fill rows: the raw points' bits
        gate = 2.0 ** -22 * (float(np.abs(ref0["mn"]).max()) + float(ref0["E"]))
        err = float(np.abs(raw[b][:M].astype(np.float64) - ref0["rows"][:M]).max())
        worst[0] = max(worst[0], err / gate if gate > 0 else err)
        assert err <= gate, (name, b, err, gate)
        assert xf0[b].tolist() == [0.0, 0.0, 0.0, 1.0]
        err1 = float(np.abs(nrm[b].astype(np.float64) - ref1["out"]).max())
        worst[1] = max(worst[1], err1)
        assert err1 <= 2.0 ** -22, (name, b, err1)
        d = np.abs(xf1[b].astype(np.float64) - ref1["xform"])
        rel = float((d / np.maximum(np.abs(ref1["xform"].astype(np.float64)), 1e-300)).max()) if d.max() > 0 else 0.0
        worst[2] = max(worst[2], rel)
        assert (d <= 2.0 ** -22 * np.abs(ref1["xform"])).all(), (name, b, xf1[b], ref1["xform"])
        top = float(np.abs(nrm[b]).max())      # r * fl(1 / r) is 1 or the float below it
        assert (1.0 - 2.0 ** -23 <= top <= 1.0) if ref1["xform"][3] > 0 else top == 0.0
    print(f"MEASURE submap {name}: cell rows vs (a) {worst[0]:.3g} of the gate, normalised out {worst[1]:.3g} (gate {2.0 ** -22:.3g}), "
          f"xform rel {worst[2]:.3g} (gate {2.0 ** -22:.3g})")


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_values_against_the_fp64_grid_average(cuda, name):
    spec, N = LAUNCHES[name]
    raw, info, _, counts = _got(name, False)
    worst = 0.0
    for b, (g, n) in enumerate(spec):
        x = R.cloud(g, n)
        j, M = int(info[b][0]), int(info[b][1])
        means = R.cell_means_fp64(x, j)                                            # on the GPU's own j*
        assert means.shape[0] == M
        _, E = R.box(x)
        gate = 2.0 ** -20 * float(E) + 4 * 2.0 ** -24 * float(np.abs(x).max())
        err = float(np.abs(raw[b][:M].astype(np.float64) - means).max())          # every cell row
        worst = max(worst, err / gate)
        assert err <= gate, (name, b, err, gate)
    print(f"MEASURE submap {name}: cell rows vs fp64 grid average {worst:.3g} of the gate")


def test_order_independence(cuda):
    x = R.scan(20000)
    a = _got("trips", False)
    b = _launch([x[np.random.default_rng(11).permutation(x.shape[0])]], 1024, False)
    M = int(a[1][0][1])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and np.array_equal(a[0][0][:M], b[0][0][:M])
    small = [R.scan(300), R.scan(5000)]
    rng = np.random.default_rng(12)
    c, d = _launch(small, 128, False), _launch([s[rng.permutation(s.shape[0])] for s in small], 128, False)
    for i in range(2):
        M = int(c[1][i][1])
        assert np.array_equal(c[1][i], d[1][i]) and np.array_equal(c[3][i], d[3][i]) and np.array_equal(c[0][i][:M], d[0][i][:M])


def test_repeatability_and_row_stride(cuda):
    clouds = [R.scan(5000), R.scan(129), R.lattice()[:9000]]
    a, b = _launch(clouds, 256, True), _launch(clouds, 256, True)
    wide = _launch(clouds, 256, True, ld=4)
    for u, v, w in zip(a, b, wide):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    assert np.array_equal(_launch(clouds, 256, False)[0], _launch(clouds, 256, False, ld=5)[0])


def test_argument_errors_launch_nothing(cuda):
    from lpdnet_hip import LpdHipError, _lib, ops
    lib = _lib.load()
    pts = torch.from_numpy(R.scan(300)).to(cuda)
    off = torch.tensor([0, 300], dtype=torch.int32, device=cuda)
    out = torch.full((1, 128, 3), 7.0, device=cuda)
    info = torch.full((1, 4), 7, dtype=torch.int32, device=cuda)
    xform = torch.full((1, 4), 7.0, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    good = [p(pts), 3, p(off), 1, 128, 1, p(out), p(info), p(xform), None, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[{"points": 0, "ld": 1, "offsets": 2, "B": 3, "N": 4, "normalize": 5, "out": 6, "info": 7, "xform": 8}[k]] = v
        rc = lib.lpd_make_submaps(*a)
        return rc, lib.lpd_last_error().decode()

    for kw in (dict(points=None), dict(offsets=None), dict(out=None), dict(info=None), dict(xform=None), dict(N=127), dict(N=0),
               dict(N=-4096), dict(ld=2), dict(B=0), dict(normalize=2), dict(out=p(pts))):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("lpd_make_submaps:"), (kw, rc, msg)
    rc, msg = call(N=4097)
    assert rc == -3 and msg.startswith("lpd_make_submaps:"), (rc, msg)
    torch.cuda.synchronize()
    assert (out == 7).all() and (info == 7).all() and (xform == 7).all()          # nothing was launched
    # offsets are checked by the wrapper, on the host
    for bad in ([300, 0], [0, 0], [-1, 299], [0, 301]):
        with pytest.raises(ValueError):
            ops.make_submaps(pts, torch.tensor(bad, dtype=torch.int32, device=cuda), 1, 128)
    with pytest.raises(ValueError):
        ops.make_submaps(pts, torch.tensor([0, 100, 50, 300], dtype=torch.int32, device=cuda), 3, 128)      # decreasing
    with pytest.raises(ValueError):
        ops.make_submaps(pts, off, 1, 100)
    with pytest.raises(ValueError):
        ops.make_submaps(pts[:, :2], off, 1, 128)
    with pytest.raises(TypeError):
        ops.make_submaps(pts, off.long(), 1, 128)
    with pytest.raises(LpdHipError):
        ops.make_submaps(pts.cpu(), off, 1, 128)
    # a raw caller's empty / reversed cloud is marked and zeroed by the kernel, its points are not read; its neighbour is unharmed
    off3 = torch.tensor([0, 300, 300, 200], dtype=torch.int32, device=cuda)
    out3 = torch.full((3, 128, 3), 7.0, device=cuda)
    info3 = torch.full((3, 4), 7, dtype=torch.int32, device=cuda)
    xf3 = torch.full((3, 4), 7.0, device=cuda)
    assert lib.lpd_make_submaps(p(pts), 3, p(off3), 3, 128, 1, p(out3), p(info3), p(xf3), None, None) == 0
    torch.cuda.synchronize()
    ref = R.cached_submap("scan", 300, 128, True)
    assert info3.cpu().tolist() == [list(ref["info"]), [-1, 0, 0, 0], [-1, 0, 0, 0]]
    assert (out3[1:] == 0).all() and (xf3[1:] == 0).all() and np.abs(out3[0].cpu().numpy() - ref["out"]).max() <= 2.0 ** -22


# ---- from raw scans to descriptors, N = 1024 -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(cuda):
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad
    m = PointNetVlad(num_points=1024, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=1024), strict=True)
    return m.to(cuda).eval()


def test_public_make_submaps_and_scan_input(cuda, model):
    from lpdnet_hip import submap
    scans = [R.scan(3000, 1), R.scan(5000), R.scan(1500, 2)]
    sub = submap.make_submaps(scans, num_points=1024, want_counts=True)
    assert sub.x.shape == (3, 1, 1024, 3) and sub.x.is_cuda and sub.x.dtype == torch.float32
    for b, (n, seed) in enumerate(((3000, 1), (5000, 0), (1500, 2))):
        ref = R.submap(scans[b], 1024)
        assert (int(sub.level[b]), int(sub.cells[b]), int(sub.n_raw[b])) == ref["info"][:3]
        assert np.array_equal(sub.counts[b].cpu().numpy(), ref["counts"])
        assert np.abs(sub.x[b, 0].cpu().numpy() - ref["out"]).max() <= 2.0 ** -22
        back = sub.restore()[b].cpu().numpy()
        assert np.abs(back - ref["rows"]).max() <= 4 * 2.0 ** -24 * (np.abs(ref["rows"]).max() + ref["xform"][3])
    cat = torch.from_numpy(np.concatenate(scans, 0)).to(cuda)
    again = submap.make_submaps(cat, [3000, 5000, 1500], num_points=1024)
    assert torch.equal(again.x, sub.x)
    from lpdnet_hip import ops
    buf = torch.full((3, 1, 1024, 3), 9.0, device=cuda)
    off = torch.tensor([0, 3000, 8000, 9500], dtype=torch.int32, device=cuda)
    res = ops.make_submaps(cat, off, 3, 1024, out=buf)
    assert res[0] is buf and res[3] is None and torch.equal(buf, sub.x) and torch.equal(res[1][:, 1], sub.cells)
    with pytest.raises(ValueError):
        ops.make_submaps(cat, off, 3, 1024, out=buf[:2])
    f64 = submap.make_submaps([s.astype(np.float64) for s in scans], num_points=1024)      # narrowed on the device: the same floats
    assert torch.equal(f64.x, sub.x)
    pts, lens = submap.filter_scans(cat, [3000, 5000, 1500], cat[:, 2] > -1.6)
    cut = submap.make_submaps(pts, lens, num_points=1024)
    assert cut.x.shape == (3, 1, 1024, 3) and cut.n_raw.cpu().tolist() == lens and sum(lens) < 9500
    with torch.no_grad():
        direct = model(sub.x)
        wrapped = submap.ScanInput(model, num_points=1024)(scans)
        wrapped2 = submap.ScanInput(model, num_points=1024)(cat, [3000, 5000, 1500])
    assert torch.equal(direct, wrapped) and torch.equal(direct, wrapped2) and torch.isfinite(direct).all()


@pytest.mark.parametrize("dtype,columns", [(np.float64, 3), (np.float32, 4)])
def test_get_latent_vectors_from_scans(cuda, model, tmp_path, dtype, columns):
    from lpdnet_hip import ingest, submap
    lengths = [2500, 1300, 4000, 1024, 3100]
    names, scans = [], []
    for i, n in enumerate(lengths):
        a = np.full((n, columns), 55.0, dtype=dtype)
        a[:, :3] = R.scan(n, 20 + i)
        names.append(f"s{i}.bin")
        a.tofile(tmp_path / names[-1])
        scans.append(a)
    (tmp_path / "broken.bin").write_bytes(b"\1" * (columns * np.dtype(dtype).itemsize * 3 + 1))
    files = names[:3] + ["broken.bin"] + names[3:]
    was = model.training
    got = ingest.get_latent_vectors_from_scans(model, files, 2, str(tmp_path), num_points=1024, dtype=dtype, columns=columns)
    assert model.training == was and got.shape == (5, 256) and got.dtype == np.float32
    with torch.no_grad():
        want = [model(submap.make_submaps(scans[i:i + 2], num_points=1024).x).cpu().numpy() for i in (0, 2, 4)]
    assert np.array_equal(got, np.concatenate(want, 0))
    model.train()
    try:
        ingest.get_latent_vectors_from_scans(model, files[:1], 2, str(tmp_path), num_points=1024, dtype=dtype, columns=columns)
        assert model.training                                                       # the caller's mode is restored
    finally:
        model.eval()
    assert ingest.get_latent_vectors_from_scans(model, ["broken.bin"], 2, str(tmp_path), num_points=1024, dtype=dtype, columns=columns).shape == (0, 256)


def _finished_submap(cuda):
    from oracle import synth
    from lpdnet_hip import submap
    x = synth.cloud(7, 1, 1024)[0]
    x = x - x.mean(0, keepdims=True).astype(np.float32)
    return submap.make_submaps([x], num_points=1024)


def test_a_finished_submap_goes_through(cuda, model, monkeypatch):
    """A cloud that already is a 1024-point submap goes through unharmed in shape: rung 0, every point its own row or a fill row,
    the shape of a model input.  Its descriptor is finite and has unit norm to the head's tolerance: the NetVLAD head's descriptor,
    the L2-normalised [E * 64] vector that lpd_vlad_finalize writes (|norm - 1| < 1e-6, the bound tests/test_fwd_ops_gpu.py holds that
    kernel to), is the quantity of the model that HAS a norm by construction -- it comes out 0 or NaN for a degenerate or non-finite
    cloud.  The 256 numbers behind the hidden projection, BatchNorm and context gating (reference PointNetVlad.py:75-83) are not
    normalised by anything (norm 0.5398 for this cloud with the synthetic weights, printed below); they must be finite and must be
    the bits of the plain forward."""
    from lpdnet_hip import engine, ops
    sub = _finished_submap(cuda)
    assert sub.x.shape == (1, 1, 1024, 3) and int(sub.n_raw[0]) == 1024 and int(sub.level[0]) == 0
    assert 1.0 - 2.0 ** -23 <= float(sub.x.abs().max()) <= 1.0
    seen = []
    real = ops.vlad_finalize

    def recording(*a, **kw):
        out = real(*a, **kw)
        seen.append(out)
        return out

    monkeypatch.setattr(ops, "vlad_finalize", recording)
    engine.DEBUG_AUX = {}                      # the test hook: the forward runs call by call, not from a recorded launch list
    try:
        with torch.no_grad():
            d = model(sub.x)
    finally:
        engine.DEBUG_AUX = None
        monkeypatch.undo()
    with torch.no_grad():
        plain = model(sub.x)
    assert d.shape == (1, 256) and torch.isfinite(d).all() and torch.equal(d, plain)
    assert len(seen) == 1 and seen[0].shape == (1, 1024 * 64) and torch.isfinite(seen[0]).all()
    vnorm = float(seen[0].double().norm(dim=1)[0])
    print(f"MEASURE submap finished-submap: NetVLAD descriptor norm {vnorm:.9f} (gate 1e-6 around 1), "
          f"256-d output norm {float(d.double().norm(dim=1)[0]):.8f} (not normalised by the model), finite True")
    assert abs(vnorm - 1.0) < 1e-6, vnorm
