"""CPU side of the motion compensation of LiDAR sweeps (lpd_scan_deskew, lpd_drive_motions, lpd_odom_motion,
lpdnet_hip/odometry.py): the kernels' arithmetic header (csrc/lpd_deskew_math.h) compiled by the host C++ compiler and compared with
the numpy restatement (tests/deskew_ref.py) value for value and with lpd_map_blend(identity, motion, a) bit for bit, hand-made motions
against written-down answers, the quality conditions of the design on deskew_cases.skewed_drive, and the host side of the wrappers.  The
kernels are tested on the GPU (tests/test_deskew_gpu.py)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import deskew_cases as C
import deskew_ref as D
import icp_ref as I
import loc_cases as LC
import map_ref as M
import odom_cases as OC
import odom_ref as O
from lpdnet_hip import odometry, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32, f64, i64 = np.float32, np.float64, np.int64

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_deskew_math.h"
// <mode> <in> <out> <n>: float64 in, float64 out (fp32 values and integers as float64)
//   row     motion 12, time, ref, x, y, z          -> done, o 3, lpd_deskew_pose 12, lpd_map_blend(identity, motion, a) 12
//   scan    motion 12                              -> dq 4, dt 3, ok
//   drive   S, i, poses 3 x 12                     -> motion 12
//   odom    t, has first_motion, first_motion 12, poses 4 x 12 -> motion 12
int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    size_t rin = 0, rout = 0;
    if (!strcmp(mode, "row")) { rin = 17; rout = 28; }
    else if (!strcmp(mode, "scan")) { rin = 12; rout = 8; }
    else if (!strcmp(mode, "drive")) { rin = 38; rout = 12; }
    else if (!strcmp(mode, "odom")) { rin = 62; rout = 12; }
    else return 2;
    std::vector<double> in(n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 8, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t k = 0; k < n; ++k) {
        const double* r = &in[k * rin];
        double* o = &out[k * rout];
        if (!strcmp(mode, "row")) {
            const LpdDeskewScan s = lpd_deskew_scan(r);
            float w[3];
            o[0] = (double)lpd_deskew_row(s, (float)r[12], r[13], (float)r[14], (float)r[15], (float)r[16], w);
            for (int c = 0; c < 3; ++c) o[1 + c] = (double)w[c];
            const double a = (double)(float)r[12] - r[13];
            double id[12];
            lpd_deskew_identity(id);
            lpd_deskew_pose(s, a, o + 4);
            lpd_map_blend(id, r, a, o + 16);
        } else if (!strcmp(mode, "scan")) {
            const LpdDeskewScan s = lpd_deskew_scan(r);
            for (int c = 0; c < 4; ++c) o[c] = s.dq[c];
            for (int c = 0; c < 3; ++c) o[4 + c] = s.dt[c];
            o[7] = (double)s.ok;
        } else if (!strcmp(mode, "drive")) {
            lpd_deskew_drive_motion(r + 2, (int)r[0], (int)r[1], o);
        } else {
            lpd_deskew_odom_motion(r + 14, (int)r[0], r[1] != 0.0 ? r + 2 : nullptr, o);
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo || fwrite(out.data(), 8, out.size(), fo) != out.size()) return 4;
    fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("deskew_math")
    src = d / "deskew_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "deskew_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, records, n_out):
        records = np.ascontiguousarray(records, dtype=f64)
        records.tofile(d / "in.bin")
        r = subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(records.shape[0])], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        return np.fromfile(d / "out.bin", dtype=f64).reshape(records.shape[0], n_out)
    return run


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=f64), np.ascontiguousarray(want, dtype=f64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def _row_records(pts, lengths, times, motions, ref):
    scan = np.repeat(np.arange(len(lengths)), lengths)
    n = int(np.sum(lengths))
    return np.concatenate((motions[scan], times[:n, None].astype(f64), np.full((n, 1), ref), pts[:n].astype(f64)), axis=1), scan


def _tables():
    out = [("boundary",) + C.boundary_table(), ("random",) + C.random_table(5, [700, 1, 500, 300])]
    d = _drive("1m2deg", 1)
    out.append(("a skewed drive", d["points"][:3000], np.array([3000]), d["times"][:3000], d["motions"][:1]))
    return out


# ---- the header against the restatement and against lpd_map_blend ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [0.5, 0.0, 1.0, 0.3])
def test_rows_equal_the_restatement_and_the_blend_in_every_bit(host, ref):
    for name, pts, lengths, times, motions in _tables():
        rec, scan = _row_records(pts, lengths, times, motions, ref)
        got = host("row", rec, 28)
        n = len(rec)
        want, ok = D.rows(pts[:n], times[:n], motions[scan], ref)
        assert np.array_equal(got[:, 0], ok.astype(f64)), name
        assert got[:, 1:4].astype(f32).tobytes() == want.tobytes(), (name, np.argwhere(got[:, 1:4].astype(f32).view(np.uint32) != want.view(np.uint32))[:4])
        fin = np.isfinite(motions[scan]).all(axis=1)      # the blend of a motion that is not finite is not defined beyond "not used"
        _same(got[fin, 4:16], got[fin, 16:28], name + ": the per-scan / per-row split is lpd_map_blend(identity, motion, a)")
        with np.errstate(all="ignore"):
            a = times[:n].astype(f64) - f64(ref)
            _same(got[fin, 4:16], D.row_pose(motions[scan][fin], a[fin]), name + ": the restatement's blended pose")
        assert ok.sum() > 0 and (name != "boundary" or (~ok).sum() > 0)


def test_scan_part_equals_the_restatement(host):
    motions = np.concatenate([m for _, _, _, _, m in _tables()])
    got = host("scan", motions, 8)
    dq, dt, ok = D.scan_part(motions)
    fin = np.isfinite(motions).all(axis=1)
    assert np.array_equal(got[:, 7], ok.astype(f64)) and np.array_equal(ok, fin) and (~fin).sum() == 2
    _same(got[fin, :4], dq[fin], "dq")
    _same(got[fin, 4:7], dt[fin], "dt")
    assert (got[fin, 0] + 1.0 >= 0.0).all()      # the sign is chosen against the identity's quaternion: q_w >= 0
    _same(got[0, :7], np.zeros(7), "the identity's part is zero")


def test_the_two_motion_rules(host):
    rng = np.random.default_rng(12)
    P = np.array([LC.pose12(I.rot_xyz(*rng.uniform(-0.3, 0.3, 3)), [500000.0 + 1.3 * k, 5.7e6 + 0.7 * k * k, 120.0 + 0.01 * k]) for k in range(4)])
    bad = P.copy()
    bad[1, 7] = np.nan
    rec, want = [], []
    for poses in (P[:3], bad[:3]):
        for i in range(3):
            rec.append(np.concatenate(([3, i], poses.reshape(36))))
            want.append(D.drive_motions(poses)[i])
    rec.append(np.concatenate(([1, 0], P[:3].reshape(36))))
    want.append(D.drive_motions(P[:1])[0])
    rec.append(np.concatenate(([2, 1], P[:3].reshape(36))))
    want.append(D.drive_motions(P[:2])[1])
    got = host("drive", np.array(rec), 12)
    _same(got, np.array(want), "lpd_deskew_drive_motion")
    _same(got[2], got[1], "the last scan repeats the motion before it")
    _same(got[6], O.IDENTITY, "one scan alone: the identity")
    _same(got[7], got[0], "two scans: both get the one motion there is")
    assert not np.isfinite(got[3]).all() and not np.isfinite(got[4]).all() and not np.isfinite(got[5]).all()      # pose 1 is in every pair of S = 3
    e = I.pose_error(M.compose(P[0:1], np.ascontiguousarray(got[0:1, M.ROT]), np.ascontiguousarray(got[0:1, M.TRA]))[0], P[1].reshape(3, 4)[:, :3], P[1].reshape(3, 4)[:, 3])
    assert e[0] < 1e-5 and e[1] < 1e-8, e      # pose_0 composed with motion_0 is pose_1 (an arccos near 1 resolves sqrt(2^-52) rad = 1e-6 degrees)
    first = LC.pose12(I.rot_xyz(0.0, 0.01, 0.02), [1.0, 0.05, 0.0])
    rec, want = [], []
    for poses in (P, bad):
        for t in range(4):
            for fm in (None, first):
                rec.append(np.concatenate(([t, fm is not None], np.zeros(12) if fm is None else fm, poses.reshape(48))))
                want.append(D.odom_motion(poses, t, fm))
    got = host("odom", np.array(rec), 12)
    _same(got, np.array(want), "lpd_deskew_odom_motion")
    _same(got[0], O.IDENTITY, "t = 0 without a first_motion")
    _same(got[3], first, "t = 1 with one")
    _same(got[4], D.between(P[0:1], P[1:2])[0], "t = 2: between the two poses before it")
    _same(got[5], got[4], "t = 2 ignores first_motion")


# ---- written-down answers --------------------------------------------------------------------------------------------------------------------------
def test_the_identity_motion_and_the_passed_rows(host):
    pts, lengths, times, motions = C.boundary_table()
    rec, scan = _row_records(pts, lengths, times, motions, 0.5)
    got = host("row", rec, 28)
    n0 = int(lengths[0])
    tm = times[:n0]
    with np.errstate(invalid="ignore"):
        inside = (tm >= 0) & (tm <= 1)
    assert inside.sum() == 3 * 7 and (~inside).sum() == 3 * 5      # 0, 1, the two neighbours inside, -0.0, 0.5, 0.25 | the two outside, NaN, +-inf
    assert np.array_equal(got[:n0, 0], inside.astype(f64))
    assert np.array_equal(got[:n0, 1:4], pts[:n0].astype(f64))      # the identity: every row compares equal to its input ...
    assert got[0, 1:4].astype(f32).tobytes() == np.zeros(3, dtype=f32).tobytes()      # ... a transformed -0.0 is +0.0
    for k, (name, m) in enumerate(C.boundary_motions()):
        a, b = k * n0, (k + 1) * n0
        fin = bool(np.isfinite(m).all())
        assert np.array_equal(got[a:b, 0], (inside & fin).astype(f64)), name
        stay = got[a:b, 0] == 0
        assert got[a:b, 1:4][stay].astype(f32).tobytes() == pts[a:b][stay].tobytes(), name      # passed through: a bit copy
        if fin and k > 0:
            assert (np.abs(got[a:b, 1:4][~stay] - pts[a:b][~stay]).max(axis=1) > 0).any(), name
    out, info = D.deskew(pts, M.offsets_of(lengths), times, motions)
    assert info.tolist() == [int(got[:, 0].sum()), int((got[:, 0] == 0).sum())] and info[1] == 3 * 15 + 2 * 36
    assert out.tobytes() == got[:, 1:4].astype(f32).tobytes()


def test_hand_made_motions(host):
    ident = O.IDENTITY
    shift = ident.copy()
    shift[M.TRA] = (2.0, -0.5, 0.25)      # binary fractions: every operation is exact
    yaw90 = LC.pose12(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), [0.0, 0.0, 0.0])
    p = np.array([3.0, 1.0, -2.0])
    rec = [np.concatenate((shift, [tm, ref], p)) for tm, ref in ((0.0, 0.5), (1.0, 0.5), (0.5, 0.5), (0.75, 0.0), (0.25, 1.0))]
    rec += [np.concatenate((yaw90, [tm, 0.5], p)) for tm in (1.0, 0.0, 0.5)]
    got = host("row", np.array(rec), 28)
    assert got[:, 0].tolist() == [1.0] * 8
    for g, a in zip(got[:5], (-0.5, 0.5, 0.0, 0.75, -0.75)):
        assert g[1:4].tolist() == (p + a * shift[M.TRA]).tolist(), a      # a pure translation: p + a t, exactly
    # a = +0.5 of a quarter turn about z: the middle of the chord between the two quaternions is the middle of the arc, 45 degrees.
    # a = -0.5 lies OUTSIDE the chord, which the blend extends as a straight line: q ~ (1.5 - r / 2, 0, 0, -r / 2) with r = sqrt(1/2),
    # a turn of 2 atan2(-r / 2, 1.5 - r / 2) = -34.3 degrees (for the few degrees of a sweep the line and the arc agree to 1e-5).
    r = math.sqrt(0.5)
    for g, th in zip(got[5:7], (math.pi / 4, 2.0 * math.atan2(-0.5 * r, 1.5 - 0.5 * r))):
        want = np.array([3.0 * math.cos(th) - math.sin(th), 3.0 * math.sin(th) + math.cos(th), -2.0])
        assert np.abs(g[1:4] - want).max() <= 4e-7, (g[1:4], want)      # 1.5 ulp of an fp32 near 2.8: the one rounding and 1e-16 of float64
        assert g[3] == -2.0
    assert got[7, 1:4].tolist() == p.tolist()      # a = 0: the identity whatever the motion
    want, _ = D.rows(np.tile(p.astype(f32), (8, 1)), np.array([r[12] for r in rec], dtype=f32), np.array([r[:12] for r in rec]), 0.5)
    assert got[5:, 1:4].astype(f32).tobytes() == want[5:].tobytes()


def test_scan_fractions():
    lengths = [4, 1, 0, 3, 2]
    stamps = np.array([10.0, 10.1, 10.05, 10.025, 7.0, 1e9 + 0.1, 1e9, 1e9 + 0.05, 5.0, 5.0])
    got = odometry.scan_fractions(torch.from_numpy(stamps), lengths)
    assert got.dtype == torch.float32 and tuple(got.shape) == (10,)
    want = D.scan_fractions(stamps, lengths)
    assert got.numpy().tobytes() == want.tobytes()
    assert got[[0, 1, 4, 6, 8, 9]].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] and abs(float(got[2]) - 0.5) < 1e-6 and abs(float(got[7]) - 0.5) < 1e-6
    assert odometry.scan_fractions(stamps, lengths).numpy().tobytes() == want.tobytes()      # a numpy array: on the host
    for bad in (lambda: odometry.scan_fractions(stamps.astype(f32), lengths), lambda: odometry.scan_fractions(stamps, [4, 1]),
                lambda: odometry.scan_fractions(stamps.reshape(2, 5), lengths), lambda: odometry.scan_fractions(stamps, [10.0])):
        with pytest.raises(ValueError):
            bad()


def test_azimuth_fractions():
    pts = np.array([[-1.0, -1e-9, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 1e-9, 0.0]], dtype=f32)
    cw = odometry.azimuth_fractions(pts, [5]).numpy()
    assert np.abs(cw - np.array([1.0, 0.75, 0.5, 0.25, 0.0])).max() < 1e-6 and cw.dtype == f32
    ccw = odometry.azimuth_fractions(torch.from_numpy(pts), [2, 3], clockwise=False).numpy()
    assert np.abs(ccw - np.array([0.0, 0.25, 0.5, 0.75, 1.0])).max() < 1e-6
    with pytest.raises(ValueError):
        odometry.azimuth_fractions(pts, [4])


# ---- the quality conditions, restatement only ----------------------------------------------------------------------------------------------------
_DRIVES, _RUNS = {}, {}


def _drive(name, seed):
    if (name, seed) not in _DRIVES:
        _DRIVES[(name, seed)] = C.skewed_drive(seed, *C.DRIVES[name])
    return _DRIVES[(name, seed)]


def _worst(poses, truth):
    e = C.errors(poses, truth)
    return max(x[0] for x in e), max(x[1] for x in e)


def _runs(name, seed):
    """the three odometries of a skewed drive: of its clean rows, of its skewed rows as they are, of its skewed rows with times"""
    if (name, seed) not in _RUNS:
        d = _drive(name, seed)
        kw = C.estimate_kw(*C.DRIVES[name])
        clean = O.estimate(d["clean"], d["lengths"], d["truth"][0], **kw)
        skewed = O.estimate(d["points"], d["lengths"], d["truth"][0], **kw)
        desk = D.estimate(d["points"], d["lengths"], d["times"], d["truth"][0], **kw)
        _RUNS[(name, seed)] = (clean, skewed, desk)
    return _RUNS[(name, seed)]


@pytest.mark.parametrize("name", list(C.DRIVES))
@pytest.mark.parametrize("seed", C.SEEDS)
def test_residual_with_the_true_motion(name, seed):
    d = _drive(name, seed)
    out, info = D.deskew_drive(d["points"], d["lengths"], d["times"], motions=d["motions"])
    res = float(np.linalg.norm(out.astype(f64) - d["clean"].astype(f64), axis=1).max())
    ratio = res / d["skew"]
    print(f"MEASURE deskew {name} seed={seed}: largest skew {d['skew']:.4f} m, largest residual {res:.5f} m, ratio {ratio:.4f}")
    assert info.tolist() == [len(out), 0]
    assert ratio <= C.RESIDUAL_BOUND
    assert abs(ratio - C.RESIDUAL_RATIO[name][C.SEEDS.index(seed)]) < 1e-5      # the recorded figure is the measured one


@pytest.mark.parametrize("name", C.ODOMETRY_DRIVES)
def test_odometry_of_the_skewed_drives(name):
    runs = [(_drive(name, seed), _runs(name, seed)) for seed in C.SEEDS]
    worst = []
    for k, what in enumerate(("clean", "skewed", "deskewed")):
        e = [_worst(r[k]["poses"], d["truth"]) for d, r in runs]
        worst.append((max(x[0] for x in e), max(x[1] for x in e)))
        print(f"MEASURE deskew odometry {name} {what}: worst of {len(C.SEEDS)} seeds {worst[-1][0]:.4f} degrees {worst[-1][1]:.4f} m; per seed "
              + ", ".join(f"{a:.4f}/{b:.4f}" for a, b in e))
    clean, skewed, desk = worst
    print(f"MEASURE deskew odometry {name}: deskewed over skewed {desk[0] / skewed[0]:.3f} (rotation) {desk[1] / skewed[1]:.3f} (translation)")
    for d, r in runs:
        assert r[2]["valid"].all() and r[2]["passed"] == 0
    assert desk[0] <= C.FACTOR * skewed[0] and desk[1] <= C.FACTOR * skewed[1]
    assert desk[0] <= C.WORST_ROT_DEG[name] and desk[1] <= C.WORST_TRANS_M[name]
    for got, rec in ((clean, C.CLEAN[name]), (skewed, C.SKEWED[name]), (desk, C.DESKEWED[name])):
        assert abs(got[0] - rec[0]) < 1e-4 and abs(got[1] - rec[1]) < 1e-4, (got, rec)      # the recorded figures are the measured ones
    assert C.WORST_ROT_DEG[name] == 1.5 * C.DESKEWED[name][0] and C.WORST_TRANS_M[name] == 1.5 * C.DESKEWED[name][1]


def test_estimate_with_times_of_a_drive_that_does_not_move_is_the_plain_estimate():
    """identity motions throughout: every deskewed row compares equal to its input, so the chain is odom_ref.estimate's"""
    d = OC.street_drive(1, S=3, rows=1500, step=0.0, turn_deg=0.0)
    tm = np.random.default_rng(1).random(len(d["points"])).astype(f32)
    a = O.estimate(d["points"], d["lengths"], d["truth"][0], refresh=2, keep_m=20.0)
    b = D.estimate(d["points"], d["lengths"], tm, d["truth"][0], refresh=2, keep_m=20.0)
    assert np.array_equal(b["motions"][:2], np.tile(O.IDENTITY, (2, 1))) and b["passed"] == 0
    assert np.array_equal(b["points"][:3000], d["points"][:3000])
    _same(b["poses"][:2], a["poses"][:2], "the first two scans move under the identity")


# ---- the host side of the wrappers -------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from lpdnet_hip import LpdHipError
    pts, off, tm, mo = torch.zeros((10, 3)), torch.tensor([0, 10], dtype=torch.int32), torch.zeros(10), torch.zeros((1, 12), dtype=torch.float64)
    with pytest.raises(LpdHipError):
        ops.scan_deskew(pts, off, tm, mo)
    with pytest.raises(LpdHipError):
        ops.drive_motions(mo)
    with pytest.raises(LpdHipError):
        ops.odom_motion(mo, 0, mo.clone())
    for bad in (1.5, -0.1, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError):
            ops.deskew_ref(bad)
    assert ops.deskew_ref(0) == 0.0 and ops.deskew_ref(np.float32(0.5)) == 0.5
    with pytest.raises(ValueError):
        odometry.deskew_scans([np.zeros((4, 3), dtype=f32)], None, np.zeros(4, dtype=f32))      # neither poses nor motions
    with pytest.raises(ValueError):
        odometry.deskew_scans([np.zeros((4, 3), dtype=f32)], None, np.zeros(4, dtype=f32), poses=np.zeros((1, 12)), motions=np.zeros((1, 12)))
    with pytest.raises(ValueError):
        odometry.deskew_scans([np.zeros((4, 3), dtype=f32)], None, np.zeros(4, dtype=f32), poses=np.zeros((1, 12)), ref=2.0)
    o = odometry.Odometry(**{n: None for n in odometry.Odometry.__slots__})
    assert o.points is None and "passed" in odometry.Odometry.__slots__
