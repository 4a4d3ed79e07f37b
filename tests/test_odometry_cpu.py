"""CPU side of LiDAR odometry (lpd_odom_predict, lpd_odom_accept, lpd_map_crop, lpd_map_touch, lpdnet_hip/odometry.py): the kernels'
arithmetic header (csrc/lpd_odom_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/odom_ref.py)
value for value, the touched sets of random small maps, the quality conditions of the design on odom_cases.street_drive, and the host
side of the wrappers.  The kernels are tested on the GPU (tests/test_odometry_gpu.py)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import icp_ref as I
import loc_ref as L
import map_ref as M
import odom_cases as C
import odom_ref as O
from lpdnet_hip import mapping, odometry, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32, f64, i64 = np.float32, np.float64, np.int64

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_odom_math.h"
// <mode> <in> <out> <n>: float64 in, float64 out (integers as float64; a key as two 32-bit halves)
//   predict  poses 4 x 12, t, has first_motion, first_motion 12      -> pose 12
//   accept   pred 12, pose 12, info 4, len, t, share_q, max_jump    -> state, pose 12, insert 12
//   keep     key lo, key hi, centre 12, origin 3, inv_cell, keep    -> has centre, qc 3, kept
static uint64_t join(double lo, double hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }
int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    size_t rin = 0, rout = 0;
    if (!strcmp(mode, "predict")) { rin = 62; rout = 12; }
    else if (!strcmp(mode, "accept")) { rin = 32; rout = 25; }
    else if (!strcmp(mode, "keep")) { rin = 19; rout = 5; }
    else return 2;
    std::vector<double> in(n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 8, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t k = 0; k < n; ++k) {
        const double* r = &in[k * rin];
        double* o = &out[k * rout];
        if (!strcmp(mode, "predict")) {
            lpd_odom_predict_pose(r, (int)r[48], r[49] != 0.0 ? r + 50 : nullptr, o);
        } else if (!strcmp(mode, "accept")) {
            double pose[12];
            for (int c = 0; c < 12; ++c) pose[c] = r[12 + c];
            const int32_t info[4] = {(int32_t)r[24], (int32_t)r[25], (int32_t)r[26], (int32_t)r[27]};
            o[0] = (double)lpd_odom_accept_pose(r, pose, info, (int64_t)r[28], (int)r[29], (int)r[30], r[31], o + 13);
            for (int c = 0; c < 12; ++c) o[1 + c] = pose[c];
        } else {
            int qc[3] = {0, 0, 0};
            const int has = lpd_odom_centre_cell(r + 2, r + 14, (float)r[17], qc);
            o[0] = (double)has;
            for (int c = 0; c < 3; ++c) o[1 + c] = (double)qc[c];
            o[4] = (double)lpd_odom_keep((int64_t)join(r[0], r[1]), has, qc, (int)r[18]);
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
    d = tmp_path_factory.mktemp("odom_math")
    src = d / "odom_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "odom_math_host"
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


def test_predict_equals_the_restatement_value_for_value(host):
    cases = C.predict_cases()
    rec = np.zeros((len(cases), 62))
    for r, (_, P, t, motion) in zip(rec, cases):
        r[:48], r[48], r[49] = P.reshape(48), t, motion is not None
        if motion is not None:
            r[50:] = motion
    got = host("predict", rec, 12)
    for g, (name, P, t, motion) in zip(got, cases):
        _same(g, O.predict(P, t, motion), name)
    by = {name: g for g, (name, *_rest) in zip(got, cases)}
    straight = C.hand_drive(5)
    _same(by["straight t=2"], straight[2], "exact arithmetic: scan 2 of a straight drive")      # every operation is exact here
    _same(by["straight t=3"], straight[3], "exact arithmetic: scan 3")
    _same(by["straight t=0"], straight[0], "t = 0")
    _same(by["straight t=1"], straight[0], "t = 1 starts at pose 0")
    e = I.pose_error(by["quarter turn t=3"], I.rot_xyz(0.0, 0.0, 3 * math.pi / 2), np.array([0.0, -1.0, 0.0]))
    assert e[0] < 1e-12 and e[1] < 1e-12, e
    R = by["UTM t=3"].reshape(3, 4)[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 4e-16      # renormalised through the quaternion
    P = cases[[n for n, *_ in cases].index("NaN at t-2")][1]
    _same(by["NaN at t-2"], P[2], "P[t-2] not finite: P[t-1]")
    P = cases[[n for n, *_ in cases].index("inf at t-1")][1]
    _same(by["inf at t-1"], P[2], "P[t-1] not finite: that pose")
    assert not np.isfinite(by["inf at t-1"]).all()
    _same(by["t=0 with a first_motion"], cases[[n for n, *_ in cases].index("UTM t=2")][1][0], "t = 0 ignores first_motion")
    assert np.abs(by["t=1 with a first_motion"][M.TRA] - by["t=1 without"][M.TRA]).max() > 0.5


def test_accept_equals_the_restatement_at_both_sides_of_every_threshold(host):
    cases = C.accept_cases()
    rec = np.array([np.concatenate((pred, pose, info, [n, t, sq, mj])) for _, pred, pose, info, n, t, sq, mj, _ in cases])
    got = host("accept", rec, 25)
    for g, (name, pred, pose, info, n, t, sq, mj, want) in zip(got, cases):
        state, p, ins = O.accept(pred, pose, info, n, t, sq, mj)
        assert int(g[0]) == state == want, (name, g[0], state, want)
        _same(g[1:13], p, name)
        _same(g[13:], ins, name)
        if want:
            _same(g[13:], pose, name + ": the insert pose is the pose")
        else:
            _same(g[1:13], pred, name + ": the pose is the prediction, bit for bit")
            assert np.isnan(g[13:]).all(), name
    assert O.share_q(0.1) == 102 and O.share_q(0.0) == 0 and O.share_q(1.0) == 1024 and ops.odom_share_q(0.1) == 102


def _halves(v):
    v = np.asarray(v).astype(np.uint64)
    return (v & np.uint64(0xffffffff)).astype(f64), (v >> np.uint64(32)).astype(f64)


def test_crop_predicate_at_the_edges(host):
    for centre, origin, cell, keep, q in C.keep_cases():
        keys = M.key(q)
        lo, hi = _halves(keys)
        rec = np.concatenate((np.stack((lo, hi), axis=1), np.tile(np.concatenate((centre, origin, [float(M.inv_cell(cell)), keep])), (len(q), 1))), axis=1)
        got = host("keep", rec, 5)
        has, qc = O.centre_cell(centre, origin, cell)
        want = O.keep(keys, has, qc, keep)
        assert np.array_equal(got[:, 0], np.full(len(q), float(has)))
        if has:
            assert np.array_equal(got[:, 1:4], np.tile(qc.astype(f64), (len(q), 1)))
            by_hand = (np.abs(q - qc[None, :]) <= keep).all(axis=1)
            assert np.array_equal(want, by_hand) and (keep >= 2 * M.QLIM or not want.all()) and want.any()
        else:
            assert want.all()
        assert np.array_equal(got[:, 4], want.astype(f64)), (cell, keep)
    has, qc = O.centre_cell(C.keep_cases()[0][0], C.keep_cases()[0][1], 1.0)
    assert has and qc.tolist() == [10, -4, 0]
    assert O.centre_cell(C.keep_cases()[3][0], C.keep_cases()[3][1], 0.5)[1].tolist() == [M.QLIM - 3, 3, 0]


# ---- the touched set -----------------------------------------------------------------------------------------------------------------------------
def _rows_equal(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)


@pytest.mark.parametrize("reach", [1, 2])
def test_touched_set_holds_every_changed_surface_row_and_nothing_out_of_reach(reach):
    rng = np.random.default_rng(20 + reach)
    origin = np.zeros(3)
    poses = np.tile(O.IDENTITY, (2, 1))
    a = rng.uniform(-6.0, 6.0, (900, 3)) * np.array([1.0, 1.0, 0.3])
    b = rng.uniform(-2.0, 3.0, (150, 3)) * np.array([1.0, 1.0, 0.3])
    pts, off = np.concatenate((a, b)).astype(f32), M.offsets_of([len(a), len(b)])
    before = M.insert(pts, off, poses, origin, 1.0, 0, 1)
    after = M.insert(pts, off, poses, origin, 1.0, 1, 2, into=before)
    s0, s1 = L.surface(before, reach, 5), L.surface(after, reach, 5)
    mark = O.touched(after.keys, O.row_keys(pts, off, poses, origin, 1.0, 1, 2), reach)
    old = L.lookup(before.keys, after.keys)
    changed = (old < 0) | ~_rows_equal(s1.rows(), s0.rows()[np.maximum(old, 0)])
    assert changed.sum() > 20 and (~mark).sum() > 20 and not (changed & ~mark).any()
    qb = M.unkey(np.unique(O.row_keys(pts, off, poses, origin, 1.0, 1, 2)))
    dist = np.abs(M.unkey(after.keys)[:, None, :] - qb[None, :, :]).max(axis=2).min(axis=1)
    assert np.array_equal(mark, dist <= reach)


# ---- the quality conditions, restatement only ------------------------------------------------------------------------------------------------------
_RUNS = {}


def _drive_run(seed, cell):
    if (seed, cell) not in _RUNS:
        d = C.street_drive(seed)
        _RUNS[(seed, cell)] = (d, C.estimate(d, cell))
    return _RUNS[(seed, cell)]


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("seed", C.SEEDS)
def test_quality_of_a_street_drive(seed, cell):
    d, r = _drive_run(seed, cell)
    e = C.errors(r["poses"], d["truth"])
    rot, trans, share = max(x[0] for x in e), max(x[1] for x in e), r["inliers"][1:].min()
    print(f"MEASURE odometry seed={seed} cell={cell}: worst {rot:.4f} degrees {trans:.4f} m, inlier shares {share:.4f} .. {r['inliers'].max():.4f}")
    assert r["valid"].all(), r["valid"]
    assert r["info"][1:, 1].tolist() == [8] * (C.DRIVE_S - 1) and not r["info"][:, 2].any()      # eight steps applied, none refused
    assert len(r["left"]) == 1 and r["left"][0] > 0, r["left"]      # the crop in the middle left cells behind
    assert rot <= C.WORST_ROT_DEG[cell] and trans <= C.WORST_TRANS_M[cell]
    assert share >= C.TRUE_SHARE_MIN - 5e-5


@pytest.mark.parametrize("cell", C.CELLS)
def test_the_bounds_are_one_and_a_half_times_the_measured_worst(cell):
    runs = [_drive_run(seed, cell) for seed in C.SEEDS]
    e = [x for d, r in runs for x in C.errors(r["poses"], d["truth"])]
    rot, trans = max(x[0] for x in e), max(x[1] for x in e)
    print(f"MEASURE odometry cell={cell}: worst of {len(C.SEEDS)} seeds {rot:.4f} degrees {trans:.4f} m")
    assert abs(rot - C.MEASURED_ROT_DEG[cell]) < 1e-4 and abs(trans - C.MEASURED_TRANS_M[cell]) < 1e-4
    assert C.WORST_ROT_DEG[cell] == 1.5 * C.MEASURED_ROT_DEG[cell] and C.WORST_TRANS_M[cell] == 1.5 * C.MEASURED_TRANS_M[cell]


@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("seed", C.SEEDS)
def test_a_lost_scan_keeps_its_prediction_and_stays_out_of_the_map(seed, cell):
    k = C.LOST_AT
    d, _ = _drive_run(seed, cell)
    pts, lengths = C.with_lost_scan(d)
    maps = {}
    lost = C.estimate(d, cell, pts, lengths, on_map=lambda t, c: maps.__setitem__(t, c))
    share = lost["info"][k, 3] / lengths[k]
    print(f"MEASURE odometry seed={seed} cell={cell}: inlier share of the lost scan {share:.4f}, of the scans after it "
          f"{lost['inliers'][k + 1:].min():.4f} .. {lost['inliers'][k + 1:].max():.4f}")
    assert share <= C.LOST_SHARE_MAX + 5e-5
    assert not lost["valid"][k] and lost["valid"].sum() == len(lengths) - 1, lost["valid"]
    _same(lost["poses"][k], lost["pred"][k], "the lost scan's pose is its prediction")
    assert np.isnan(lost["insert_pose"][k]).all()
    # the map after the lost scan is the map of the same drive without that scan (up to it the two drives are the same drive)
    pts0, lengths0 = C.without_scan(d)
    maps0 = {}
    C.estimate(d, cell, pts0, lengths0, on_map=lambda t, c: maps0.__setitem__(t, c))
    for name in ("keys", "sums", "counts"):
        assert np.array_equal(getattr(maps[k], name), getattr(maps0[k], name)), name
    e = C.errors(lost["poses"], d["truth"])
    assert max(x[0] for x in e[k + 1:]) <= C.WORST_ROT_DEG[cell] and max(x[1] for x in e[k + 1:]) <= C.WORST_TRANS_M[cell]


def test_default_min_share_separates_lost_from_true_scans():
    assert C.LOST_SHARE_MAX < C.TRUE_SHARE_MIN
    gm = math.sqrt(C.LOST_SHARE_MAX * C.TRUE_SHARE_MIN)
    print(f"MEASURE odometry min_share: largest lost {C.LOST_SHARE_MAX}, smallest true {C.TRUE_SHARE_MIN}, geometric mean {gm:.4f}")
    assert abs(gm - C.MIN_SHARE) < 0.01 and C.LOST_SHARE_MAX < C.MIN_SHARE < C.TRUE_SHARE_MIN
    assert odometry.OdometrySearch().min_share == C.MIN_SHARE


def test_occupied_cells_at_the_estimated_poses():
    worst = 0.0
    for seed in C.SEEDS:
        d, r = _drive_run(seed, 1.0)
        off, org = M.offsets_of(d["lengths"]), d["truth"][0, M.TRA]
        worst = max(worst, M.occupied(d["points"], off, r["poses"], org, 1.0) / M.occupied(d["points"], off, d["truth"], org, 1.0))
    print(f"MEASURE odometry: occupied cells at the estimated over the true poses, worst {worst:.4f}")
    assert worst <= C.OCCUPIED_RATIO + 5e-5 and worst <= C.OCCUPIED_BOUND


# ---- the host side of the wrappers -------------------------------------------------------------------------------------------------------------
def test_search_is_validated_and_frozen():
    s = odometry.OdometrySearch()
    assert (s.cell, s.refresh, s.capacity, s.surface, s.first_motion) == (1.0, 10, None, odometry.SURFACES[0], None) and s.keep_cells == 60
    assert odometry.OdometrySearch(cell=0.5, keep=10.2).keep_cells == 21 and s.share_q == O.share_q(s.min_share)
    assert s == odometry.OdometrySearch() and hash(s) == hash(odometry.OdometrySearch()) and s != odometry.OdometrySearch(refresh=None)
    with pytest.raises(AttributeError):
        s.cell = 2.0
    m = odometry.OdometrySearch(first_motion=np.eye(4)[:3]).first_motion
    assert m == tuple(O.IDENTITY)
    for kw in (dict(cell=0.0), dict(cell=32.0), dict(cell="1"), dict(keep=-1.0), dict(keep=float("nan")), dict(keep=1e9, cell=2.0 ** -10),
               dict(refresh=0), dict(refresh=2.5), dict(refresh=True), dict(capacity=1000), dict(capacity=8), dict(capacity=2.0 ** 10),
               dict(localize=None), dict(min_share=-0.1), dict(min_share=1.5), dict(min_share=float("nan")), dict(max_jump=-1.0),
               dict(max_jump=float("inf")), dict(first_motion=np.zeros(11)), dict(first_motion=np.full(12, np.nan)),
               dict(first_motion=np.zeros(12, dtype=f32)), dict(surface="fast"), dict(surface=None)):
        with pytest.raises(ValueError):
            odometry.OdometrySearch(**kw)


def test_wrappers_refuse_host_tensors_and_estimate_poses_checks_its_search():
    from lpdnet_hip import LpdHipError
    P = torch.zeros((3, 12), dtype=torch.float64)
    with pytest.raises(LpdHipError):
        ops.odom_predict(P, P.clone(), 1)
    with pytest.raises(LpdHipError):
        ops.odom_accept(P, P.clone(), torch.zeros((3, 4), dtype=torch.int32), torch.zeros(4, dtype=torch.int32), 1, 100, 5.0, P.clone(),
                        torch.zeros(3, dtype=torch.int32))
    with pytest.raises(LpdHipError):
        ops.map_surface_touched(torch.zeros(16, dtype=torch.int64), torch.zeros((16, 4), dtype=torch.int64), torch.zeros((16, 8)),
                                torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(TypeError):
        odometry.estimate_poses([np.zeros((4, 3), dtype=f32)], None, search=mapping.LocalizeSearch())
    with pytest.raises(ValueError):
        ops.odom_share_q(2.0)
