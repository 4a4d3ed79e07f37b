"""CPU side of the 6-DoF refinement (lpd_point_normals, lpd_icp_pairs, lpdnet_hip/verify.py): the kernels' arithmetic header
(csrc/lpd_icp_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/icp_ref.py) value for value,
the three-row Jacobi against fp64 eigh, hand-made registrations with their answers written down, the quality of the restatement on
the labelled street scenes of tests/align_ref.py, and the validation of RefineSearch, ops.point_normals and ops.icp_pairs.  The
kernels themselves are tested on the GPU (tests/test_icp_gpu.py)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_ref as AR
import icp_ref as R
from lpdnet_hip import LpdHipError, ops, verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32 = np.float32

# ---- the gates ---------------------------------------------------------------------------------------------------------------------
# Normals: 1 - |n . n_ref| of the fp32 three-row Jacobi against fp64 eigh on noisy planar patches whose fp64 eigengap (l2 - l3) / l1
# is at least NORMAL_MIN_GAP.  The restatement shows NORMAL_MEASURED at most (test_normals_against_eigh prints it); the gate is 4 x.
NORMAL_MIN_GAP = 0.05
NORMAL_MEASURED = 8.3e-8
NORMAL_GATE = 4 * NORMAL_MEASURED
# Quality on true_pair(0..11), N = 4096, eight iterations at dmax = 1 m, normals from 16 neighbours, from the start of
# icp_ref.tilted_true_pair: the restatement ends at QUALITY_MEASURED_* at most (test_quality_on_street_scenes prints every pair); the
# gates are 1.5 x, twelve scenes being a small sample.
QUALITY_MEASURED_DEG, QUALITY_MEASURED_M = 0.268, 0.072
QUALITY_GATE_DEG, QUALITY_GATE_M = 1.5 * QUALITY_MEASURED_DEG, 1.5 * QUALITY_MEASURED_M
QUALITY_SEARCH = dict(k=16, dmax=1.0, iterations=8, min_inliers=32)

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_icp_math.h"
// <mode> <in> <out> <n>: n fixed-size records in, n fixed-size records out
//   xform   12 f64 (pose) + 4 f32 (x y z sc)          -> 3 f32 (p) + 1 i32 (ok)
//   d2      7 f32 (q, p, dmax)                        -> 1 f32 (d2) + 1 i32 (within) + 1 i32 (nearer than dmax as a running best)
//   quant   1 f32                                     -> 1 i64
//   row     9 f32 (p, q, n)                           -> 32 i64 (the terms; 29..31 zero) + 7 i64 (Ji, ri)
//   solve   32 i64 (sums) + 1 i64 (min_inliers) + 12 f64 (pose) -> 1 i64 (applied) + 12 f64 (pose)
//   normal  9 f32 (sx sy sz sxx sxy sxz syy syz szz) + 1 f32 (k) -> 4 f32 (n, flatness)
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    size_t rin = 0, rout = 0;
    if (!strcmp(mode, "xform")) { rin = 112; rout = 16; }
    else if (!strcmp(mode, "d2")) { rin = 28; rout = 12; }
    else if (!strcmp(mode, "quant")) { rin = 4; rout = 8; }
    else if (!strcmp(mode, "row")) { rin = 36; rout = 312; }
    else if (!strcmp(mode, "solve")) { rin = 360; rout = 104; }
    else if (!strcmp(mode, "normal")) { rin = 40; rout = 16; }
    else return 2;
    std::vector<unsigned char> in(n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 1, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char* r = &in[i * rin];
        unsigned char* o = &out[i * rout];
        if (!strcmp(mode, "xform")) {
            double pose[12];
            float f[4], p[3];
            memcpy(pose, r, 96);
            memcpy(f, r + 96, 16);
            const int32_t ok = lpd_icp_transform(lpd_icp_pose32(pose), f[0], f[1], f[2], f[3], p) ? 1 : 0;
            memcpy(o, p, 12);
            memcpy(o + 12, &ok, 4);
        } else if (!strcmp(mode, "d2")) {
            float f[7];
            memcpy(f, r, 28);
            const float d = lpd_icp_d2(f[0], f[1], f[2], f[3], f[4], f[5]);
            const int32_t w[2] = {lpd_icp_within(d, f[6]) ? 1 : 0, lpd_icp_nearer(d, f[6]) ? 1 : 0};
            memcpy(o, &d, 4);
            memcpy(o + 4, w, 8);
        } else if (!strcmp(mode, "quant")) {
            float v;
            memcpy(&v, r, 4);
            const int64_t q = lpd_icp_quant(v);
            memcpy(o, &q, 8);
        } else if (!strcmp(mode, "row")) {
            float f[9];
            memcpy(f, r, 36);
            int64_t t[LPD_ICP_SUMS] = {0}, J[7];
            lpd_icp_row(f, f + 3, f + 6, J, &J[6]);
            lpd_icp_terms(J, J[6], t);
            memcpy(o, t, 256);
            memcpy(o + 256, J, 56);
        } else if (!strcmp(mode, "solve")) {
            int64_t s[33];
            double pose[12];
            memcpy(s, r, 264);
            memcpy(pose, r + 264, 96);
            const int64_t ok = lpd_icp_solve(s, (int)s[32], pose);
            memcpy(o, &ok, 8);
            memcpy(o + 8, pose, 96);
        } else {
            float f[10], res[4];
            memcpy(f, r, 40);
            LpdFeatMoments m;
            lpd_feat_init(m);
            m.sx = f[0]; m.sy = f[1]; m.sz = f[2]; m.sxx = f[3]; m.sxy = f[4]; m.sxz = f[5]; m.syy = f[6]; m.syz = f[7]; m.szz = f[8];
            lpd_icp_normal(m, (int)f[9], res, res + 3);
            memcpy(o, res, 16);
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo || fwrite(out.data(), 1, out.size(), fo) != out.size()) return 4;
    fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("icp_math")
    src = d / "icp_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "icp_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, blob, n, out_bytes):
        (d / "in.bin").write_bytes(blob)
        r = subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(n)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        got = np.fromfile(d / "out.bin", dtype=np.uint8)
        assert got.size == n * out_bytes
        return got.reshape(n, out_bytes)
    return run


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _pack(*cols):
    """records: the byte images of the columns side by side"""
    return np.concatenate([_bits(c) for c in cols], axis=1).tobytes()


def _next(v, toward):
    return np.nextafter(f32(v), f32(toward))


def _small_pose(g, rot=0.1, shift=3.0):
    M = np.zeros((3, 4))
    M[:, :3] = R.rot_xyz(*g.uniform(-rot, rot, 3))
    M[:, 3] = g.uniform(-shift, shift, 3)
    return M.reshape(12)


# ---- 1. the arithmetic header against the restatement -------------------------------------------------------------------------------
def test_transform_and_the_512_m_rule(host):
    g = np.random.default_rng(1)
    n = 3000
    poses = np.stack([_small_pose(g, 3.0, 30.0) for _ in range(n)])
    pts = g.uniform(-60, 60, (n, 3)).astype(f32)
    sc = g.choice([1.0, 0.7, 25.0], n).astype(f32)
    # the edges: exactly +-512 passes, one ulp beyond does not; NaN, inf and an overflowing product do not
    eye = np.eye(3, 4).reshape(12)
    edge = [(eye, [512.0, 0, 0], 1.0), (eye, [_next(512.0, 1e9), 0, 0], 1.0), (eye, [0, -512.0, 0], 1.0), (eye, [0, _next(-512.0, -1e9), 0], 1.0),
            (eye, [0, 0, 256.0], 2.0), (eye, [0, 0, _next(256.0, 1e9)], 2.0), (eye, [np.nan, 0, 0], 1.0), (eye, [0, np.inf, 0], 1.0),
            (eye, [1e30, 0, 0], 1e30), (eye, [1.0, 2.0, 3.0], np.nan), (np.where(np.arange(12) == 3, 511.5, eye), [0.5, 0, 0], 1.0),
            (np.where(np.arange(12) == 3, 511.5, eye), [_next(0.5, 1.0), 0, 0], 1.0)]
    poses = np.concatenate((poses, np.stack([e[0] for e in edge])))
    pts = np.concatenate((pts, np.array([e[1] for e in edge], dtype=f32)))
    sc = np.concatenate((sc, np.array([e[2] for e in edge], dtype=f32)))
    got = host("xform", _pack(poses, pts, sc), len(pts), 16)
    for i in range(len(pts)):
        p, live = R.transform(poses[i], pts[i:i + 1], sc[i])
        assert got[i, :12].tobytes() == p.astype(f32).tobytes() and int(got[i, 12:].view(np.int32)[0]) == int(live[0]), i
    lives = got[n:, 12:].view(np.int32)[:, 0].tolist()
    assert lives == [1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1]      # the last: 511.5 + nextafter(0.5) rounds to 512.0 -- the rule reads the rounded p
    rnd = got[:n, 12:].view(np.int32)[:, 0]
    assert 0 < rnd.sum() < n      # both outcomes among the random records


def test_d2_and_the_dmax_decision_at_equality(host):
    g = np.random.default_rng(2)
    q, p = g.uniform(-30, 30, (4000, 3)).astype(f32), g.uniform(-30, 30, (4000, 3)).astype(f32)
    dmax = g.uniform(0.1, 16.0, 4000).astype(f32)
    # d2 == dmax * dmax exactly, and nextafter on both sides: d = (dmax, 0, 0) with dmax * dmax exact in fp32
    for dm in (0.5, 1.0, 1.5, 3.0, 16.0):
        for step in (0.0, 1e9, -1e9):
            dd = f32(dm) if step == 0.0 else _next(dm, step)
            q = np.concatenate((q, np.array([[dd, 0, 0]], dtype=f32)))
            p = np.concatenate((p, np.zeros((1, 3), dtype=f32)))
            dmax = np.concatenate((dmax, np.array([dm], dtype=f32)))
    for bad in (np.nan, np.inf, -np.inf):
        q = np.concatenate((q, np.array([[bad, 0, 0]], dtype=f32)))
        p = np.concatenate((p, np.zeros((1, 3), dtype=f32)))
        dmax = np.concatenate((dmax, np.array([16.0], dtype=f32)))
    got = host("d2", _pack(q, p, dmax), len(q), 12)
    want = np.array([R.d2(q[i:i + 1], p[i:i + 1])[0, 0] for i in range(len(q))], dtype=f32)
    assert got[:, :4].tobytes() == want.tobytes()
    dec = got[:, 4:].view(np.int32)
    with np.errstate(all="ignore"):
        assert np.array_equal(dec[:, 0], np.array([int(R.within(want[i], dmax[i])) for i in range(len(q))]))
        assert np.array_equal(dec[:, 1], (want < dmax).astype(np.int32))      # a NaN or inf distance is never nearer
    assert dec[4000:4015, 0].tolist() == [1, 0, 1] * 5 and dec[4015:, 0].tolist() == [0, 0, 0] and dec[4015:, 1].tolist() == [0, 0, 0]


def test_rows_terms_and_quantisation(host):
    vals = [0.0, -0.0, 1.0, -1.0, 0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024, -1.5 / 1024, 1023.5 / 1024, 1024.0, 1024.0 + 1 / 1024, -1024.0, 1e9, -1e9,
            np.inf, -np.inf, np.nan, 3.4e38, 1e-30, _next(0.5 / 1024, 1.0), _next(0.5 / 1024, 0.0), 1023.9995]
    g = np.random.default_rng(3)
    v = np.concatenate((np.array(vals, dtype=f32), g.uniform(-1100, 1100, 4000).astype(f32), (g.integers(-2000, 2000, 2000) + 0.5).astype(f32) / f32(1024)))
    got = host("quant", _pack(v), len(v), 8).view(np.int64)[:, 0]
    assert np.array_equal(got, R.quant(v))
    assert got[:18].tolist() == [0, 0, 1024, -1024, 0, 2, 2, 0, -2, 1024, 1 << 20, 1 << 20, -(1 << 20), 1 << 20, -(1 << 20), 1 << 20, -(1 << 20), 0]
    # rows: random correspondences, and clamped ones (a lever arm of 500 m against a unit normal: 500 * 1024 < 2^20, 512 * 2 > it)
    n = 3000
    p = g.uniform(-40, 40, (n, 3)).astype(f32)
    q = (p + g.uniform(-1, 1, (n, 3))).astype(f32)
    nr = g.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(f32)
    p[:50] = g.uniform(-512, 512, (50, 3)).astype(f32) * f32(3.0)
    nr[50:60] = np.nan
    q[60:70] = np.inf
    rec = host("row", _pack(p, q, nr), n, 312).view(np.int64)
    Ji, ri = R.rows(p, q, nr)
    assert np.array_equal(rec[:, 32:38], Ji) and np.array_equal(rec[:, 38], ri)
    assert np.abs(Ji[:50, :3]).max() == 1 << 20      # the clamp is reached
    for i in range(0, n, 37):
        want = R.sums_of(Ji[i:i + 1], ri[i:i + 1])
        assert rec[i, :32].tolist() == want and want[0] == 1 and want[29:] == [0, 0, 0]


# ---- 2. the step -------------------------------------------------------------------------------------------------------------------
def _corner(g, n_side=20, noise=0.0):
    """three orthogonal patches x = 0, y = 0, z = 0 of a corner, with their exact normals -> (points [3 m, 3] fp32, normals)"""
    u, v = np.meshgrid(np.linspace(0.3, 6.0, n_side), np.linspace(0.3, 6.0, n_side))
    u, v = u.ravel() + g.uniform(-0.1, 0.1, u.size), v.ravel() + g.uniform(-0.1, 0.1, v.size)
    z = np.zeros_like(u)
    pts = np.concatenate((np.stack((z, u, v), 1), np.stack((u, z, v), 1), np.stack((u, v, z), 1)))
    nrm = np.repeat(np.eye(3), u.size, axis=0)
    return (pts + g.normal(0, noise, pts.shape) if noise else pts).astype(f32), nrm.astype(f32)


def _solve_records(host, sums, mins, poses):
    sums, poses = np.asarray(sums, dtype=np.int64), np.asarray(poses, dtype=np.float64)
    got = host("solve", _pack(sums, np.asarray(mins, dtype=np.int64), poses), len(sums), 104)
    return got[:, :8].view(np.int64)[:, 0], got[:, 8:].view(np.float64)


def test_solve_and_pose_update_bit_for_bit(host):
    g = np.random.default_rng(4)
    b, nb = _corner(g, 12, 0.01)
    sums, mins, poses = [], [], []
    for i in range(200):      # integer sums made from real correspondences of a corner under small random poses
        pose = _small_pose(g, 0.05, 0.3)
        a = b[g.choice(len(b), 200)] + g.normal(0, 0.02, (200, 3)).astype(f32)
        s, _ = R.one_pass(pose, a, 1.0, b, 1.0, nb, 1.0)
        sums.append(s)
        mins.append(6)
        poses.append(_small_pose(g, 3.0, 50.0) if i % 2 else pose)
    ok, out = _solve_records(host, sums, mins, poses)
    assert ok.min() == 1
    for i in range(len(sums)):
        applied, want = R.solve(sums[i], mins[i], poses[i])
        assert applied and out[i].tobytes() == want.tobytes(), i
        assert out[i].tobytes() != np.asarray(poses[i]).tobytes()
    # the update keeps a rotation a rotation
    Rm = out[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14


def test_refused_steps_return_the_poses_exact_bits(host):
    g = np.random.default_rng(5)
    b, nb = _corner(g, 12)
    pose = _small_pose(g, 0.05, 0.3)
    good, _ = R.one_pass(pose, b, 1.0, b, 1.0, nb, 1.0)
    assert R.solve(good, 6, pose)[0]
    # too few inliers; a singular system (a single plane: all normals parallel); a pivot that is not finite; a NaN in the pose
    plane = b[nb[:, 2] == 1]
    flat, _ = R.one_pass(pose, plane, 1.0, plane, 1.0, nb[nb[:, 2] == 1], 1.0)
    huge = list(good)
    for e in (R.SUM_H, R.SUM_H + 6, R.SUM_H + 11, R.SUM_H + 15, R.SUM_H + 18, R.SUM_H + 20):
        huge[e] = (1 << 62)
    huge[R.SUM_H + 1] = -(1 << 62)      # the second pivot is 2^62 - 2^62 = 0
    empty = [0] * 32
    odd = np.array(pose)
    odd[5] = -0.0
    cases = [(good, good[0] + 1, pose), (flat, 6, pose), (huge, 6, pose), (empty, 6, pose), (good, 1 << 40, odd)]
    ok, out = _solve_records(host, [c[0] for c in cases], [min(c[1], (1 << 31) - 1) for c in cases], [c[2] for c in cases])
    assert ok.tolist() == [0] * len(cases)
    for i, (s, mn, ps) in enumerate(cases):
        applied, want = R.solve(s, min(mn, (1 << 31) - 1), ps)
        assert not applied and want.tobytes() == np.asarray(ps, dtype=np.float64).tobytes()
        assert out[i].tobytes() == np.asarray(ps, dtype=np.float64).tobytes(), i
    assert flat[0] == len(plane) and R.ldl(flat) is None and R.ldl(huge) is None
    nanpose = np.array(pose)
    nanpose[3] = np.nan      # the system is fine, the new pose is not finite: refused, the NaN's bits included
    ok, out = _solve_records(host, [good], [6], [nanpose])
    assert ok.tolist() == [0] and out[0].tobytes() == nanpose.tobytes() and not R.solve(good, 6, nanpose)[0]


# ---- 3. normals --------------------------------------------------------------------------------------------------------------------
def _patches(seed, n_patches=60, per=64):
    """noisy planar patches of random orientation, extent 0.5-3 m, noise 1-3 cm, anywhere within 40 m -> [n, 3] fp32"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n_patches):
        Rm = R.rot_xyz(*g.uniform(-np.pi, np.pi, 3))
        ext = g.uniform(0.5, 3.0, 2)
        loc = np.column_stack((g.uniform(-ext[0], ext[0], per), g.uniform(-ext[1], ext[1], per), g.normal(0, g.uniform(0.01, 0.03), per)))
        out.append(loc @ Rm.T + g.uniform(-40, 40, 3))
    return np.concatenate(out).astype(f32)


def test_normals_against_eigh(host):
    worst, used, total = 0.0, 0, 0
    for seed in range(4):
        x = _patches(seed)
        idx = R.knn_lists(x, 16)
        n, flat = R.point_normals(x, idx)
        ref, gap = R.eigh_normals(x, idx)
        sel = gap >= NORMAL_MIN_GAP
        err = 1.0 - np.abs((n.astype(np.float64) * ref).sum(axis=1))
        worst, used, total = max(worst, float(err[sel].max())), used + int(sel.sum()), total + len(x)
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 2e-7 and (flat[sel] < 1.0).all()
        # the header's three-row Jacobi gives the restatement's bits
        s = R.moments(x, idx)
        rec = host("normal", _pack(*[s[k] for k in ("sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz")], np.full(len(x), 16, dtype=f32)), len(x), 16)
        assert rec[:, :12].tobytes() == n.tobytes() and rec[:, 12:].tobytes() == flat.tobytes()
    print(f"MEASURE icp/normals restatement 1-|n.n_ref| max={worst:.3e} over {used} of {total} points with gap >= {NORMAL_MIN_GAP}; "
          f"recorded {NORMAL_MEASURED:.1e}, gate {NORMAL_GATE:.1e}")
    assert used > 0.8 * total
    assert worst <= NORMAL_GATE
    assert worst >= NORMAL_MEASURED / 4      # the recorded value is what the restatement shows, not a guess far above it


def test_normals_hand_made(host):
    g = np.random.default_rng(6)
    # a cloud in the plane z = 0: exactly (0, 0, +-1), flatness 0
    x = np.column_stack((g.uniform(-5, 5, (300, 2)), np.zeros(300))).astype(f32)
    idx = R.knn_lists(x, 12)
    n, flat = R.point_normals(x, idx)
    assert np.array_equal(np.abs(n), np.tile(np.array([0, 0, 1], dtype=f32), (300, 1))) and not flat.any()
    # zero extent (every neighbour is the point itself) and non-finite inputs: (0, 0, 0)
    same = np.zeros((300, 12), dtype=np.int32) + np.arange(300, dtype=np.int32)[:, None]
    n0, f0 = R.point_normals(x, same)
    assert not n0.any() and not f0.any()
    bad = x.copy()
    bad[7, 0], bad[9, 2], bad[11, 1] = np.nan, np.inf, 3e38
    nb, fb = R.point_normals(bad, idx)
    touched = np.isin(idx, (7, 9, 11)).any(axis=1)
    touched[[7, 9, 11]] = True
    assert touched.sum() > 3 and not nb[touched].any() and not fb[touched].any()
    assert np.array_equal(np.abs(nb[~touched]), np.abs(n[~touched]))
    # an index outside the cloud reads the last point
    wild = idx.copy()
    wild[:, 3] = np.where(np.arange(300) % 2 == 0, -5, 10 ** 6)
    last = idx.copy()
    last[:, 3] = 299
    assert np.array_equal(R.point_normals(x, wild)[0], R.point_normals(x, last)[0])
    for pts, lists in ((x, idx), (x, same), (bad, idx)):
        s = R.moments(pts, lists)
        rec = host("normal", _pack(*[s[k] for k in ("sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz")], np.full(300, 12, dtype=f32)), 300, 16)
        want = R.point_normals(pts, lists)
        assert rec[:, :12].tobytes() == want[0].tobytes() and rec[:, 12:].tobytes() == want[1].tobytes()


# ---- 4. hand-made registration -----------------------------------------------------------------------------------------------------
CORNER_W, CORNER_T = (0.02, -0.015, 0.01), (0.05, -0.03, 0.04)      # the written-down transform: rotation vector (rad), translation (m)
CORNER_EXT_DEG, CORNER_EXT_M = 4.7e-4, 3.7e-4      # the chain's error with the step solved in np.longdouble (printed by the test)


def _rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _solve_extended(sums, pose):
    """the step with the 6 x 6 system solved in np.longdouble by Gaussian elimination with partial pivoting, the update in longdouble"""
    ld = np.longdouble
    H = np.zeros((6, 6), dtype=ld)
    e = R.SUM_H
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = ld(int(sums[e]))
            e += 1
    M = np.concatenate((H, np.array([ld(int(sums[R.SUM_G + a])) for a in range(6)], dtype=ld)[:, None]), axis=1)
    for c in range(6):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, piv]] = M[[piv, c]]
        for r in range(c + 1, 6):
            M[r] = M[r] - M[c] * (M[r, c] / M[c, c])
    x = np.zeros(6, dtype=ld)
    for c in range(5, -1, -1):
        x[c] = (M[c, 6] - (M[c, c + 1:6] * x[c + 1:]).sum()) / M[c, c]
    h = x[:3] / ld(2)
    q = np.concatenate((np.array([ld(1)]), h)) / np.sqrt(ld(1) + (h * h).sum())
    w_, x_, y_, z_ = q
    dR = np.array([[1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - w_ * z_), 2 * (x_ * z_ + w_ * y_)],
                   [2 * (x_ * y_ + w_ * z_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ - w_ * x_)],
                   [2 * (x_ * z_ - w_ * y_), 2 * (y_ * z_ + w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)]], dtype=ld)
    Pm = np.asarray(pose, dtype=ld).reshape(3, 4)
    out = dR @ Pm
    out[:, 3] += x[3:]
    return out.astype(np.float64).reshape(12)


def test_corner_registration_recovers_the_written_down_transform():
    g = np.random.default_rng(7)
    b, nb = _corner(g, 20)
    Rt, tt = _rodrigues(CORNER_W), np.array(CORNER_T)
    a = ((b.astype(np.float64) - tt) @ Rt).astype(f32)      # p_B = Rt p_A + tt
    dmax = [0.5] * 11
    eye = np.eye(3, 4).reshape(12)
    r = R.icp_pair(a, b, nb, eye, dmax, 6)
    ext = eye.copy()
    for s in range(10):
        ss, _ = R.one_pass(ext, a, 1.0, b, 1.0, nb, dmax[s])
        ext = _solve_extended(ss, ext)
    e_deg, e_m = R.pose_error(r["pose"], Rt, tt)
    x_deg, x_m = R.pose_error(ext, Rt, tt)
    print(f"MEASURE icp/corner restatement {e_deg:.3e} deg {e_m:.3e} m; extended-precision solve {x_deg:.3e} deg {x_m:.3e} m "
          f"(recorded {CORNER_EXT_DEG:.1e} deg {CORNER_EXT_M:.1e} m, gates 10 x)")
    assert r["info"].tolist() == [1, 10, 0, len(a)] and (r["nn"] >= 0).all()
    assert x_deg <= 2 * CORNER_EXT_DEG and x_m <= 2 * CORNER_EXT_M      # the recorded figures are what the extended solve shows
    assert e_deg <= 10 * CORNER_EXT_DEG and e_m <= 10 * CORNER_EXT_M
    assert R.rms(r["sums"][-1]) < 1e-3 and R.rms(r["sums"][0]) > 0.02      # the residual goes from centimetres to the quantisation step


def test_single_plane_is_refused_at_every_step():
    g = np.random.default_rng(8)
    b, nb = _corner(g, 20)
    keep = nb[:, 2] == 1
    plane, npl = b[keep], nb[keep]
    start = _small_pose(g, 0.02, 0.05)
    r = R.icp_pair(plane, plane, npl, start, [0.5] * 6, 6)
    assert r["info"].tolist()[:3] == [1, 0, 5] and r["info"][3] > 300
    assert r["pose"].tobytes() == start.tobytes()
    assert (r["sums"] == r["sums"][0]).all()      # the pose never moved: every pass is the first


# ---- 5. quality on the street scenes -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def street():
    """(true results, false results) of the restatement on true_pair(0..11) and false_pair(0..5) at N = 4096"""
    dmax = [QUALITY_SEARCH["dmax"]] * (QUALITY_SEARCH["iterations"] + 1)
    true, false = [], []
    for seed in range(12):
        a, b, Rt, tt, start = R.tilted_true_pair(seed)
        nb, _ = R.point_normals(b, R.knn_lists(b, QUALITY_SEARCH["k"]))
        r = R.icp_pair(a, b, nb, start, dmax, QUALITY_SEARCH["min_inliers"])
        true.append(dict(r, start_err=R.pose_error(start, Rt, tt), err=R.pose_error(r["pose"], Rt, tt)))
    for seed in range(6):
        a, b = AR.false_pair(seed)
        nb, _ = R.point_normals(b, R.knn_lists(b, QUALITY_SEARCH["k"]))
        false.append(R.icp_pair(a, b, nb, np.eye(3, 4).reshape(12), dmax, QUALITY_SEARCH["min_inliers"]))
    return true, false


def test_quality_on_street_scenes(street):
    true, false = street
    for i, r in enumerate(true):
        print(f"MEASURE icp/quality true_pair({i}) start {r['start_err'][0]:.2f} deg {r['start_err'][1]:.3f} m -> {r['err'][0]:.3f} deg "
              f"{r['err'][1]:.3f} m  inliers {r['info'][3]} rms {R.rms(r['sums'][-1]):.4f} m  steps {r['info'][1]}")
    for i, r in enumerate(false):
        print(f"MEASURE icp/quality false_pair({i}) inliers {r['info'][3]} rms {R.rms(r['sums'][-1]):.4f} m")
    worst_deg, worst_m = max(r["err"][0] for r in true), max(r["err"][1] for r in true)
    print(f"MEASURE icp/quality worst {worst_deg:.3f} deg {worst_m:.3f} m; recorded {QUALITY_MEASURED_DEG} deg {QUALITY_MEASURED_M} m, "
          f"gates {QUALITY_GATE_DEG:.3f} deg {QUALITY_GATE_M:.4f} m")
    assert max(r["start_err"][0] for r in true) > 3.0 and max(r["start_err"][1] for r in true) > 0.4      # the starts are bad
    assert worst_deg < QUALITY_GATE_DEG and worst_m < QUALITY_GATE_M
    assert worst_deg > QUALITY_MEASURED_DEG / 1.5 and worst_m > QUALITY_MEASURED_M / 1.5      # the record is the measurement
    assert all(r["info"][1] == QUALITY_SEARCH["iterations"] for r in true)


def test_true_and_false_pairs_separate(street):
    true, false = street
    share_t, share_f = [r["info"][3] / 4096 for r in true], [r["info"][3] / 4096 for r in false]
    rms_t, rms_f = [R.rms(r["sums"][-1]) for r in true], [R.rms(r["sums"][-1]) for r in false]
    print(f"MEASURE icp/quality inlier_share true min {min(share_t):.3f} false max {max(share_f):.3f}; rms true max {max(rms_t):.4f} m "
          f"false min {min(rms_f):.4f} m")
    assert min(share_t) > max(share_f)
    assert max(rms_t) < min(rms_f)


# ---- 6. validation -----------------------------------------------------------------------------------------------------------------
def test_refine_search_rules():
    s = verify.RefineSearch()
    assert (s.k, s.dmax, s.iterations, s.min_inliers, s.final_dmax) == (16, (1.0,) * 8, 8, 32, 1.0) and s.schedule == (1.0,) * 9
    assert verify.RefineSearch(dmax=[2.0, 1.0, 0.5], iterations=3).schedule == (2.0, 1.0, 0.5, 0.5)
    assert verify.RefineSearch(dmax=(2.0, 1.0), iterations=2, final_dmax=0.25).schedule == (2.0, 1.0, 0.25)
    assert verify.RefineSearch(iterations=0, dmax=0.75).schedule == (0.75,)
    assert s == verify.RefineSearch() and hash(s) == hash(verify.RefineSearch()) and s != verify.RefineSearch(k=8) and "dmax" in repr(s)
    with pytest.raises(AttributeError):
        s.k = 3
    with pytest.raises(AttributeError):
        del s.k
    for kw in (dict(k=3), dict(k=65), dict(k=16.0), dict(k=True), dict(dmax=0.0), dict(dmax=-1.0), dict(dmax=16.5), dict(dmax=float("nan")),
               dict(dmax=float("inf")), dict(dmax="1"), dict(dmax=[1.0, 1.0]), dict(dmax=[1.0] * 7 + [0.0]), dict(dmax=1e-50), dict(iterations=-1),
               dict(iterations=65), dict(iterations=2.0), dict(min_inliers=5), dict(min_inliers=1 << 31), dict(final_dmax=0.0),
               dict(final_dmax=17.0), dict(final_dmax=float("nan")), dict(iterations=0, dmax=[])):
        with pytest.raises(ValueError):
            verify.RefineSearch(**kw)
    with pytest.raises(TypeError):
        verify.refine_pairs(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 2, dtype=torch.int32), search=dict(k=16))
    with pytest.raises(TypeError):
        verify.refine_candidates(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), torch.zeros(1, 1, dtype=torch.int32), refine=dict(k=16))


def test_point_normals_argument_errors_are_raised_on_the_host():
    x, idx = torch.zeros(2 * 16, 3), torch.zeros(2, 16, 8, dtype=torch.int32)
    for args, err in (((x.double(), idx, 2, 16), TypeError), ((x, idx.long(), 2, 16), TypeError), ((x.numpy(), idx, 2, 16), TypeError),
                      ((x, idx, 3, 16), ValueError), ((x, idx, 0, 16), ValueError), ((x[:, :2], idx, 2, 16), ValueError),
                      ((x, idx[:, :, :3], 2, 16), ValueError), ((x, idx[0], 2, 16), ValueError), ((x, torch.zeros(2, 16, 65, dtype=torch.int32), 2, 16), ValueError),
                      ((torch.zeros(2 * 4, 3), torch.zeros(2, 4, 5, dtype=torch.int32), 2, 4), ValueError),
                      ((torch.zeros(3, 2 * 16).t(), idx, 2, 16), ValueError)):
        with pytest.raises(err):
            ops.point_normals(*args)
    with pytest.raises(LpdHipError):      # everything is right but the device: no CPU path
        ops.point_normals(x, idx, 2, 16)
    with pytest.raises(ValueError):
        verify.point_normals(torch.zeros(2, 16, 3), k=17)
    with pytest.raises(ValueError):
        verify.point_normals(torch.zeros(2, 16, 3), k=3)


def test_icp_pairs_argument_errors_are_raised_on_the_host():
    a, b, nb = torch.zeros(2, 16, 3), torch.zeros(3, 16, 3), torch.zeros(3, 16, 3)
    pairs, pose = torch.zeros(4, 2, dtype=torch.int32), torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(4, 1)
    good = dict(a=a, b=b, normals_b=nb, pairs=pairs, pose=pose, dmax=[1.0, 1.0], min_inliers=6)
    bad = [(dict(a=a.double()), TypeError), (dict(normals_b=nb.double()), TypeError), (dict(pairs=pairs.long()), TypeError), (dict(pose=pose.float()), TypeError),
           (dict(scale_a=torch.zeros(2, dtype=torch.float64)), TypeError), (dict(pose=None), TypeError), (dict(dmax=1.0), TypeError),
           (dict(b=torch.zeros(3, 17, 3)), ValueError), (dict(a=torch.zeros(2, 16, 4)), ValueError), (dict(a=torch.zeros(2, 16385, 3), b=torch.zeros(3, 16385, 3)), ValueError),
           (dict(normals_b=torch.zeros(2, 16, 3)), ValueError), (dict(normals_b=torch.zeros(3, 16, 4)), ValueError), (dict(pairs=torch.zeros(4, 3, dtype=torch.int32)), ValueError),
           (dict(pairs=torch.zeros(0, 2, dtype=torch.int32)), ValueError), (dict(pose=pose[:3]), ValueError), (dict(pose=pose.reshape(4, 3, 4)), ValueError),
           (dict(scale_a=torch.ones(3)), ValueError), (dict(scale_b=torch.ones(2)), ValueError), (dict(dmax=[]), ValueError), (dict(dmax=[1.0] * 66), ValueError),
           (dict(dmax=[1.0, 0.0]), ValueError), (dict(dmax=[1.0, 16.5]), ValueError), (dict(dmax=[float("nan")]), ValueError), (dict(dmax=[float("inf"), 1.0]), ValueError),
           (dict(dmax=[1e-50]), ValueError), (dict(min_inliers=5), ValueError), (dict(min_inliers=6.5), ValueError), (dict(min_inliers=True), ValueError)]
    for change, err in bad:
        with pytest.raises(err):
            ops.icp_pairs(**dict(good, **change))
    with pytest.raises(LpdHipError):      # everything is right but the device: no CPU path
        ops.icp_pairs(**good)
    assert ops.icp_dmax([0.5, 16.0], 1)[1] == 16.0
    for init, err in ((torch.zeros(4, 12), TypeError), (torch.zeros(4, 11, dtype=torch.float64), ValueError), (torch.zeros(3, 12, dtype=torch.float64), ValueError),
                      ("identity", TypeError)):
        with pytest.raises(err):
            verify.refine_pairs(a, b, pairs, init=init)
