"""CPU side of the drive step (lpd_drive_steps / lpd_drive_plan / lpd_drive_rows, lpdnet_hip/drive.py): the kernels' arithmetic header
(csrc/lpd_drive_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/drive_ref.py) value for value
and decision for decision, the distances and window counts against Python integers, hand-made drives whose windows can be written
down, the fp32 error against extended precision at UTM scale, argument validation, load_poses and the no-GPU errors.  The kernels
themselves are tested on the GPU (tests/test_drive_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import drive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32 = np.float32
U = R.UNITS

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_drive_math.h"
// <mode> <in> <out> <n>: an optional table, then n fixed-size records in; n fixed-size records out
//   quant   1 f64                                      -> 1 i64
//   step    6 f64 (t_prev, t_cur)                      -> 1 f64 (the length) + 1 i64
//   lb      table: i64 S, D [S] i64;  1 i64 (v)        -> 1 i64
//   window  table: i64 S, D [S] i64;  3 i64 (L T w)    -> 4 i64 (first end ref count)
//   scan    table: i64 n, offsets [n] i32 (+ pad to 8); 3 i64 (lo hi g) -> 1 i64
//   rel     24 f64 (P_i, P_ref) + 1 i64 (frame)        -> 12 f32 (M rows, u)
//   coord   15 f32 (M rows, u, x y z)                  -> 3 f32
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) return 3;
    fseek(fi, 0, SEEK_END);
    const long size = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    std::vector<unsigned char> in((size_t)size);
    if (fread(in.data(), 1, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    size_t rin = 0, rout = 0, at = 0;
    std::vector<int64_t> D;
    std::vector<int32_t> off;
    if (!strcmp(mode, "quant")) { rin = 8; rout = 8; }
    else if (!strcmp(mode, "step")) { rin = 48; rout = 16; }
    else if (!strcmp(mode, "lb") || !strcmp(mode, "window")) {
        int64_t S;
        memcpy(&S, in.data(), 8);
        D.resize((size_t)S);
        memcpy(D.data(), in.data() + 8, (size_t)S * 8);
        at = 8 + (size_t)S * 8;
        rin = !strcmp(mode, "lb") ? 8 : 24;
        rout = !strcmp(mode, "lb") ? 8 : 32;
    } else if (!strcmp(mode, "scan")) {
        int64_t m;
        memcpy(&m, in.data(), 8);
        off.resize((size_t)m);
        memcpy(off.data(), in.data() + 8, (size_t)m * 4);
        at = 8 + (((size_t)m * 4 + 7) & ~(size_t)7);
        rin = 24; rout = 8;
    } else if (!strcmp(mode, "rel")) { rin = 200; rout = 48; }
    else if (!strcmp(mode, "coord")) { rin = 60; rout = 12; }
    else return 2;
    if (in.size() != at + n * rin) return 5;
    std::vector<unsigned char> out(n * rout);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char* r = &in[at + i * rin];
        unsigned char* o = &out[i * rout];
        if (!strcmp(mode, "quant")) {
            double v;
            memcpy(&v, r, 8);
            const int64_t q = lpd_drive_quant(v);
            memcpy(o, &q, 8);
        } else if (!strcmp(mode, "step")) {
            double t[6], a[12] = {0}, b[12] = {0};
            memcpy(t, r, 48);
            a[3] = t[0]; a[7] = t[1]; a[11] = t[2]; b[3] = t[3]; b[7] = t[4]; b[11] = t[5];
            const double dl = lpd_drive_step_length(a, b);
            const int64_t q = lpd_drive_step(a, b);
            memcpy(o, &dl, 8); memcpy(o + 8, &q, 8);
        } else if (!strcmp(mode, "lb")) {
            int64_t v;
            memcpy(&v, r, 8);
            const int64_t got = lpd_drive_lower_bound(D.data(), (int)D.size(), v);
            memcpy(o, &got, 8);
        } else if (!strcmp(mode, "window")) {
            int64_t a[3];
            memcpy(a, r, 24);
            const LpdDriveWindow w = lpd_drive_window(D.data(), (int)D.size(), a[0], a[1], a[2]);
            const int64_t got[4] = {w.first, w.end, w.ref, lpd_drive_window_count(D.back(), a[0], a[1])};
            memcpy(o, got, 32);
        } else if (!strcmp(mode, "scan")) {
            int64_t a[3];
            memcpy(a, r, 24);
            const int64_t got = lpd_drive_scan_of(off.data(), (int)a[0], (int)a[1], a[2]);
            memcpy(o, &got, 8);
        } else if (!strcmp(mode, "rel")) {
            double P[24];
            int64_t frame;
            memcpy(P, r, 192); memcpy(&frame, r + 192, 8);
            const LpdDriveRel q = lpd_drive_rel(P, P + 12, (int)frame);
            memcpy(o, q.m, 36); memcpy(o + 36, q.u, 12);
        } else {
            float f[15];
            memcpy(f, r, 60);
            const float got[3] = {lpd_drive_coord(f + 0, f[9], f[12], f[13], f[14]), lpd_drive_coord(f + 3, f[10], f[12], f[13], f[14]),
                                  lpd_drive_coord(f + 6, f[11], f[12], f[13], f[14])};
            memcpy(o, got, 12);
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
    d = tmp_path_factory.mktemp("drive_math")
    src = d / "drive_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "drive_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, raw, n, dtype):
        (d / "in.bin").write_bytes(raw)
        r = subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(n)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        return np.fromfile(d / "out.bin", dtype=dtype)
    return run


def _table(D):
    D = np.asarray(D, dtype=np.int64)
    return np.int64(len(D)).tobytes() + D.tobytes()


def _host_windows(host, D, L, T, ws):
    rec = np.array([[L, T, w] for w in ws], dtype=np.int64)
    return host("window", _table(D) + rec.tobytes(), len(rec), np.int64).reshape(-1, 4)


# ---- 1. steps ----

def test_quantisation_on_the_host_equals_the_restatement(host):
    g = np.random.default_rng(2)
    v = list(g.uniform(0.0, 30.0, 4000)) + list(g.uniform(0.0, 1e-4, 500)) + list(10.0 ** g.uniform(-12, 12, 500))
    for k in (0, 1, 2, 3, 655360, 1310720, (1 << 36) - 1, 1 << 36, (1 << 36) + 1):      # rounding boundaries (k + 0.5) / 65536 and neighbours
        b = np.float64(k + 0.5) / np.float64(U)
        v += [b, np.nextafter(b, np.inf), np.nextafter(b, -np.inf), np.float64(k) / U]
    v += [0.0, -0.0, np.nan, np.inf, -np.inf, -1.0, 1e300, 1.7976931348623157e308, 5e-324, (1 << 20) + 0.25]
    v = np.array(v, dtype=np.float64)
    got = host("quant", v.tobytes(), len(v), np.int64)
    want = R.quant(v)
    assert np.array_equal(got, want)
    assert want.min() == 0 and want.max() == 1 << 36
    # half to even, as Python rounds
    for x, q in zip(v, want):
        if np.isfinite(x) and 0 <= x < 1e6:
            assert int(q) == round(float(x) * U), x


def test_step_lengths_on_the_host_equal_the_restatement(host):
    g = np.random.default_rng(3)
    n = 3000
    a = g.normal(0, 1, (n, 3)) * np.array([5.7e6, 6.2e5, 100.0])
    step = g.normal(0, 1, (n, 3)) * (10.0 ** g.uniform(-6, 3, (n, 1)))
    b = a + step
    L, T = 20.0, 10.0
    exact = np.array([[0, 0, 0, L, 0, 0], [1, 2, 3, 1, 2 + L / 2, 3], [5.7e6, 6.2e5, 0, 5.7e6 + T, 6.2e5, 0], [0, 0, 0, 3 * 4, 4 * 4, 0],
                      [0, 0, 0, np.nan, 0, 0], [0, 0, 0, np.inf, 0, 0], [np.inf, 0, 0, np.inf, 0, 0], [0, 0, 0, 1e200, 1e200, 0],
                      [0, 0, 0, 0, 0, 0]], dtype=np.float64)
    rec = np.concatenate((np.concatenate((a, b), 1), exact))
    got = host("step", rec.tobytes(), len(rec), np.uint8).reshape(len(rec), 16)
    got_dl, got_q = got[:, :8].copy().view(np.float64)[:, 0], got[:, 8:].copy().view(np.int64)[:, 0]
    want_dl = np.empty(len(rec))
    want_q = np.empty(len(rec), dtype=np.int64)
    for i, r in enumerate(rec):
        P = np.zeros((2, 12))
        P[0, [3, 7, 11]], P[1, [3, 7, 11]] = r[:3], r[3:]
        want_dl[i] = R.step_lengths(P)[1]
        want_q[i] = R.steps(P)[1]
    assert np.array_equal(got_dl.view(np.uint64), want_dl.view(np.uint64))
    assert np.array_equal(got_q, want_q)
    k = len(a)
    assert list(want_q[k:k + 4]) == [int(L * U), int(L * U) // 2, int(T * U), 20 * U]      # steps of exactly L, L/2, T and a 3-4-5 step
    assert list(want_q[k + 4:]) == [0, 0, 0, 0, 0]      # NaN, inf, inf - inf, an overflowing square (inf), no step


def test_distance_and_window_count_against_python_integers(host):
    g = np.random.default_rng(4)
    q = R.quant(g.uniform(0.0, 3.0, 5000))
    D = R.distance(q)
    total = 0
    for i, v in enumerate(q.tolist()):
        total += v
        assert int(D[i]) == total
    rec, want = [], []
    for _ in range(300):
        L, T = int(g.integers(1, 40 * U)), int(g.integers(1, 40 * U))
        rec.append((L, T, 0))
        want.append(sum(1 for w in range(0, total // T + 2) if w * T + L <= total))
    for L, T in ((total, 1), (total + 1, 1), (total, total), (1, total), (1, 1 << 40)):
        rec.append((L, T, 0))
        want.append(sum(1 for w in range(0, min(total // T + 2, 10)) if w * T + L <= total) if T > 1 else max(total - L + 1, 0))
    got = host("window", _table(D) + np.array(rec, dtype=np.int64).tobytes(), len(rec), np.int64).reshape(-1, 4)[:, 3]
    assert got.tolist() == want == [R.window_count(total, L, T) for L, T, _ in rec]


# ---- 3. windows ----

def test_lower_bounds_and_windows_on_the_host_equal_the_restatement(host):
    g = np.random.default_rng(5)
    for S, zero_share in ((1, 0.0), (2, 0.0), (37, 0.3), (1000, 0.1), (1000, 0.9)):
        q = R.quant(g.uniform(0.0, 2.0, S))
        q[g.uniform(0, 1, S) < zero_share] = 0
        q[0] = 0
        D = R.distance(q)
        vs = np.concatenate((D, D + 1, D - 1, g.integers(-5, int(D[-1]) + 5, 200), [0, -1, int(D[-1]) + 1, 1 << 62]))
        got = host("lb", _table(D) + vs.astype(np.int64).tobytes(), len(vs), np.int64)
        assert got.tolist() == [R.lower_bound(D, int(v)) for v in vs]
        for L, T in ((4 * U, 2 * U), (4 * U, 4 * U), (3 * U, U), (U, 3 * U), (7, 3), (20 * U + 1, 10 * U)):
            W = R.window_count(D[-1], L, T)
            ws = list(range(0, min(W, 400))) + [W, W + 1, W + 1000]
            got = _host_windows(host, D, L, T, ws)
            assert [tuple(r[:3]) for r in got.tolist()] == [R.window(D, L, T, w) for w in ws]
            for first, end, ref, _ in got.tolist():
                assert (first == end and ref == -1) or first <= ref < end <= S


def test_window_bounds_hold_on_a_table_that_does_not_ascend(host):
    g = np.random.default_rng(6)
    D = g.integers(-(1 << 40), 1 << 40, 500)
    rec = [(int(g.integers(1, 1 << 30)), int(g.integers(1, 1 << 30)), int(g.integers(0, 1 << 12))) for _ in range(500)]
    got = host("window", _table(D) + np.array(rec, dtype=np.int64).tobytes(), len(rec), np.int64).reshape(-1, 4)
    for first, end, ref, _ in got.tolist():
        assert 0 <= first <= end <= 500 and ((first == end and ref == -1) or first <= ref < end)


def test_scan_of_a_row_on_the_host_equals_the_restatement(host):
    g = np.random.default_rng(7)
    lengths = g.integers(0, 6, 300)
    lengths[[10, 11, 12, 299]] = 0
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    rec, want = [], []
    for _ in range(2000):
        lo = int(g.integers(0, 300))
        hi = int(g.integers(lo + 1, 301))
        if off[hi] == off[lo]:
            continue
        row = int(g.integers(off[lo], off[hi]))
        rec.append((lo, hi, row))
        want.append(R.scan_of(off, row))
    raw = np.int64(len(off)).tobytes() + off.tobytes() + b"\0" * ((-len(off) * 4) % 8) + np.array(rec, dtype=np.int64).tobytes()
    got = host("scan", raw, len(rec), np.int64)
    assert got.tolist() == want
    assert all(off[i] <= r < off[i + 1] for i, (_, _, r) in zip(want, rec))


def _line(steps):
    """a straight drive along x with the given steps -> poses [S, 12]"""
    x = np.concatenate(([0.0], np.cumsum(np.asarray(steps, dtype=np.float64))))
    P = np.zeros((len(x), 12))
    P[:, [0, 5, 10]] = 1.0
    P[:, 3] = x
    return P


HAND_MADE = {
    # name: (steps, length, stride, the windows (first, end, ref) written down by hand)
    "unit steps, stride 2": ([1] * 10, 4.0, 2.0, [(0, 4, 2), (2, 6, 4), (4, 8, 6), (6, 10, 8)]),
    "unit steps, stride 4": ([1] * 10, 4.0, 4.0, [(0, 4, 2), (4, 8, 6)]),
    "stride > length": ([1] * 10, 2.0, 5.0, [(0, 2, 1), (5, 7, 6)]),      # scans 2, 3, 4, 7, 8, 9, 10 lie in no window
    "stride = length / 3": ([1] * 10, 3.0, 1.0, [(w, w + 3, w + 2) for w in range(8)]),      # scan 2 .. 7 lie in three windows
    "stationary stretch": ([1, 1, 0, 0, 0, 1, 1, 1, 1], 2.0, 1.0, [(0, 2, 1), (1, 6, 2), (2, 7, 6), (6, 8, 7), (7, 9, 8)]),
    "a step longer than length": ([1, 1, 10, 1, 1], 2.0, 2.0, [(0, 2, 1), (2, 3, 2), (3, 3, -1), (3, 3, -1), (3, 3, -1), (3, 3, -1), (3, 5, 4)]),
    "one scan": ([], 2.0, 1.0, []),
}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_drives(host, name):
    steps, length, stride, want = HAND_MADE[name]
    P = _line(steps)
    D = R.distance(R.steps(P))
    assert D.tolist() == [int(v * U) for v in np.concatenate(([0.0], np.cumsum(steps)))]
    L, T = R.units(length), R.units(stride)
    W = R.window_count(D[-1], L, T)
    assert W == len(want)
    assert [R.window(D, L, T, w) for w in range(W)] == want
    S = len(P)
    got = _host_windows(host, D, L, T, list(range(W + 2)))
    assert [tuple(r[:3]) for r in got.tolist()] == want + [(S, S, -1)] * 2 and set(got[:, 3].tolist()) == {W}
    table, position = R.plan(D, np.arange(S + 1) * 3, P, L, T, 0, W + 1)
    assert table[:, 3].tolist() == [3 * (e - f) for f, e, _ in want] + [0]
    assert position[:, 0].tolist() == [float(P[r, 3]) if r >= 0 else 0.0 for _, _, r in want] + [0.0]
    if name == "stationary stretch":      # equal D: the whole run 2 .. 5 is in the same windows
        member = [{w for w, (f, e, _) in enumerate(want) if f <= i < e} for i in range(2, 6)]
        assert member[0] == member[1] == member[2] == member[3] == {1, 2}
    if name == "stride = length / 3":
        assert sum(f <= 4 < e for f, e, _ in want) == 3
    if name == "stride > length":
        assert not any(f <= 3 < e for f, e, _ in want)


# ---- 5. / 6. relative pose and rows ----

def _random_poses(g, n, scale):
    _, P = R.make_drive(g, [0] * n, step=g.uniform(0.0, 3.0, n - 1), heading_noise=0.3, origin=scale)
    return P


def test_relative_pose_and_rows_on_the_host_equal_the_restatement(host):
    g = np.random.default_rng(8)
    P = np.concatenate((_random_poses(g, 200, (0.0, 0.0, 0.0)), _random_poses(g, 200, (5.7e6, 6.2e5, 80.0))))
    bad = P[:6].copy()
    bad[0, 3], bad[1, 0], bad[2, 7], bad[3, 5] = np.nan, np.inf, -np.inf, np.nan
    bad[4, :] = 1e200
    bad[5, :] = 0.0
    P = np.concatenate((P, bad))
    pairs = [(int(a), int(b)) for a, b in zip(g.integers(0, 200, 300), g.integers(0, 200, 300))]
    pairs += [(int(a) + 200, int(b) + 200) for a, b in zip(g.integers(0, 200, 300), g.integers(0, 200, 300))]
    pairs += [(400 + k, 7) for k in range(6)] + [(7, 400 + k) for k in range(6)] + [(i, i) for i in (0, 250, 400, 404)]
    rec = b"".join(P[i].tobytes() + P[r].tobytes() + np.int64(frame).tobytes() for i, r in pairs for frame in (0, 1))
    got = host("rel", rec, 2 * len(pairs), np.uint32).reshape(-1, 12)
    want = []
    for i, r in pairs:
        for frame in (0, 1):
            M, u = R.rel(P[i], P[r], frame)
            want.append(np.concatenate((M.reshape(9), u)))
    want = np.array(want, dtype=f32)
    assert np.array_equal(got, want.view(np.uint32))
    assert np.isnan(want).any() and np.isinf(want).any()

    xyz = (g.uniform(-1, 1, (len(want), 3)) * 80.0).astype(f32)
    xyz[5], xyz[6], xyz[7] = (np.nan, 1, 2), (np.inf, 1, 2), (0, -np.inf, 0)
    rows = host("coord", np.concatenate((want, xyz), 1).astype(f32).tobytes(), len(want), np.uint32).reshape(-1, 3)
    ref = np.concatenate([R.transform(m[:9].reshape(3, 3), m[9:], x[None]) for m, x in zip(want, xyz)])
    assert np.array_equal(rows, ref.view(np.uint32))


def _signed_permutations(g, n):
    out = []
    for _ in range(n):
        M = np.zeros((3, 3))
        M[np.arange(3), g.permutation(3)] = g.choice([-1.0, 1.0], 3)
        out.append(M)
    return out


def test_reference_scan_rows_are_bit_copies_under_signed_permutations():
    g = np.random.default_rng(9)
    S, n = 24, 5
    P = np.zeros((S, 12))
    for i, M in enumerate(_signed_permutations(g, S)):
        P[i] = np.concatenate((M, np.array([[5.7e6 + 0.9 * i], [6.2e5 - 0.3 * i], [70.0]])), 1).reshape(12)
    pts = (g.uniform(-1, 1, (S * n, 3)) * 50.0).astype(f32)
    d = R.drive(pts, [n] * S, P, 4.0, 2.0, 1)
    assert d["W"] >= 3
    for w, (first, end, ref, _) in enumerate(d["plan"]):
        at = int(d["out_off"][w]) + (ref - first) * n
        assert np.array_equal(d["out"][at:at + n].view(np.uint32), pts[ref * n:(ref + 1) * n].view(np.uint32))


def test_fp32_rows_against_extended_precision_at_utm_scale():
    """Coordinates stay below 256 m after the subtraction, where an fp32 ulp is 1.5e-5 m; three products, three sums and the rounding of
    M and u: a few ulp.  Asserted at 1e-3 m."""
    g = np.random.default_rng(10)
    S, n = 120, 40
    pts, P = R.make_drive(g, [n] * S, step=g.uniform(0.2, 1.2, S - 1), heading_noise=0.05, origin=(5.7e6, 6.2e5, 80.0), point_scale=60.0)
    worst = 0.0
    for frame in (0, 1):
        d = R.drive(pts, [n] * S, P, 20.0, 10.0, frame)
        assert d["W"] >= 4
        ext = R.rows_extended(pts, d["offsets"], P, d["plan"], frame)
        err = float(np.abs(d["out"].astype(np.longdouble) - ext).max())
        assert float(np.abs(ext).max()) < 256.0
        print(f"MEASURE drive fp32 vs extended precision, frame {frame}: max |error| = {err:.3e} m over {len(ext)} rows")
        worst = max(worst, err)
    assert worst < 1e-3


# ---- the Python surface ----

def test_argument_validation_and_the_no_gpu_errors(tmp_path):
    from lpdnet_hip import LpdHipError, drive, ops
    assert ops.drive_units(20.0, "length") == 20 * U == R.units(20.0)
    assert ops.drive_units(1.5 / U, "x") == 2 and ops.drive_units(2.5 / U, "x") == 2      # half to even, as the definition's rint
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-9, 2.0 ** 25):
        with pytest.raises(ValueError):
            ops.drive_units(bad, "length")
    P = np.zeros((5, 12))
    for bad in (np.zeros((5, 11)), np.zeros((0, 12)), np.zeros((5, 12), dtype=np.float32), np.zeros((5, 2, 4))):
        with pytest.raises(ValueError):
            drive.plan_windows(bad, device="cuda")
    with pytest.raises(LpdHipError):
        drive.plan_windows(P, device="cpu")
    with pytest.raises(LpdHipError):
        ops.drive_distance(torch.zeros((5, 12), dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.drive_distance(None)
    pts = np.zeros((10, 3), dtype=f32)
    with pytest.raises(ValueError):
        drive.accumulate(pts, [2] * 5, P, frame="sensor")
    with pytest.raises(ValueError):
        drive._drive_input(pts, [2] * 4)      # lengths that do not sum to the rows
    with pytest.raises(ValueError):
        drive._lengths([2] * 4, 5, "accumulate")      # four lengths for five poses
    with pytest.raises(ValueError):
        drive._drive_input(pts, [-1, 11])
    with pytest.raises(TypeError):
        drive.accumulate(pts, [2] * 5)
    for kw in (dict(num_points=100), dict(window_batch=0), dict(window_batch=65536), dict(frame="x")):
        with pytest.raises(ValueError):
            drive.submaps_from_drive(pts, [2] * 5, P, **kw)
    with pytest.raises(TypeError):
        drive.submaps_from_drive(pts, [2] * 5, P, clean="road")
    with pytest.raises(LpdHipError):
        drive.submaps_from_drive(pts, [2] * 5, P, device="cpu")
    assert drive._window_range(None, 7) == (0, 7) and drive._window_range(range(2, 5), 7) == (2, 5) and drive._window_range((3, 3), 7) == (3, 3)
    for bad in ((5, 2), (0, 8), range(0, 6, 2)):
        with pytest.raises(ValueError):
            drive._window_range(bad, 7)


def test_load_poses(tmp_path):
    from lpdnet_hip import ingest
    g = np.random.default_rng(11)
    P = g.normal(0, 1, (7, 12)) * 1e6
    path = tmp_path / "poses.txt"
    path.write_text("# a comment\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in P) + "\n\n")
    got = ingest.load_poses(str(path))
    assert got.dtype == np.float64 and got.shape == (7, 12) and np.array_equal(got, P)
    assert np.array_equal(ingest.load_poses("poses.txt", str(tmp_path)), P)
    (tmp_path / "short.txt").write_text("1 2 3\n")
    (tmp_path / "word.txt").write_text(" ".join(["1"] * 11) + " x\n")
    (tmp_path / "none.txt").write_text("\n# nothing\n")
    for name in ("short.txt", "word.txt", "none.txt"):
        with pytest.raises(ValueError):
            ingest.load_poses(str(tmp_path / name))


def test_the_three_entry_points_are_declared_and_exported():
    from lpdnet_hip import _lib
    lib = _lib.load()
    for name, n_args in (("lpd_drive_steps", 4), ("lpd_drive_plan", 11), ("lpd_drive_rows", 13)):
        assert len(_lib.SIGNATURES[name]) == n_args and hasattr(lib, name)
