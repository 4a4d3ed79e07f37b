"""CPU side of the geometric verification (lpd_align_pairs, lpdnet_hip/verify.py): the kernel's arithmetic header
(csrc/lpd_align_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/align_ref.py) value for
value, the 128-bit shift against Python integers, hand-made clouds with their answers written down, the quality of the restatement
on labelled street scenes, and the validation of AlignSearch and ops.align_pairs.  The kernel itself is tested on the GPU
(tests/test_align_gpu.py)."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import align_ref as R
from lpdnet_hip import LpdHipError, _lib, ops, verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
MATH_H = os.path.join(CSRC, "lpd_align_math.h")
f32 = np.float32
INF = np.inf

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_align_math.h"
// <mode> <in> <out> <n>: n fixed-size records in, n fixed-size records out (every field 4 bytes)
//   cell   14 f32 (x y z sc c s has_t0 t0x t0y inv_cell z0 inv_zcell layers is_a)   -> 4 i32 (ix iy iz valid)
//   shift  4 u32 + 1 i32 (row, dx)                                                  -> 4 u32
//   score  8 u32 (a, b)                                                             -> 1 i32
//   key    7 i32 (score h dyi dxi nA S nB)                                          -> 2 u32 (key lo, hi) + 8 i32 (best)
//   rot    3 i32 (first h R)                                                        -> 1 i32
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    size_t rin = 0, rout = 0;
    if (!strcmp(mode, "cell")) { rin = 56; rout = 16; }
    else if (!strcmp(mode, "shift")) { rin = 20; rout = 16; }
    else if (!strcmp(mode, "score")) { rin = 32; rout = 4; }
    else if (!strcmp(mode, "key")) { rin = 28; rout = 40; }
    else if (!strcmp(mode, "rot")) { rin = 12; rout = 4; }
    else return 2;
    std::vector<unsigned char> in(n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 1, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t i = 0; i < n; ++i) {
        const unsigned char* r = &in[i * rin];
        unsigned char* o = &out[i * rout];
        if (!strcmp(mode, "cell")) {
            float f[14];
            memcpy(f, r, 56);
            const int layers = (int)f[12];
            const LpdAlignCell c = f[13] != 0.0f
                ? lpd_align_cell_a(f[0], f[1], f[2], f[3], f[4], f[5], f[6] != 0.0f, f[7], f[8], f[9], f[10], f[11], layers)
                : lpd_align_cell_b(f[0], f[1], f[2], f[3], f[9], f[10], f[11], layers);
            const int32_t v[4] = {c.ix, c.iy, c.iz, c.valid ? 1 : 0};
            memcpy(o, v, 16);
        } else if (!strcmp(mode, "shift")) {
            uint32_t a[4], s[4];
            int32_t dx;
            memcpy(a, r, 16);
            memcpy(&dx, r + 16, 4);
            lpd_align_shift128(a, dx, s);
            memcpy(o, s, 16);
        } else if (!strcmp(mode, "score")) {
            uint32_t a[8];
            memcpy(a, r, 32);
            const int32_t v = lpd_align_row_score(a, a + 4);
            memcpy(o, &v, 4);
        } else if (!strcmp(mode, "key")) {
            int32_t q[7], best[8];
            memcpy(q, r, 28);
            const unsigned long long k = lpd_align_key(q[0], q[1], q[2], q[3], q[4]);
            lpd_align_unkey(k, q[5], q[6], best);
            const uint32_t w[2] = {(uint32_t)k, (uint32_t)(k >> 32)};
            memcpy(o, w, 8);
            memcpy(o + 8, best, 32);
        } else {
            int32_t q[3];
            memcpy(q, r, 12);
            const int32_t v = lpd_align_rot_index(q[0], q[1], q[2]);
            memcpy(o, &v, 4);
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
    d = tmp_path_factory.mktemp("align_math")
    src = d / "align_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "align_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, records, out_bytes):
        (d / "in.bin").write_bytes(records.tobytes())
        n = len(records)
        r = subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(n)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        got = np.fromfile(d / "out.bin", dtype=np.uint8)
        assert got.size == n * out_bytes
        return got.reshape(n, out_bytes)
    return run


def _next(v, toward):
    return np.nextafter(f32(v), f32(toward))


def _cell_records():
    """(x y z sc c s has_t0 t0x t0y inv_cell z0 inv_zcell layers is_a) and the index of the first edge record"""
    g = np.random.default_rng(1)
    rot = R.rot_table(120)
    rec = []
    for _ in range(4000):      # random points around the grid and its layers, both clouds, with and without t0 and scale
        x, y = g.uniform(-40, 40, 2)
        z = g.uniform(-2, 10)
        c, s = rot[g.integers(0, 120)]
        rec.append([x, y, z, g.choice([1.0, 0.7, 25.0 / 0.9]) if g.random() < 0.5 else 1.0, c, s, float(g.random() < 0.5), g.uniform(-4, 4),
                    g.uniform(-4, 4), g.choice([2.0, 4.0, 1.0 / 0.3]), g.choice([0.0, -1.5]), g.choice([0.5, 1.0 / 1.5]), float(g.integers(1, 5)),
                    float(g.random() < 0.5)])
    edge = len(rec)
    ident = [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]      # sc c s has_t0 t0x t0y: the rotation by the table's entry 0 is exact
    # cell boundaries of the 0.5 m grid (inv_cell = 2): x exactly on k / 2 and one ulp either side, for both clouds; the grid's first
    # cell (x = -32), its last (x just under 32), fx = 128 exactly (x = 32)
    for is_a in (0.0, 1.0):
        for k in (-64, -63, -1, 0, 1, 7, 63, 64):
            for x in (k * 0.5, _next(k * 0.5, INF), _next(k * 0.5, -INF)):
                rec.append([x, 0.25, 1.0] + ident + [2.0, 0.0, 0.5, 4.0, is_a])
                rec.append([0.25, x, 1.0] + ident + [2.0, 0.0, 0.5, 4.0, is_a])
        # z exactly at z0, one ulp under it, at the top of the last layer (z0 + layers * z_cell) and one ulp under that; z0 = 0.5, so
        # that every z - z0 here is exact
        for layers in (1.0, 4.0):
            top = 0.5 + layers * 2.0
            for z in (0.5, _next(0.5, -INF), _next(0.5, INF), top, _next(top, -INF), _next(top, INF)):
                rec.append([0.25, 0.25, z] + ident + [2.0, 0.5, 0.5, layers, is_a])
        for v in (np.nan, INF, -INF, 1e30, -1e30, 3e38):      # no bit: the conversion to int is never reached
            rec += [[v, 0.25, 1.0] + ident + [2.0, 0.0, 0.5, 4.0, is_a], [0.25, v, 1.0] + ident + [2.0, 0.0, 0.5, 4.0, is_a],
                    [0.25, 0.25, v] + ident + [2.0, 0.0, 0.5, 4.0, is_a]]
        rec.append([INF, 0.25, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.5, 4.0, is_a])      # inf * 0 scale: NaN, and raw is not finite
    # cloud A alone: the 90-degree entry (0, 1) takes (x, y) to (-y, x) exactly; t0 moves a point across a boundary
    rec.append([3.25, -7.75, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.5, 4.0, 1.0])
    rec.append([0.25, 0.25, 1.0, 1.0, 1.0, 0.0, 1.0, 0.25, -0.25, 2.0, 0.0, 0.5, 4.0, 1.0])
    rec.append([0.25, 0.25, 1.0, 1.0, 1.0, 0.0, 1.0, 0.25 - 2.0 ** -10, -0.25 - 2.0 ** -10, 2.0, 0.0, 0.5, 4.0, 1.0])      # exact sums
    rec.append([0.25, 0.25, 1.0, 1.0, 1.0, 0.0, 1.0, np.nan, 0.0, 2.0, 0.0, 0.5, 4.0, 1.0])
    return np.array(rec, dtype=np.float32), edge


def _ref_cells(rec):
    out = np.zeros((len(rec), 4), dtype=np.int32)
    for i, r in enumerate(rec):
        cs = (r[4], r[5]) if r[13] != 0 else None
        t0 = (r[7], r[8]) if r[13] != 0 and r[6] != 0 else None
        ix, iy, iz, v = R.cells(r[None, :3], r[3], r[9], r[10], r[11], int(r[12]), cs, t0)
        out[i] = (ix[0], iy[0], iz[0], v[0])
    return out


def test_cells_on_the_host_equal_the_restatement(host):
    rec, edge = _cell_records()
    got = host("cell", rec, 16).view(np.int32)
    want = _ref_cells(rec)
    print(f"MEASURE align/cells {len(rec)} points, {int(want[:, 3].sum())} valid")
    assert np.array_equal(got, want)
    assert 0.1 < want[:edge, 3].mean() < 0.9
    # the answers written down, cloud B's block (the first after the random records)
    e = want[edge:]
    k = 0
    for cell_no in (-64, -63, -1, 0, 1, 7, 63, 64):      # x = k/2 on the boundary belongs to the cell above; one ulp under, the one below
        on, up, down = e[k], e[k + 2], e[k + 4]
        assert (on[3], up[3]) == (int(cell_no < 64), int(cell_no < 64)) and down[3] == int(cell_no > -64)
        if cell_no < 64:
            assert on[0] == cell_no + 64 == up[0] and on[1] == 64
        if cell_no > -64:
            assert down[0] == cell_no + 63
        assert e[k + 1][3] == on[3] and (e[k + 1][1] == on[0] or not on[3])      # the same along y
        k += 6
    assert [tuple(v) for v in e[k:k + 6]] == [(64, 64, 0, 1), (0, 0, 0, 0), (64, 64, 0, 1), (0, 0, 0, 0), (64, 64, 0, 1), (0, 0, 0, 0)]      # layers = 1
    k += 6
    assert [tuple(v) for v in e[k:k + 6]] == [(64, 64, 0, 1), (0, 0, 0, 0), (64, 64, 0, 1), (0, 0, 0, 0), (64, 64, 3, 1), (0, 0, 0, 0)]      # layers = 4
    k += 6
    assert not e[k:k + 19, 3].any()      # NaN, inf, 1e30, and inf times a zero scale
    assert want[-4].tolist() == [64 + 15, 64 + 6, 0, 1]         # (3.25, -7.75) -> (7.75, 3.25): cells 15 and 6
    assert want[-3].tolist() == [65, 64, 0, 1]                  # 0.25 + 0.25 = 0.5 exactly: the next cell; 0.25 - 0.25 = 0: cell 0
    assert want[-2].tolist() == [64, 63, 0, 1]                  # 2^-10 less: the cells below
    assert want[-1].tolist() == [0, 0, 0, 0]


def test_shift_and_row_score_against_python_integers(host):
    g = np.random.default_rng(2)
    rows = [g.integers(0, 1 << 32, 4, dtype=np.uint64).astype(np.uint32) for _ in range(60)]
    rows += [np.array(w, dtype=np.uint32) for w in ([0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 0], [0, 0, 0, 0x80000000], [0x80000000, 1, 0x80000000, 1])]
    shifts = list(range(-16, 17))
    rec = np.zeros((len(rows) * len(shifts), 5), dtype=np.uint32)
    k = 0
    for w in rows:
        for dx in shifts:
            rec[k, :4] = w
            rec[k, 4] = np.int32(dx).view(np.uint32)
            k += 1
    got = host("shift", rec, 16).view(np.uint32)
    k = 0
    for w in rows:
        v = R.row_int(w)
        for dx in shifts:
            assert got[k].tolist() == R.row_words(R.shift_int(v, dx)), (w, dx)
            k += 1
    for dx in (-16, -1, 0, 1, 16):      # a single bit at either end: it moves by dx or leaves the row
        assert R.shift_int(1, dx) == (1 << dx if dx >= 0 else 0) and R.shift_int(1 << 127, dx) == (1 << (127 + dx) if dx <= 0 else 0)
    pairs = np.array([np.concatenate((rows[i], rows[(i * 7 + 3) % len(rows)])) for i in range(len(rows))], dtype=np.uint32)
    sc = host("score", pairs, 4).view(np.int32)[:, 0]
    assert sc.tolist() == [bin(R.row_int(p[:4]) & R.row_int(p[4:])).count("1") for p in pairs]
    assert sc[61] == bin(R.row_int(rows[61]) & R.row_int(rows[(61 * 7 + 3) % len(rows)])).count("1") and max(sc) > 40


def test_key_orders_the_candidates_and_the_table_index_wraps(host):
    g = np.random.default_rng(3)
    rec = [[0, 0, 0, 0, 0, 0, 0], [16384, 1023, 32, 32, 16384, 16, 16384], [5, 0, 0, 0, 7, 8, 9], [5, 0, 0, 1, 7, 8, 9], [5, 0, 1, 0, 7, 8, 9],
           [5, 1, 0, 0, 3, 8, 9], [6, 1023, 16, 16, 1, 8, 9]]
    for _ in range(500):
        S = int(g.integers(0, 17))
        rec.append([int(g.integers(0, 16385)), int(g.integers(0, 1024)), int(g.integers(0, 2 * S + 1)), int(g.integers(0, 2 * S + 1)),
                    int(g.integers(0, 16385)), S, int(g.integers(0, 16385))])
    rec = np.array(rec, dtype=np.int32)
    got = host("key", rec, 40)
    keys = [int(lo) | (int(hi) << 32) for lo, hi in got[:, :8].copy().view(np.uint32)]
    best = got[:, 8:].copy().view(np.int32)
    for (score, h, dyi, dxi, nA, S, nB), b, k in zip(rec.tolist(), best.tolist(), keys):
        assert b == [h, dyi - S, dxi - S, score, nA, nB, 1, 0]
        assert k == (score << 36) | (((1 << 21) - 1 - ((h * 33 + dyi) * 33 + dxi)) << 15) | nA and k > 0
    # larger score first; then the smaller h, then the smaller dy, then the smaller dx -- whatever nA is
    assert keys[6] > keys[2] > keys[3] > keys[4] > keys[5]
    order = sorted(range(len(rec)), key=lambda i: (-rec[i][0], rec[i][1], rec[i][2], rec[i][3], -rec[i][4]))
    assert [keys[i] for i in order] == sorted(keys, reverse=True)
    q = np.array([[0, 0, 120], [119, 1, 120], [952, 16, 960], [-8, 3, 960], [-8, 8, 960], [2147483647, 1023, 8192], [-2147483648, 0, 7]], dtype=np.int32)
    ri = host("rot", q, 4).view(np.int32)[:, 0]
    assert ri.tolist() == [(f + h) % r for f, h, r in q.tolist()] == [R.rot_index(*r) for r in q.tolist()]
    assert ri[:5].tolist() == [0, 0, 8, 955, 0]


# ---- hand-made clouds, the answers written down ----
def _cloud(cells, n=None, z=1.0, cell=0.5):
    """one point at the middle of every (ix, iy) cell (indices relative to the grid's origin cell)"""
    p = np.array([[(ix + 0.5) * cell, (iy + 0.5) * cell, z] for ix, iy in cells], dtype=np.float32)
    if n is not None:
        p = np.concatenate((p, np.tile(p[:1], (n - len(p), 1))))
    return p


BLOB = [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (5, 3), (-7, 9), (-20, -11), (13, -30), (31, 17), (4, 4), (-3, -2)]


def test_hand_made_pairs():
    rot = R.rot_table(4)      # entries (1, 0), (0, 1), (-1, 0), (0, -1) up to the rounding of cos(pi / 2)
    rot[1], rot[3] = (0.0, 1.0), (0.0, -1.0)
    rot[2] = (-1.0, 0.0)
    a = _cloud(BLOB)
    # a cloud against itself: (0, 0, 0), score = nA = nB
    best, ys = R.align_pair(a, a, rot, 1, 2.0, 4, 0.0, 0.5, 4)
    assert best.tolist() == [0, 0, 0, 12, 12, 12, 1, 0] and ys.tolist() == [12]
    # ... against its copy moved by (3, -2) cells: dx = 3, dy = -2
    b = a + np.array([3 * 0.5, -2 * 0.5, 0.0], dtype=np.float32)
    best, _ = R.align_pair(a, b, rot, 1, 2.0, 4, 0.0, 0.5, 4)
    assert best.tolist() == [0, -2, 3, 12, 12, 12, 1, 0]
    assert R.score_slices(R.bitmap(a, 1.0, 2.0, 0.0, 0.5, 4, rot[0]), R.bitmap(b, 1.0, 2.0, 0.0, 0.5, 4), -2, 3) == 12
    # ... against its copy turned by exactly 90 degrees: the table entry (0, 1), h = 1
    b = np.column_stack((-a[:, 1], a[:, 0], a[:, 2])).astype(np.float32)
    best, ys = R.align_pair(a, b, rot, 4, 2.0, 2, 0.0, 0.5, 4)
    assert best.tolist() == [1, 0, 0, 12, 12, 12, 1, 0] and ys[1] == 12 and max(ys[0], ys[2], ys[3]) < 12
    # the tie rule: two identical, well separated blobs in B, one in A: both offsets score alike, the smaller (dy, dx) wins
    blob = [(0, 0), (1, 0), (0, 1), (2, 2), (3, 1)]
    a2 = _cloud(blob)
    b2 = _cloud([(x + 5, y - 4) for x, y in blob] + [(x - 6, y + 3) for x, y in blob])
    best, _ = R.align_pair(a2, b2, rot, 2, 2.0, 8, 0.0, 0.5, 4)
    assert best.tolist() == [0, -4, 5, 5, 5, 10, 1, 0]
    sc = R.scores_all(np.stack([R.bitmap(a2, 1.0, 2.0, 0.0, 0.5, 4, rot[0])]), R.bitmap(b2, 1.0, 2.0, 0.0, 0.5, 4), 8)[0]
    assert sc[-4 + 8, 5 + 8] == 5 == sc[3 + 8, -6 + 8] and (sc == 5).sum() == 2
    # ... and over h: the same blob at two yaws -- h = 0 wins over h = 2 (180 degrees of a point-symmetric cloud)
    sym = _cloud([(0, 0), (-1, -1), (3, 2), (-4, -3)])
    best, ys = R.align_pair(sym, sym, rot, 4, 2.0, 2, 0.0, 0.5, 4)
    assert best[:4].tolist() == [0, 0, 0, 4] and ys[2] == 4      # R(180) sends cell (i, j) to (-1 - i, -1 - j): the set is the same
    # an empty cloud (every point outside the grid): score 0, the winner is the first candidate (0, -S, -S)
    far = np.full((7, 3), 1000.0, dtype=np.float32)
    best, ys = R.align_pair(far, a, rot, 3, 2.0, 5, 0.0, 0.5, 4)
    assert best.tolist() == [0, -5, -5, 0, 0, 12, 1, 0] and ys.tolist() == [0, 0, 0]
    # the layers: the same plan-view cells at another height do not score
    best, _ = R.align_pair(a, a + np.array([0, 0, 2.0], dtype=np.float32), rot, 1, 2.0, 2, 0.0, 0.5, 4)
    assert best[3] == 0 and best[4] == 12 and best[5] == 12
    # rows outside every table are not read
    best, ys = R.align_pairs(a[None], a[None], [[0, 0], [1, 0], [0, -1]], rot, 2, 2.0, 1, 0.0, 0.5, 4)
    assert best[1:].tolist() == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 2 and not ys[1:].any() and best[0, 3] == 12


def test_slices_and_dot_products_agree():
    """the two ways the restatement counts a shift: a slice of the two bitmaps, and a window of the padded one"""
    a, b, _, _ = R.true_pair(0)
    rot = R.rot_table(120)
    occB = R.bitmap(b, 1.0, 2.0, 0.0, 0.5, 4)
    occA = np.stack([R.bitmap(a, 1.0, 2.0, 0.0, 0.5, 4, rot[h]) for h in (0, 37)])
    sc = R.scores_all(occA, occB, 16)
    g = np.random.default_rng(4)
    for dy, dx in [(-16, -16), (16, 16), (0, 0), (-16, 16)] + [tuple(int(v) for v in g.integers(-16, 17, 2)) for _ in range(40)]:
        for k in range(2):
            assert sc[k, dy + 16, dx + 16] == R.score_slices(occA[k], occB, dy, dx)
    assert sc.max() > 20 and sc.min() < sc.max()      # not a comparison of zeros (the two yaws are arbitrary, not the pair's own)


N_TRUE, N_FALSE = 6, 6


@pytest.fixture(scope="module")
def quality():
    rows = []
    for seed in range(N_TRUE):
        a, b, yaw, t = R.true_pair(seed)
        rows.append((R.chain(a[None], b[None], [[0, 0]]), yaw, t))
    false = [R.chain(*(c[None] for c in R.false_pair(seed)), [[0, 0]]) for seed in range(N_FALSE)]
    return rows, false


def test_quality_on_labelled_scenes(quality):
    """The restatement with the default search on the committed scenes (align_ref.true_pair / false_pair, seeds 0 .. 5).  The
    conditions are properties of the method: after the coarse pass the yaw is within one coarse step (3 degrees) and the translation
    within one coarse cell (0.5 m) per axis; after the fine pass within two fine steps (0.75 degrees) and one fine cell (0.25 m);
    every true pair's overlap exceeds every false pair's.  Observed: coarse 1.27 degrees / 0.22 m at the worst, fine 0.38 degrees /
    0.11 m; true overlap 0.50 or more (coarse) and 0.62 or more (fine), false overlap 0.34 or less."""
    rows, false = quality
    H, fd = R.DEFAULTS["yaw_steps"], R.DEFAULTS["fine_div"]
    worst = dict(cy=0.0, ct=0.0, fy=0.0, ft=0.0)
    true_ov, false_ov = [], []
    for seed, (r, yaw, t) in enumerate(rows):
        c = r["coarse"][0]
        cyaw = 2 * math.pi * c[0] / H
        ct = np.array([c[2], c[1]]) * 0.5
        cy_err, ct_err = R.yaw_error(cyaw, yaw), np.abs(ct - t).max()
        fy_err, ft_err = R.yaw_error(r["yaw"][0], yaw), np.abs(r["translation"][0] - t).max()
        c_ov = c[3] / min(c[4], c[5])
        print(f"MEASURE align/quality/true{seed} coarse {math.degrees(cy_err):.2f} deg {ct_err:.3f} m overlap {c_ov:.3f}  "
              f"fine {math.degrees(fy_err):.2f} deg {ft_err:.3f} m overlap {r['overlap'][0]:.3f}  cells {c[4]} / {c[5]}")
        worst = dict(cy=max(worst["cy"], cy_err), ct=max(worst["ct"], ct_err), fy=max(worst["fy"], fy_err), ft=max(worst["ft"], ft_err))
        true_ov += [c_ov, r["overlap"][0]]
        assert cy_err <= 2 * math.pi / H + 1e-9 and ct_err <= 0.5
        assert fy_err <= 2 * (2 * math.pi / (H * fd)) + 1e-9 and ft_err <= 0.25
    for seed, r in enumerate(false):
        c = r["coarse"][0]
        c_ov = c[3] / max(min(c[4], c[5]), 1)
        print(f"MEASURE align/quality/false{seed} overlap coarse {c_ov:.3f} fine {r['overlap'][0]:.3f}")
        false_ov += [c_ov, r["overlap"][0]]
    print(f"MEASURE align/quality worst coarse {math.degrees(worst['cy']):.2f} deg {worst['ct']:.3f} m, fine {math.degrees(worst['fy']):.2f} deg "
          f"{worst['ft']:.3f} m; true overlap >= {min(true_ov):.3f}, false overlap <= {max(false_ov):.3f}")
    assert min(true_ov) > max(false_ov)


def test_align_search_validation():
    d = verify.AlignSearch()
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert [a for a in inspect.signature(verify.AlignSearch.__init__).parameters][1:] == list(R.DEFAULTS)
    for bad in (dict(layers=0), dict(layers=5), dict(layers=2.5), dict(shifts=-1), dict(shifts=17), dict(fine_shifts=17), dict(yaw_steps=0),
                dict(yaw_steps=1025), dict(yaw_steps=1024, fine_div=16), dict(cell=0.0), dict(cell=-1.0), dict(cell=np.nan), dict(cell=INF),
                dict(z_cell=0.0), dict(z_lo=np.nan), dict(z_lo=INF), dict(fine=1), dict(fine_div=0), dict(fine_div=512), dict(yaw_steps=1, fine_div=2),
                dict(shifts=True)):
        with pytest.raises(ValueError):
            verify.AlignSearch(**bad)
    verify.AlignSearch(yaw_steps=1024, fine=False, fine_div=100)      # the dense table is not made when there is no fine pass
    verify.AlignSearch(yaw_steps=1024, fine_div=8, shifts=0, fine_shifts=16, layers=1)
    with pytest.raises(AttributeError):
        d.cell = 1.0
    assert d == verify.AlignSearch() and hash(d) == hash(verify.AlignSearch()) and "yaw_steps=120" in repr(d)
    t = d.coarse_table("cpu")
    assert t is d.coarse_table("cpu") and t.dtype == torch.float32 and np.array_equal(t.numpy(), R.rot_table(120))
    assert np.array_equal(d.dense_table("cpu").numpy(), R.rot_table(960)) and np.array_equal(verify.rot_table(960), R.rot_table(960))
    assert np.array_equal(R.rot_table(960)[::8], R.rot_table(120))      # the coarse angles are entries of the dense table, bit for bit


def test_ops_align_pairs_validation_and_no_cpu_path():
    a = torch.zeros(3, 64, 3)
    b = torch.zeros(2, 1, 64, 3)
    pairs = torch.zeros(5, 2, dtype=torch.int32)
    rot = torch.from_numpy(R.rot_table(16))
    ok = dict(H=16, inv_cell=2.0, S=8, z0=0.0, inv_zcell=0.5, layers=4)

    def call(a=a, b=b, pairs=pairs, rot=rot, **kw):
        args = dict(ok)
        extra = {k: kw.pop(k) for k in ("scale_a", "scale_b", "first", "t0") if k in kw}
        args.update(kw)
        return ops.align_pairs(a, b, pairs, rot, args["H"], args["inv_cell"], args["S"], args["z0"], args["inv_zcell"], args["layers"], **extra)
    for bad in (dict(layers=0), dict(layers=5), dict(S=-1), dict(S=17), dict(H=17), dict(H=0), dict(inv_cell=0.0), dict(inv_cell=INF),
                dict(inv_zcell=-1.0), dict(z0=np.nan), dict(a=torch.zeros(3, 65, 3)), dict(a=torch.zeros(3, 64, 4)), dict(a=torch.zeros(64, 3)),
                dict(b=torch.zeros(2, 2, 64, 3)), dict(a=torch.zeros(1, 16385, 3), b=torch.zeros(1, 16385, 3)), dict(pairs=torch.zeros(5, 3, dtype=torch.int32)),
                dict(pairs=torch.zeros(0, 2, dtype=torch.int32)), dict(rot=torch.zeros(16, 3)), dict(rot=torch.zeros(8193, 2)), dict(H=1025, rot=torch.zeros(2048, 2)),
                dict(scale_a=torch.ones(2)), dict(scale_b=torch.ones(3)), dict(first=torch.zeros(4, dtype=torch.int32)), dict(t0=torch.zeros(5, 3))):
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (dict(a=a.double()), dict(b=b.half()), dict(pairs=pairs.long()), dict(rot=rot.double()), dict(first=torch.zeros(5)),
                dict(t0=torch.zeros(5, 2, dtype=torch.float64)), dict(scale_a=torch.ones(3, dtype=torch.float64)), dict(a=np.zeros((3, 64, 3), dtype=np.float32)),
                dict(pairs=None), dict(rot=None)):
        with pytest.raises(TypeError):
            call(**bad)
    with pytest.raises(LpdHipError):      # everything is in order but the device: there is no CPU path
        call()
    with pytest.raises(LpdHipError):
        verify.align_pairs(a, b, pairs)
    with pytest.raises(TypeError):
        verify.align_pairs(a, b, pairs, search=dict(cell=0.5))
    with pytest.raises(TypeError):
        verify.align_pairs(a, b, pairs.float())
    with pytest.raises(ValueError):
        verify.align_pairs(a, b, torch.zeros(5, 3, dtype=torch.int64))
    with pytest.raises(TypeError):
        verify.verify_candidates(a, b, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        verify.verify_candidates(a, b, torch.zeros(3, 2, dtype=torch.int64), min_overlap=1.5)


def test_public_surface():
    import lpdnet_hip
    assert lpdnet_hip.verify is verify
    i, p, f = _lib._c_int, _lib._c_p, _lib._c_f
    assert _lib.SIGNATURES["lpd_align_pairs"] == [p, i, p, p, i, p, i, p, i, p, i, p, i, p, f, i, f, f, i, p, p, p, p]
    assert _lib.SIGNATURES["lpd_align_workspace_bytes"] == [i, i] and _lib._RESTYPES["lpd_align_workspace_bytes"] is ctypes.c_longlong
    hdr = open(os.path.join(ROOT, "include", "lpd_hip.h")).read()
    for text in ("int lpd_align_pairs(", "long long lpd_align_workspace_bytes(int P, int H);", "csrc/lpd_align_math.h", "xr = (px*c) - (py*s)",
                 "yr = (px*s) + (py*c)", "floorf(xr * inv_cell) + 64.0f", "(first[p] + h) mod R", "(h, dy, dx, score, nA, nB, 1, 0)",
                 "(-1, 0, 0, 0, 0, 0, 0, 0)"):
        assert text in hdr, text
    math_h = open(MATH_H).read()
    assert not re.search(r"\bfmaf?\s*\(", math_h) and "__HIPCC__" in math_h and not re.search(r"\b(sinf?|cosf?|atan2f?)\s*\(", math_h)
    for define in ("LPD_ALIGN_GRID 128", "LPD_ALIGN_MAX_S 16", "LPD_ALIGN_MAX_LAYERS 4", "LPD_ALIGN_MAX_H 1024", "LPD_ALIGN_MAX_R 8192",
                   "LPD_ALIGN_MAX_POINTS 16384"):
        assert "#define " + define in hdr and "#define " + define.split()[0] not in math_h      # the public header's, once
    kern = open(os.path.join(CSRC, "lpd_align.hip")).read()
    code = re.sub(r"//[^\n]*", "", kern)
    assert "atomicOr" in code and not re.search(r"\bfmaf?\s*\(", code) and not re.search(r"\b(sinf?|cosf?|sincosf?)\s*\(", code)
    assert not re.search(r"atomic\w*\s*\([^;]*float", code) and "unsafeAtomic" not in code      # integer atomics only
    assert (ops.ALIGN_GRID, ops.ALIGN_MAX_S, ops.ALIGN_MAX_LAYERS, ops.ALIGN_MAX_H, ops.ALIGN_MAX_R, ops.ALIGN_MAX_POINTS) == \
        (R.GRID, R.MAX_S, R.MAX_LAYERS, R.MAX_H, R.MAX_R, R.MAX_POINTS) == (128, 16, 4, 1024, 8192, 16384)
    assert [a for a in inspect.signature(ops.align_pairs).parameters] == ["a", "b", "pairs", "rot", "H", "inv_cell", "S", "z0", "inv_zcell", "layers",
                                                                         "scale_a", "scale_b", "first", "t0", "want_yaw_scores"]
    sig = inspect.signature(verify.align_pairs)
    assert [a for a in sig.parameters] == ["a", "b", "pairs", "search", "scale_a", "scale_b", "center_a", "center_b"]
    assert sig.parameters["search"].default == verify.AlignSearch()
    sig = inspect.signature(verify.verify_candidates)
    assert [a for a in sig.parameters] == ["query", "database", "topk_idx", "search", "min_overlap"] and sig.parameters["min_overlap"].default is None
    assert set(verify.Alignment.__slots__) >= {"yaw", "translation", "score", "cells_a", "cells_b", "overlap", "yaw_scores", "valid"}
    assert callable(verify.Alignment.matrix)


def test_matrix_composes_centres_on_the_host():
    yaw = torch.tensor([math.pi / 2, 0.0], dtype=torch.float64)
    al = verify.Alignment(yaw=yaw, translation=torch.tensor([[1.0, 2.0], [0.0, 0.0]], dtype=torch.float64), score=None, cells_a=None, cells_b=None,
                          overlap=None, yaw_scores=None, valid=None, coarse=None, fine=None,
                          center_a=torch.tensor([[10.0, 0.0, 3.0], [1.0, 1.0, 1.0]], dtype=torch.float64),
                          center_b=torch.tensor([[0.0, 5.0, 4.5], [2.0, 2.0, 2.0]], dtype=torch.float64))
    M = al.matrix()
    assert M.shape == (2, 4, 4) and M.dtype == torch.float64
    # p_B = R (p_A - c_A) + t + c_B with R = 90 degrees: p_A = (11, 0, 3) -> R (1, 0, 0) = (0, 1, 0) -> (1, 8, 4.5)
    got = M[0] @ torch.tensor([11.0, 0.0, 3.0, 1.0], dtype=torch.float64)
    assert torch.allclose(got, torch.tensor([1.0, 8.0, 4.5, 1.0], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(M[1], torch.tensor([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=torch.float64))
    al.center_a = al.center_b = None
    assert torch.allclose(al.matrix()[0, :3, 3], torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64))
