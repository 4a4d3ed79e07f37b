"""CPU side of localisation against the drive map (lpd_map_surface, lpd_map_localize, lpdnet_hip/mapping.py): the kernels' arithmetic
header (csrc/lpd_loc_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/loc_ref.py) value for
value, hand-made cases with their answers written down, the quality conditions of the design on loc_cases.street_case, and the host
side of the wrappers.  The kernels are tested on the GPU (tests/test_localize_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import icp_ref as I
import loc_cases as C
import loc_ref as L
import map_ref as M
from lpdnet_hip import mapping, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32, f64, i64 = np.float32, np.float64, np.int64

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_loc_math.h"
// <mode> <in> <out> <n> <capacity>: float64 in, float64 out (integers as float64; 64-bit words as two 32-bit halves).  With a capacity
// the input starts with the table: capacity x (key lo, key hi, Sx, Sy, Sz, m); surf is made from it with reach 1, min_cells 5.
//   find     key lo, key hi                                   -> slot
//   surface  slot, reach, min_cells                           -> ret, row 8
//   match    w 3, inv_cell, dmax, max_flat, g32 3             -> has a cell, centred ok, slot, d2, accepted, key lo, key hi, p 3, terms 29
//   step     sums 29 x (lo, hi), min_inliers, origin 3, g 3, pose 12 -> applied, pose 12
//   valid    pose 12, origin 3, o0, o1, rows                  -> valid, g 3, g32 3
static double lo32(uint64_t v) { return (double)(uint32_t)(v & 0xffffffffull); }
static double hi32(uint64_t v) { return (double)(uint32_t)(v >> 32); }
static uint64_t join(double lo, double hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }
int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    const int64_t cap = (int64_t)atoll(argv[5]);
    size_t rin = 0, rout = 0;
    if (!strcmp(mode, "find")) { rin = 2; rout = 1; }
    else if (!strcmp(mode, "surface")) { rin = 3; rout = 9; }
    else if (!strcmp(mode, "match")) { rin = 9; rout = 39; }
    else if (!strcmp(mode, "step")) { rin = 77; rout = 13; }
    else if (!strcmp(mode, "valid")) { rin = 18; rout = 7; }
    else return 2;
    std::vector<double> in((size_t)cap * 6 + n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 8, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    std::vector<int64_t> keys((size_t)cap), acc((size_t)cap * 4);
    std::vector<float> surf((size_t)cap * LPD_LOC_SURF);
    for (int64_t s = 0; s < cap; ++s) {
        keys[s] = (int64_t)join(in[6 * s], in[6 * s + 1]);
        for (int c = 0; c < 4; ++c) acc[4 * s + c] = (int64_t)in[6 * s + 2 + c];
    }
    for (int64_t s = 0; s < cap; ++s) lpd_loc_surface(keys.data(), acc.data(), cap, s, 1, 5, &surf[LPD_LOC_SURF * s]);
    for (size_t k = 0; k < n; ++k) {
        const double* r = &in[(size_t)cap * 6 + k * rin];
        double* o = &out[k * rout];
        if (!strcmp(mode, "find")) {
            o[0] = (double)lpd_loc_find(keys.data(), cap, (int64_t)join(r[0], r[1]));
        } else if (!strcmp(mode, "surface")) {
            float row[LPD_LOC_SURF];
            o[0] = (double)lpd_loc_surface(keys.data(), acc.data(), cap, (int64_t)r[0], (int)r[1], (int)r[2], row);
            for (int c = 0; c < LPD_LOC_SURF; ++c) o[1 + c] = (double)row[c];
        } else if (!strcmp(mode, "match")) {
            const float w[3] = {(float)r[0], (float)r[1], (float)r[2]}, g32[3] = {(float)r[6], (float)r[7], (float)r[8]};
            int q[3] = {0, 0, 0};
            float p[3], best = 0.0f;
            o[0] = (double)(lpd_map_index(w[0], (float)r[3], q) && lpd_map_index(w[1], (float)r[3], q + 1) && lpd_map_index(w[2], (float)r[3], q + 2));
            o[1] = (double)lpd_loc_centred(w, g32, p);
            o[2] = -1.0;
            if (o[0] != 0.0) {
                const int64_t at = lpd_loc_nearest(keys.data(), surf.data(), cap, q, w, &best);
                o[2] = (double)at;
                o[3] = (double)best;
                if (at >= 0) {
                    const float* row = &surf[LPD_LOC_SURF * at];
                    o[4] = (double)lpd_loc_accept(row, best, (float)r[4], (float)r[5]);
                    o[5] = lo32((uint64_t)keys[at]);
                    o[6] = hi32((uint64_t)keys[at]);
                    int64_t t[LPD_ICP_SUMS] = {0};
                    lpd_loc_terms(p, row, g32, t);
                    for (int c = 0; c < 29; ++c) o[10 + c] = (double)t[c];
                }
            }
            for (int c = 0; c < 3; ++c) o[7 + c] = (double)p[c];
        } else if (!strcmp(mode, "step")) {
            int64_t s[LPD_ICP_SUMS] = {0};
            for (int c = 0; c < 29; ++c) s[c] = (int64_t)join(r[2 * c], r[2 * c + 1]);
            double pose[12];
            for (int c = 0; c < 12; ++c) pose[c] = r[65 + c];
            o[0] = (double)lpd_loc_step(s, (int)r[58], r + 59, r + 62, pose);
            for (int c = 0; c < 12; ++c) o[1 + c] = pose[c];
        } else {
            o[0] = (double)lpd_loc_scan_valid(r, (int64_t)r[15], (int64_t)r[16], (int64_t)r[17]);
            double g[3];
            float g32[3];
            lpd_loc_centre(r, r + 12, g, g32);
            for (int c = 0; c < 3; ++c) { o[1 + c] = g[c]; o[4 + c] = (double)g32[c]; }
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
    d = tmp_path_factory.mktemp("loc_math")
    src = d / "loc_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "loc_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, records, n_out, table=None):
        records = np.ascontiguousarray(records, dtype=f64)
        head = np.zeros(0) if table is None else table.reshape(-1)
        np.concatenate((head, records.reshape(-1))).tofile(d / "in.bin")
        cmd = [str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(records.shape[0]), str(0 if table is None else table.shape[0])]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        return np.fromfile(d / "out.bin", dtype=f64).reshape(records.shape[0], n_out)
    return run


def _halves(v):
    v = np.asarray(v).astype(np.uint64)
    return (v & np.uint64(0xffffffff)).astype(f64), (v >> np.uint64(32)).astype(f64)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=f64), np.ascontiguousarray(want, dtype=f64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def make_table(keys, sums, counts, capacity, order=None):
    """a hand-made hash table as lpd_map_insert would leave it when the keys arrive in `order`: [capacity, 6] float64 records (key lo,
    key hi, Sx, Sy, Sz, m) and the slot of every key"""
    keys = np.asarray(keys, dtype=i64)
    tk = np.full(capacity, -1, dtype=i64)
    acc = np.zeros((capacity, 4), dtype=i64)
    where = np.full(len(keys), -1, dtype=i64)
    for j in (range(len(keys)) if order is None else order):
        s = int(M.slot(keys[j:j + 1], capacity)[0])
        for _ in range(M.probes(capacity)):
            if tk[s] == -1:
                tk[s], acc[s, :3], acc[s, 3], where[j] = keys[j], sums[j], counts[j], s
                break
            s = (s + 1) & (capacity - 1)
        else:
            raise AssertionError("the table is too small for this test")
    lo, hi = _halves(tk)
    return np.concatenate((np.stack((lo, hi), axis=1), acc.astype(f64)), axis=1), where


def _random_cells(seed, n, span=6):
    rng = np.random.default_rng(seed)
    q = np.unique(rng.integers(-span, span, (n, 3)), axis=0)
    keys = np.sort(M.key(q))
    counts = rng.integers(1, 40, len(keys))
    q = M.unkey(keys)
    sums = np.rint((q + rng.uniform(0.05, 0.95, q.shape)) * 65536.0 * counts[:, None]).astype(i64)
    return keys, sums, counts


# ---- the lookup ----------------------------------------------------------------------------------------------------------------------------
def test_lookup_on_hand_made_tables_does_not_depend_on_slot_placement(host):
    keys, sums, counts = _random_cells(1, 200)
    absent = M.key(np.array([[50, 50, 50], [-50, 0, 3], [7, -60, 1]]))
    ask = np.concatenate((keys, absent))
    rng = np.random.default_rng(2)
    for cap in (256, 1024):
        for order in (None, rng.permutation(len(keys))):
            table, where = make_table(keys, sums, counts, cap, order)
            got = host("find", np.stack(_halves(ask), axis=1), 1, table)[:, 0]
            assert np.array_equal(got[:len(keys)], where.astype(f64)) and np.all(got[len(keys):] == -1)
    assert np.array_equal(L.lookup(keys, ask), np.concatenate((np.arange(len(keys)), [-1, -1, -1])))


def test_a_full_table_of_16_slots_ends_every_lookup_after_16_probes(host):
    keys, sums, counts = _random_cells(3, 40, span=2)
    keys, sums, counts = keys[:16], sums[:16], counts[:16]
    table, where = make_table(keys, sums, counts, 16)
    assert (where >= 0).all() and M.probes(16) == 16
    absent = M.key(np.random.default_rng(4).integers(10, 20, (50, 3)))
    got = host("find", np.stack(_halves(np.concatenate((keys, absent))), axis=1), 1, table)[:, 0]
    assert np.array_equal(got[:16], where.astype(f64)) and np.all(got[16:] == -1)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach,min_cells", [(1, 5), (2, 5), (1, 27), (2, 30), (1, 4)])
def test_surface_rows_equal_the_restatement_for_every_placement(host, reach, min_cells):
    keys, sums, counts = _random_cells(5, 500, span=5)
    want = L.surface_of(keys, M.extract(sums, counts), reach, min_cells)
    if (reach, min_cells) in ((1, 5), (2, 30)):      # both sides of min_cells turn up
        assert 0 < (want.used < min_cells).sum() < len(keys)
    rng = np.random.default_rng(6)
    for cap, order in ((1024, None), (2048, rng.permutation(len(keys)))):
        table, where = make_table(keys, sums, counts, cap, order)
        got = host("surface", np.stack((where, np.full(len(keys), reach), np.full(len(keys), min_cells)), axis=1).astype(f64), 9, table)
        _same(got[:, 1:], want.rows().astype(f64), (reach, min_cells, cap))
        has = ~((want.normals == 0).all(axis=1))
        assert np.array_equal(got[:, 0], np.where(has, 1.0, 2.0))
    empty = np.flatnonzero(table[:, 1] == float(0xffffffff))[:5]
    got = host("surface", np.stack((empty, np.ones(5), np.full(5, 5)), axis=1).astype(f64), 9, table)
    assert np.all(got == 0)


def test_a_slot_without_rows_is_absent_and_never_the_nearest(host):
    keys = M.key(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0]]))
    order = np.argsort(keys)
    keys = keys[order]
    q = M.unkey(keys)
    counts = np.array([2, 2, 0, 2, 2, -3])
    sums = ((q + 0.5) * 65536.0 * 2).astype(i64)
    table, where = make_table(keys, sums, counts, 64)
    got = host("surface", np.stack((where, np.ones(6), np.full(6, 4)), axis=1).astype(f64), 9, table)
    live = counts > 0
    want = L.surface_of(keys[live], M.extract(sums[live], counts[live]), 1, 4)
    _same(got[live, 1:], want.rows().astype(f64), "the cells with rows")
    assert np.isnan(got[~live, 1:4]).all() and np.all(got[~live, 4:] == 0) and np.all(got[~live, 0] == 2)
    assert want.used.tolist() == [4, 4, 4, 4]
    w = (M.unkey(keys[~live][:1])[0] + 0.5).astype(f64)      # a point in the middle of a cell without rows
    rec = np.array([[w[0], w[1], w[2], 1.0, 16.0, 1.0, 0.0, 0.0, 0.0]])
    m = host("match", rec, 39, table)[0]
    assert m[0] == 1 and m[2] in where[live].astype(f64)


# ---- hand-made surfaces with written-down answers -------------------------------------------------------------------------------------------
def _slab(nx=5, ny=5, z=0, at=(0, 0)):
    q = np.array([[at[0] + x, at[1] + y, z] for y in range(ny) for x in range(nx)])
    keys = M.key(q)
    order = np.argsort(keys)
    return keys[order], (q[order] + 0.5).astype(f32)


def test_a_flat_slab_has_vertical_normals_and_an_isolated_cell_has_none():
    keys, pts = _slab()
    s = L.surface_of(keys, pts, 1, 4)
    assert np.array_equal(np.abs(s.normals), np.tile(f32([0, 0, 1]), (25, 1))) and np.all(s.flatness == 0)
    assert sorted(set(s.used.tolist())) == [4, 6, 9]
    s5 = L.surface_of(keys, pts, 1, 5)      # the four corners see four cells
    assert ((s5.normals == 0).all(axis=1) == (s5.used == 4)).all() and (s5.used == 4).sum() == 4
    far = M.key(np.array([[40, 40, 40]]))
    k2 = np.concatenate((keys, far))
    s = L.surface_of(k2, np.concatenate((pts, f32([[40.5, 40.5, 40.5]]))), 2, 4)
    assert s.used[-1] == 1 and np.all(s.normals[-1] == 0) and s.flatness[-1] == 0
    assert sorted(set(s.used[:-1].tolist())) == [9, 12, 15, 16, 20, 25]


def test_a_point_equidistant_from_two_centroids_takes_the_lower_key(host):
    keys, pts = _slab(2, 5)
    surf = L.surface_of(keys, pts, 1, 4)
    w = f32([[1.0, 2.5, 0.5]])      # on the face between cells (0, 2, 0) and (1, 2, 0): 0.25 from both centroids
    q, ok = M.index(w, f32(1.0))
    at, best = L.nearest(surf, q, w, ok.all(axis=1))
    assert q[0].tolist() == [1, 2, 0] and best[0] == f32(0.25)
    assert surf.keys[at[0]] == M.key(np.array([[0, 2, 0]]))[0] < M.key(np.array([[1, 2, 0]]))[0]
    table, where = make_table(keys, (pts.astype(f64) * 65536.0).astype(i64), np.ones(len(keys), dtype=i64), 32)
    m = host("match", np.array([[1.0, 2.5, 0.5, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]]), 39, table)[0]
    assert m[2] == where[at[0]] and m[3] == 0.25 and m[4] == 1


def test_cells_at_the_index_border_skip_the_neighbours_beyond_it(host):
    top = M.QLIM - 1
    keys, pts = _slab(3, 3, z=top, at=(top - 2, -M.QLIM))
    k, inside = L.neighbour(M.unkey(keys), (1, 0, 0))
    assert (~inside).sum() == 3 and L.neighbour(M.unkey(keys), (0, -1, 0))[1].sum() == 6 and L.neighbour(M.unkey(keys), (0, 0, 1))[1].sum() == 0
    s = L.surface_of(keys, pts, 2, 4)
    assert s.used.tolist() == [9] * 9 and np.array_equal(np.abs(s.normals), np.tile(f32([0, 0, 1]), (9, 1)))
    sums = (pts.astype(f64) * 65536.0).astype(i64)
    table, where = make_table(keys, sums, np.ones(9, dtype=i64), 64)
    got = host("surface", np.stack((where, np.full(9, 2), np.full(9, 4)), axis=1).astype(f64), 9, table)
    _same(got[:, 1:], s.rows().astype(f64), "border")
    # a point in the corner cell: its 27 candidates are 4 cells
    w = pts[[-1]] + f32(0.25)
    q, ok = M.index(w, f32(1.0))
    assert q[0].tolist() == [top, -M.QLIM + 2, top] and sum(int(L.neighbour(q, d)[1][0]) for d in L.OFFSETS27) == 12
    at, best = L.nearest(L.surface_of(keys, pts, 1, 4), q, w, ok.all(axis=1))
    m = host("match", np.array([[w[0, 0], w[0, 1], w[0, 2], 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]], dtype=f64), 39, table)[0]
    assert m[2] == where[at[0]] and m[3] == float(best[0])


# ---- the correspondence, the centred row, the step, the validity ---------------------------------------------------------------------------
def test_candidate_order_decisions_and_centred_rows_equal_the_restatement(host):
    keys, sums, counts = _random_cells(7, 900, span=5)
    pts = M.extract(sums, counts)
    surf = L.surface_of(keys, pts, 1, 5)
    table, where = make_table(keys, sums, counts, 2048, np.random.default_rng(8).permutation(len(keys)))
    rng = np.random.default_rng(9)
    n = 1500
    w = rng.uniform(-6.5, 6.5, (n, 3)).astype(f32)
    w[:60] = pts[rng.integers(0, len(pts), 60)] + f32([0.5, 0.0, 0.0])      # equal distances turn up on the lattice of centroids
    w[60:64] = f32([[np.nan, 0, 0], [0, np.inf, 0], [3e7, 0, 0], [0, 0, -3e7]])
    g32 = np.tile(f32([0.25, -0.5, 0.125]), (n, 1))
    g32[64:80] = f32([600.0, 0.0, 0.0])      # |p_x| beyond 512: no correspondence
    dmax, max_flat = f32(0.75), f32(0.3)
    rec = np.concatenate((w.astype(f64), np.full((n, 1), 1.0), np.full((n, 1), float(dmax)), np.full((n, 1), float(max_flat)), g32.astype(f64)), axis=1)
    got = host("match", rec, 39, table)
    q, ok = M.index(w, f32(1.0))
    ok = ok.all(axis=1)
    p, near = L.centred(w, g32)
    assert np.array_equal(got[:, 0] != 0, ok) and np.array_equal(got[:, 1] != 0, near) and 0 < (~near[ok]).sum()
    at, best = L.nearest(surf, q, w, ok)
    assert np.array_equal(got[:, 2], np.where(at >= 0, where[np.maximum(at, 0)], -1).astype(f64))
    hit = at >= 0
    _same(got[hit, 3], best[hit].astype(f64), "d2")
    acc = L.accept(surf, at, best, dmax, max_flat)
    assert np.array_equal(got[hit, 4] != 0, acc[hit]) and 0 < acc[hit].sum() < hit.sum()
    _same(got[ok, 7:10], p[ok].astype(f64), "p")
    T = L.terms(p[hit], surf.points[at[hit]], surf.normals[at[hit]], g32[hit])
    assert np.array_equal(got[hit, 10:39], T[:, :29].astype(f64))


def test_dmax_and_max_flat_decide_at_equality(host):
    keys, pts = _slab()
    surf = L.surface_of(keys, pts, 1, 4)
    table, where = make_table(keys, (pts.astype(f64) * 65536.0).astype(i64), np.ones(25, dtype=i64), 64)
    w = f32([[2.5, 2.5, 0.75]])      # 0.25 above the middle centroid: d2 = 0.0625 = 0.25^2 exactly
    for dmax, want in ((0.25, 1.0), (float(np.nextafter(f32(0.25), f32(0))), 0.0)):
        m = host("match", np.array([[2.5, 2.5, 0.75, 1.0, dmax, 1.0, 0, 0, 0]], dtype=f64), 39, table)[0]
        q, ok = M.index(w, f32(1.0))
        at, best = L.nearest(surf, q, w, ok.all(axis=1))
        assert m[3] == 0.0625 and m[4] == want and bool(L.accept(surf, at, best, f32(dmax), f32(1.0))[0]) == bool(want)
    # flatness: a cell whose l3 / l2 is exactly max_flat is kept, the next fp32 below refuses it
    keys, sums, counts = _random_cells(7, 900, span=5)
    surf = L.surface_of(keys, M.extract(sums, counts), 1, 5)
    j = int(np.argmax((surf.flatness > 0.05) & (surf.flatness < 0.9)))
    flat = surf.flatness[j]
    table, where = make_table(keys, sums, counts, 2048)
    c = surf.points[j].astype(f64)
    for mf, want in ((float(flat), 1.0), (float(np.nextafter(flat, f32(0))), 0.0)):
        m = host("match", np.array([[c[0], c[1], c[2], 1.0, 1.0, mf, 0, 0, 0]]), 39, table)[0]
        assert m[2] == where[j] and m[3] == 0.0 and m[4] == want
        assert bool(L.accept(surf, np.array([j]), f32([0.0]), f32(1.0), f32(mf))[0]) == bool(want)


def _sums_of_a_pass():
    case, cells, surf = C.street_map(1, 1.0)
    off = M.offsets_of(case["lengths"])
    P = case["start"].copy()
    g, g32 = L.centre(P, case["origin"])
    grow = np.arange(off[-1])
    gscan = np.searchsorted(off[:-1], grow, side="right") - 1
    return L.one_pass(surf, case["points"], grow, gscan, P, case["origin"], g32, M.inv_cell(1.0), f32(1.0), 0.3, len(P))[0], P, g


def test_the_centred_step_at_a_utm_origin_equals_the_restatement(host):
    sums, P, g = _sums_of_a_pass()
    utm = np.array([5.7e6, 6.2e5, 120.0])
    rec, want = [], []
    for i in range(len(P)):
        pose = P[i].copy()
        pose[M.TRA] += utm      # the same scan at a UTM easting and northing: origin and pose move, the centre does not
        origin = utm.copy()
        for mi, s in ((50, sums[i]), (int(sums[i, 0]) + 1, sums[i]), (6, np.zeros(32, dtype=i64))):
            lo, hi = _halves(s[:29].astype(np.uint64))
            rec.append(np.concatenate((np.stack((lo, hi), axis=1).reshape(-1), [mi], origin, g[i], pose)))
            want.append(L.step(s, mi, pose, origin, g[i]))
    got = host("step", np.array(rec), 13)
    assert got[:, 0].tolist() == [1.0, 0.0, 0.0] * len(P) == [float(w[0]) for w in want]
    _same(got[:, 1:], np.array([w[1] for w in want]), "step")
    moved = np.abs(got[0::3, 1:] - np.array(rec)[0::3, 65:]).max(axis=1)
    assert np.all(moved > 1e-3) and np.all(got[1::3, 1:] == np.array(rec)[1::3, 65:])      # a refused step leaves the pose bit for bit
    # the rotation is about the centre: the same sums with g = 0 move the translation by the lever arm as well
    ok, away = L.step(sums[0], 50, np.array(rec)[0, 65:], utm, np.zeros(3))
    assert ok and np.abs(away[M.TRA] - got[0, 1:][M.TRA]).max() > 1e-4


def test_validity_and_centre(host):
    ident = np.array([1.0, 0, 0, 5.7e6 + 0.3, 0, 1.0, 0, 6.2e5 - 0.7, 0, 0, 1.0, 120.125])
    origin = np.array([5.7e6, 6.2e5, 100.0])
    nan, inf = ident.copy(), ident.copy()
    nan[5], inf[11] = np.nan, np.inf
    big = L.MAX_SCAN_ROWS
    cases = [(ident, 0, 10, 10, 1), (ident, 0, 0, 10, 1), (ident, 5, 4, 10, 0), (ident, -1, 4, 10, 0), (ident, 0, 11, 10, 0), (nan, 0, 10, 10, 0),
             (inf, 0, 10, 10, 0), (ident, 7, 7 + big, 2 * big, 1), (ident, 7, 8 + big, 2 * big, 0)]
    rec = np.array([np.concatenate((p, origin, [a, b, r])) for p, a, b, r, _ in cases])
    got = host("valid", rec, 7)
    assert got[:, 0].tolist() == [float(c[4]) for c in cases]
    for k, (p, a, b, r, v) in enumerate(cases):
        assert bool(L.scan_valid(p[None], np.array([a, b]), r, 0, 1)[0]) == bool(v)
    g, g32 = L.centre(np.array([c[0] for c in cases]), origin)
    _same(got[:, 1:4], g, "g")
    _same(got[:, 4:7], g32.astype(f64), "g32")
    assert g[0].tolist() == [(5.7e6 + 0.3) - 5.7e6, (6.2e5 - 0.7) - 6.2e5, 20.125] and g32[0, 2] == f32(20.125)


# ---- a scan at its true pose ---------------------------------------------------------------------------------------------------------------
def test_a_scan_at_its_true_pose_on_a_noise_free_map_stays_there():
    pts, pose, origin = C.flat_case()
    off = np.array([0, len(pts)], dtype=np.int32)
    cells = M.insert(pts, off, pose[None], origin, 1.0)
    surf = L.surface(cells)
    bare = (surf.normals == 0).all(axis=1)      # the twelve corner cells of the three sheets see four cells
    assert np.array_equal(np.unique(np.abs(surf.normals[~bare]), axis=0), f32([[0, 0, 1], [0, 1, 0], [1, 0, 0]])) and np.all(surf.flatness == 0)
    assert bare.sum() == 12 and np.all(surf.used[bare] == 4) and np.all(cells.counts == 16)
    r = L.localize(surf, pts, off, pose[None], origin, 1.0, (1.0, 1.0))
    x64, m = L.step_float64(surf, pts, pose, origin, 1.0, 1.0, 0.3)
    d = np.abs(r["pose"][0] - pose)
    print(f"MEASURE true pose: {m} correspondences of {len(pts)}; step taken: rotation {d[M.ROT].max():.3e}, translation {d[M.TRA].max():.3e} m; "
          f"float64 unquantised step: rotation {np.abs(x64[:3]).max():.3e} rad, translation {np.abs(x64[3:]).max():.3e} m")
    assert r["info"].tolist() == [[1, 1, 0, m]] and m == len(pts) - 12 * 16      # every row reads the cell it was inserted into
    assert np.array_equal(np.sort(r["cell"][r["cell"] >= 0]), np.repeat(cells.keys[~bare], 16))
    assert max(d[M.ROT].max(), np.abs(x64[:3]).max()) <= C.TRUE_POSE_STEP_ROT and max(d[M.TRA].max(), np.abs(x64[3:]).max()) <= C.TRUE_POSE_STEP_TRANS


# ---- the quality conditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", C.CELLS)
@pytest.mark.parametrize("seed", C.SEEDS)
def test_scans_started_off_end_at_the_truth_and_lost_scans_find_little(seed, cell):
    """Hard conditions on loc_cases.street_case(seed) at the default search: every true case ends nearer the truth than it started, in
    rotation and in translation; the smallest inlier share of the true cases exceeds the largest of the same scans started 45 m away;
    the final errors stay within loc_cases.FINAL_* (1.5 x the worst measured over the four seeds)."""
    case, cells, surf = C.street_map(seed, cell)
    off = M.offsets_of(case["lengths"])
    dm = L.schedule(cell)
    r = L.localize(surf, case["points"], off, case["start"], case["origin"], cell, dm)
    far = L.localize(surf, case["points"], off, case["far"], case["origin"], cell, dm)
    e0, e1 = C.errors(case["start"], case["truth"]), C.errors(r["pose"], case["truth"])
    share, share_far = r["info"][:, 3] / case["lengths"], far["info"][:, 3] / case["lengths"]
    print(f"MEASURE seed {seed} cell {cell}: {len(cells.keys)} cells; start " + ", ".join(f"{a:.2f} deg / {b:.2f} m" for a, b in e0) + "; end "
          + ", ".join(f"{a:.4f} deg / {b:.4f} m" for a, b in e1) + f"; share {share.min():.3f} .. {share.max():.3f}, 45 m away at most {share_far.max():.3f}")
    assert r["info"][:, 0].tolist() == [1, 1, 1] and r["info"][:, 1].tolist() == [8, 8, 8]
    for (r0, t0), (r1, t1) in zip(e0, e1):
        assert r1 < r0 and t1 < t0
    assert share.min() > share_far.max()
    assert max(e[0] for e in e1) <= C.FINAL_ROT_DEG[cell] and max(e[1] for e in e1) <= C.FINAL_TRANS_M[cell]


# ---- the host side of the wrappers ---------------------------------------------------------------------------------------------------------
def test_search_parameters_are_validated_and_frozen():
    s = mapping.LocalizeSearch()
    assert (s.iters, s.dmax, s.min_inliers, s.max_flat, s.reach, s.min_cells) == (8, None, 50, 0.3, 1, 5)
    assert s.schedule(1.0) == L.schedule(1.0) == (1.0,) * 5 + (0.5,) * 4 and s.schedule(0.5) == L.schedule(0.5)
    assert s.schedule(40.0)[0] == 16.0 and mapping.LocalizeSearch(iters=0).schedule(2.0) == (2.0,)
    assert mapping.LocalizeSearch(iters=2, dmax=0.7).schedule(1.0) == (0.7, 0.7, 0.7)
    assert mapping.LocalizeSearch(iters=1, dmax=[1.0, 0.5]).schedule(9.0) == (1.0, 0.5)
    with pytest.raises(AttributeError, match="frozen"):
        s.iters = 3
    assert s == mapping.LocalizeSearch() and hash(s) == hash(mapping.LocalizeSearch())
    for kw in (dict(iters=65), dict(iters=-1), dict(min_inliers=5), dict(max_flat=0.0), dict(max_flat=1.5), dict(max_flat=float("nan")),
               dict(reach=3), dict(reach=0), dict(min_cells=3), dict(min_cells=28), dict(reach=2, min_cells=126), dict(dmax=0.0),
               dict(dmax=17.0), dict(dmax=float("nan")), dict(dmax=[1.0] * 8), dict(dmax="1"), dict(reach=1.0)):
        with pytest.raises(ValueError, match="LocalizeSearch"):
            mapping.LocalizeSearch(**kw)
    assert mapping.LocalizeSearch(reach=2, min_cells=125).min_cells == 125
    assert (ops.LOC_SURF, ops.LOC_MAX_ITERS, ops.LOC_MAX_SCAN_ROWS, ops.LOC_SUMS) == (8, 64, L.MAX_SCAN_ROWS, I.SUMS)


def test_wrappers_refuse_the_cpu_and_bad_arguments_by_name():
    from lpdnet_hip._lib import LpdHipError
    keys, acc = torch.full((16,), -1, dtype=torch.int64), torch.zeros((16, 4), dtype=torch.int64)
    with pytest.raises(LpdHipError, match="keys"):
        ops.map_surface(keys, acc)
    with pytest.raises(ValueError, match="map_surface: reach"):
        ops.map_surface(keys, acc, reach=3)
    with pytest.raises(ValueError, match="map_surface: min_cells"):
        ops.map_surface(keys, acc, min_cells=28)
    with pytest.raises(TypeError, match="map_surface: reach"):
        ops.map_surface(keys, acc, reach=1.5)
    with pytest.raises(LpdHipError, match="points"):
        ops.map_localize(torch.zeros((4, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((1, 12), dtype=torch.float64),
                         torch.zeros(3, dtype=torch.float64), 1.0, keys, torch.zeros((16, 8)), (1.0,))
    for bad in ((), (0.0,), (float("inf"),), (17.0,), (1.0,) * 66):
        with pytest.raises(ValueError, match="map_localize: dmax"):
            ops.map_localize_dmax("map_localize", bad)
    with pytest.raises(TypeError, match="map_localize: dmax"):
        ops.map_localize_dmax("map_localize", 1.0)
    arr, iters = ops.map_localize_dmax("map_localize", (1.0, 0.5, 0.25))
    assert iters == 2 and list(arr) == [1.0, 0.5, 0.25]
    with pytest.raises(TypeError, match="localize_scans: vmap"):
        mapping.localize_scans(object(), None, None, None)
    m = mapping.VoxelMap.__new__(mapping.VoxelMap)
    m.keys = None
    with pytest.raises(TypeError, match="localize_scans: search"):
        mapping.localize_scans(m, None, None, None, search=dict())
    with pytest.raises(ValueError, match="localize_scans: nothing was inserted"):
        mapping.localize_scans(m, None, None, None)
    with pytest.raises(ValueError, match="VoxelMap.surface: nothing was inserted"):
        m.surface()
    with pytest.raises(ValueError, match="VoxelMap.surface: reach"):
        m.surface(reach=4)
