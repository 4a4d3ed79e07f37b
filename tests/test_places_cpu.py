"""CPU side of the place lists (lpd_radius_count / lpd_radius_fill, lpdnet_hip/places.py): the numpy restatement (tests/places_ref.py)
against sklearn's KDTree.query_radius -- the reference's own search -- and against construct_query_dict's expressions, the kernels'
predicate header (csrc/lpd_places_math.h) compiled by the host C++ compiler and compared with the restatement decision for decision,
the fp32 guard that records why the definition is float64, and the host side of lpdnet_hip.places.  The kernels themselves are tested
on the GPU (tests/test_places_gpu.py)."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import places_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATH_H = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc", "lpd_places_math.h")
RADII = (10.0, 25.0, 50.0)
BOUNDARY = ((6.0, 8.0), (8.0, 6.0), (10.0, 0.0))      # offsets of length exactly 10


@pytest.fixture(scope="module")
def routes():
    return {T: R.route(T, seed=T) for T in (130, 4097)}


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("T", [130, 4097])
def test_restatement_equals_kdtree_query_radius(routes, T, r):
    from sklearn.neighbors import KDTree
    pos = routes[T]
    want = KDTree(pos).query_radius(pos, r=r)
    off, idx, counts = R.radius_lists(pos, pos, r)
    rows = R.rows_of(off, idx)
    assert off[-1] == idx.size and np.array_equal(np.diff(off), counts)
    sizes = [len(w) for w in want]
    print(f"MEASURE places/restatement/T{T}/r{r:g} members {sum(sizes)} longest row {max(sizes)}")
    assert max(sizes) > 2      # the route revisits its places: the rows hold more than the item and its two neighbours
    for i in range(T):
        assert np.array_equal(rows[i], np.sort(want[i])), (i, rows[i], np.sort(want[i]))


def test_boundary_points_are_members_as_kdtree_reports_them():
    from sklearn.neighbors import KDTree
    pts = np.array([[0.0, 0.0]] + [list(b) for b in BOUNDARY]) + R.ORIGIN
    assert all(tuple(pts[1 + k] - pts[0]) == BOUNDARY[k] for k in range(3))      # the offsets survive the addition exactly
    want = np.sort(KDTree(pts).query_radius(pts[:1], r=10.0)[0])
    off, idx, _ = R.radius_lists(pts[:1], pts, 10.0)
    assert want.tolist() == [0, 1, 2, 3] and idx.tolist() == [0, 1, 2, 3]
    out = pts.copy()
    out[1:, 0] = np.nextafter(out[1:, 0], np.inf)      # one ulp farther along the northing: outside
    assert R.radius_lists(pts[:1], out, 10.0)[1].tolist() == [0]
    assert np.sort(KDTree(out).query_radius(pts[:1], r=10.0)[0]).tolist() == [0]


def test_lists_equal_construct_query_dict(routes):
    """generate_training_tuples_baseline.py:52-60 written out: positives = setdiff1d(ind_nn[i], [i]), negatives = setdiff1d(all, ind_r[i]);
    places.to_queries_dict on the restated lists gives the same two lists (negatives sorted: the reference shuffles them)."""
    from sklearn.neighbors import KDTree
    from lpdnet_hip import places, tuples
    T = 130
    pos = routes[T]
    tree = KDTree(pos)
    ind_nn, ind_r = tree.query_radius(pos, r=10), tree.query_radius(pos, r=50)
    po, pi, pc = R.radius_lists(pos, pos, 10.0, self_item=np.arange(T))
    no, ni, nc = R.radius_lists(pos, pos, 50.0)
    t = torch.from_numpy
    lists = places.PlaceLists(T, t(po), t(pi), pc.astype(np.int64), t(no), t(ni), nc.astype(np.int64), 10.0, 50.0)
    files = [f"run/{i}.bin" for i in range(T)]
    got = places.to_queries_dict(lists, files)
    assert sorted(got) == list(range(T)) and len(lists) == T
    for i in range(T):
        assert got[i]["query"] == files[i]
        assert got[i]["positives"] == np.setdiff1d(ind_nn[i], [i]).tolist()
        assert got[i]["negatives"] == np.setdiff1d(list(range(T)), ind_r[i]).tolist()
    assert lists.max_pos == max(len(np.setdiff1d(ind_nn[i], [i])) for i in range(T)) and lists.max_near == max(len(v) for v in ind_r)
    # and back: the bank's existing entry for that layout recovers `near`
    positives, near = tuples.TupleBank.lists_from_queries_dict(got)
    assert all(np.array_equal(near[i], np.sort(ind_r[i])) for i in range(T))
    with pytest.raises(ValueError):
        places.to_queries_dict(lists, files[:-1])


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "lpd_places_math.h"
int main(int argc, char** argv)
{
    // in: n records of five doubles (qx, qy, px, py, r); out: n bytes, the decision of each
    if (argc != 4) return 2;
    const size_t n = (size_t)atol(argv[3]);
    std::vector<double> in(n * 5);
    std::vector<unsigned char> out(n);
    FILE* fi = fopen(argv[1], "rb");
    if (!fi || fread(in.data(), 8, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t i = 0; i < n; ++i) {
        const double* p = &in[i * 5];
        out[i] = lpd_place_within(p[0], p[1], p[2], p[3], lpd_place_radius_sq(p[4])) ? 1 : 0;
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo || fwrite(out.data(), 1, n, fo) != n) return 4;
    fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def math_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("places_math")
    src = d / "places_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "places_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.dirname(MATH_H), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _decision_pairs(route):
    """(qx, qy, px, py, r) records: route pairs near the three radii, the exact-boundary points with their nextafter neighbours on
    both sides, r = 0 with coincident and almost coincident points, NaN and inf positions"""
    g = np.random.default_rng(20261018)
    rec = []
    T = len(route)
    for r in RADII:      # pairs whose distance is close to r: neighbours in time and the revisits
        i = g.integers(0, T, size=1200)
        j = np.clip(i + g.integers(-12, 13, size=1200), 0, T - 1)
        j[::3] = T - 1 - i[::3]      # the way back passes the same place
        rec += [[route[a, 0], route[a, 1], route[b, 0], route[b, 1], r] for a, b in zip(i, j)]
    q = R.ORIGIN
    for bx, by in BOUNDARY:
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            p = q + np.array([sx * bx, sy * by])
            rec.append([q[0], q[1], p[0], p[1], 10.0])                      # on the circle: a member
            rec.append([p[0], p[1], q[0], q[1], 10.0])                      # symmetric
            for axis in (0, 1):
                for toward in (-np.inf, np.inf):
                    pp = p.copy()
                    pp[axis] = np.nextafter(pp[axis], toward)
                    rec.append([q[0], q[1], pp[0], pp[1], 10.0])
                    rec.append([q[0], q[1], p[0], p[1], float(np.nextafter(10.0, toward))])
    for p in (q, route[7], np.array([1.0, -2.5])):      # r = 0: coincident points only
        rec.append([p[0], p[1], p[0], p[1], 0.0])
        rec.append([p[0], p[1], np.nextafter(p[0], np.inf), p[1], 0.0])
        rec.append([p[0], p[1], p[0], np.nextafter(p[1], -np.inf), 0.0])
    rec.append([0.0, 0.0, 5e-324, 0.0, 0.0])      # the square of a denormal underflows to zero: a member at r = 0, by the rule
    bad = (np.nan, np.inf, -np.inf)
    for v in bad:
        for w in bad + (q[1],):
            rec += [[v, w, q[0], q[1], 50.0], [q[0], q[1], v, w, 50.0], [v, w, v, w, 50.0], [q[0], v, q[0], w, 0.0]]
    rec.append([1e200, 0.0, -1e200, 0.0, 50.0])      # the square overflows: not a member
    return np.array(rec, dtype=np.float64)


def test_predicate_header_on_the_host_equals_the_restatement(math_program, tmp_path, routes):
    rec = _decision_pairs(routes[4097])
    rec.tofile(tmp_path / "in.bin")
    r = subprocess.run([str(math_program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(len(rec))], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).astype(bool)
    want = R.within(rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] * rec[:, 4])
    print(f"MEASURE places/predicate {len(rec)} decisions, {int(want.sum())} members")
    assert len(rec) >= 3000 and got.shape == want.shape and np.array_equal(got, want)
    assert 0.2 < want[:3600].mean() < 0.8      # the route pairs straddle the radii
    # what the hand-made records are for
    k = 3600
    for _ in range(12):                       # 3 boundary offsets x 4 sign patterns
        assert want[k] and want[k + 1], k      # on the circle, both ways round
        block = want[k + 2:k + 10]
        assert not block.all() and block.any()      # some neighbours fall outside, some inside
        k += 10
    assert want[k:k + 9].reshape(3, 3)[:, 0].all() and not want[k:k + 9].reshape(3, 3)[:, 1:].any()      # r = 0
    assert want[k + 9]                        # the denormal
    assert not want[k + 10:].any()            # NaN / inf / overflow: never members


def test_fp32_positions_change_memberships(routes):
    """Why the definition is float64: the same route with its positions rounded to float32 (ulp 0.5 m at this northing) gives other
    lists at every radius."""
    pos = routes[4097]
    p32 = pos.astype(np.float32).astype(np.float64)
    assert np.abs(p32 - pos).max() > 0.05
    for r in RADII:
        a, b = R.radius_lists(pos, pos, r), R.radius_lists(p32, p32, r)
        ra, rb = R.rows_of(a[0], a[1]), R.rows_of(b[0], b[1])
        changed = sum(len(np.setxor1d(x, y)) for x, y in zip(ra, rb))
        print(f"MEASURE places/fp32-guard/r{r:g} memberships changed {changed} of {a[1].size}")
        assert changed > 0


def test_in_test_regions_against_the_reference_loop():
    from lpdnet_hip import places
    centres = [[1000.0, 2000.0], [1200.0, 2100.0], [5000.0, -300.0]]      # two overlap

    def check_in_test_set(northing, easting, points, x_width, y_width):      # generate_test_sets.py:37-43
        in_test_set = False
        for point in points:
            if (point[0] - x_width < northing and northing < point[0] + x_width and point[1] - y_width < easting and easting < point[1] + y_width):
                in_test_set = True
                break
        return in_test_set
    g = np.random.default_rng(3)
    pts = np.concatenate((g.uniform([700, 1700], [1500, 2400], size=(400, 2)), g.uniform([4700, -600], [5300, 0], size=(100, 2)),
                          [[850.0, 2000.0], [1150.0, 2000.0], [1000.0, 1850.0], [1000.0, 2150.0], [1150.0, 2150.0],      # on edges: outside
                           [1350.0, 2100.0], [np.nextafter(850.0, 1e9), 2000.0], [np.nan, 2000.0]]))
    for xw, yw in ((150, 150), (40, 260)):
        want = np.array([check_in_test_set(n, e, centres, xw, yw) for n, e in pts])
        got = places.in_test_regions(pts, centres, xw, yw)
        assert got.dtype == bool and np.array_equal(got, want)
    got = places.in_test_regions(pts, centres)
    assert got[:500].any() and not got[:500].all()
    assert got[-8:].tolist() == [False, True, False, False, True, False, True, False]      # (1150, 2000) and (1150, 2150) lie inside region 2
    assert not places.in_test_regions(pts, np.zeros((0, 2))).any()
    assert np.array_equal(places.in_test_regions(torch.from_numpy(pts), centres), got)
    sig = inspect.signature(places.in_test_regions)
    assert sig.parameters["x_width"].default == 150 and sig.parameters["y_width"].default == 150
    src = open(places.__file__).read()
    assert "5735712" not in src and "620084" not in src and "363621" not in src      # no coordinates of the reference in the package


def _three_runs():
    """three runs of (40, 70, 1) database items on one road; the queries of a run are its items inside two regions"""
    from lpdnet_hip import places
    road = R.route(222, seed=9)
    db = [road[0:40] + 1.0, road[20:160:2] - 2.0, road[30:31] + 0.5]
    centres = [road[25], road[110]]
    qs = [d[places.in_test_regions(d, centres, 60, 60)] for d in db]
    return db, qs


def test_truth_table_round_trip():
    from lpdnet_hip import harness, places
    db, qs = _three_runs()
    assert [len(d) for d in db] == [40, 70, 1] and all(len(q) >= 1 for q in qs) and len(qs[0]) < 40
    off, idx = R.truth_table(db, qs, 25.0)
    table = places.TruthTable(torch.from_numpy(off), torch.from_numpy(idx), [len(q) for q in qs], 3, 25.0)
    assert len(table) == 3 and table.q_counts == [len(q) for q in qs] and table.n_db_runs == 3
    sets = table.to_query_sets()
    assert len(sets) == 3 and all(sorted(sets[n][0]) == [m for m in range(3) if m != n] for n in range(3))
    o2, i2 = harness.build_truth_csr(sets, table.q_counts, 3, harness.all_pairs(3))
    assert o2.dtype == np.int32 and np.array_equal(o2, off) and np.array_equal(i2, idx)
    assert idx.size > 0 and all(off[g * 3 + n] == off[g * 3 + n + 1] for n in range(3)
                                for g in range(sum(table.q_counts[:n]), sum(table.q_counts[:n + 1])))      # own-run rows are empty


def test_from_positions_has_no_cpu_path():
    from lpdnet_hip import LpdHipError, ops, places, tuples
    clouds = np.zeros((12, 8, 3), dtype=np.float32)
    pos = R.route(12, seed=1)
    with pytest.raises(LpdHipError):
        tuples.TupleBank.from_positions(clouds, pos, device="cpu")
    with pytest.raises(LpdHipError):
        places.training_lists(pos, device="cpu")
    with pytest.raises(LpdHipError):
        places.evaluation_truth([pos], [pos], device="cpu")
    with pytest.raises(LpdHipError):
        ops.radius_lists(torch.from_numpy(pos), torch.from_numpy(pos), 10.0)
    if not torch.cuda.is_available():
        with pytest.raises(LpdHipError):
            tuples.TupleBank.from_positions(clouds, pos)
    with pytest.raises(ValueError):
        tuples.TupleBank.from_positions(np.zeros((12, 8, 2)), pos, device="cpu")      # the shape is checked first


def test_public_surface():
    import ctypes
    from lpdnet_hip import _lib, harness, ops, places, tuples
    i, p, d = _lib._c_int, _lib._c_p, ctypes.c_double
    assert _lib.SIGNATURES["lpd_radius_count"] == [p, i, p, i, p, i, d, p, p, p, p]
    assert _lib.SIGNATURES["lpd_radius_fill"] == [p, i, p, i, p, i, d, p, p, p, p, i, p]
    hdr = open(os.path.join(ROOT, "include", "lpd_hip.h")).read()
    assert "int lpd_radius_count(" in hdr and "int lpd_radius_fill(" in hdr and "(dx * dx) + (dy * dy) <= r * r" in hdr
    math = open(MATH_H).read()
    assert "(dx * dx) + (dy * dy) <= r2" in math and "fma" not in math.replace("fused multiply-add", "")
    assert (ops.PLACES_MAX_ITEMS, ops.PLACES_MAX_SEGMENTS, ops.PLACES_CHUNK) == (1 << 22, 4096, 1024)
    for define in ("LPD_PLACES_MAX_ITEMS 4194304", "LPD_PLACES_MAX_SEGMENTS 4096", "LPD_PLACES_CHUNK 1024"):
        assert "#define " + define in hdr and "#define " + define.split()[0] not in math      # the public header's, once
    assert [a for a in inspect.signature(ops.radius_lists).parameters] == ["qpos", "dpos", "radius", "seg_off", "skip_seg", "self_item"]
    sig = inspect.signature(places.training_lists)
    assert [a for a in sig.parameters] == ["positions", "pos_radius", "near_radius", "device"]
    assert sig.parameters["pos_radius"].default == 10.0 and sig.parameters["near_radius"].default == 50.0
    sig = inspect.signature(places.evaluation_truth)
    assert [a for a in sig.parameters] == ["db_positions", "query_positions", "radius", "device"] and sig.parameters["radius"].default == 25.0
    sig = inspect.signature(tuples.TupleBank.from_positions)
    assert [a for a in sig.parameters] == ["clouds", "positions", "pos_radius", "near_radius", "device"]
    assert [a for a in inspect.signature(harness.evaluate_pairs).parameters] == ["DATABASE_VECTORS", "QUERY_VECTORS", "QUERY_SETS", "recall_num",
                                                                                "pairs", "device"]
    src = open(places.__file__).read()
    assert "import oracle" not in src and "from oracle" not in src and "import sklearn" not in src and "from sklearn" not in src
