"""The walk in bound order of the 64-channel kNN search (csrc/lpd_knn.hip, knn7_kernel<SORTED>) on the device.

The single-wave kernel runs only where B * nt > 512 (below that four waves share a query tile and keep the Z-curve), so the shapes are
small clouds in larger batches; C = 64, k = 20 unless said (tests/knn_sorted_walk_ref.py, CASES):

  B x N        nt    why
  260 x 64     2     the smallest walk; most lanes hold no tile
  180 x 96     3     odd count, one register of the order nearly empty
  40 x 416     13    the bound test's own size (also with k = 5, and the three special clouds below)
  9 x 2080     65    the order crosses from the first register into the second
  5 x 4096     128   both registers full: the product's shape
  20 x 1000    32    last tile partial: branchy body, padded queries excluded from the stop test

Special clouds at 40 x 416: two clusters 50 standard deviations apart (tiles 0 .. 5 and 6 .. 12 of every cloud); cloud 0 made of 416
identical points; cloud 0 with one inf and one NaN coordinate.

  1. indices equal orc.knn_np on every row outside orc.knn_tie_rows, the excluded share under 1 % (asserted for the oracle alone in
     tests/test_knn_sorted_walk_cpu.py).  Cloud 0 of the identical-points and non-finite batches is left to 2.
  2. every output bit -- the int32 lists of lpd_knn_pm and the packed uint16 lists of lpd_knn_pm16 -- equals the Z-curve walk's, which
     runs in ONE fresh interpreter with LPD_DEBUG=no-knn-sorted (the library reads the switch once).
  3. at nt = 13, 65 and 128 the walk order that the statistics variant writes for every wave equals the numpy argsort of the keys built
     from the bound table read back from the same workspace.
  4. two clusters: a wave tests the tiles of its own cluster and then stops -- 6 bound tests of 13 tiles in the first cluster (fewer
     than half), 7 in the second.  (Over BOTH clusters a cloud of 13 tiles cannot stay under half: a waves of a tiles and 13 - a waves
     of 13 - a tiles make a^2 + (13 - a)^2 >= 85 tests of 169.)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_sorted_walk_ref as ref
from oracle import lpd_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = sorted(ref.CASES)


@functools.lru_cache(maxsize=None)
def sorted_run(name):
    return ref.searches(name)


@functools.lru_cache(maxsize=None)
def stats_run(name):
    return ref.statistics(name)


@pytest.fixture(scope="module")
def z_curve(tmp_path_factory):
    """every case through the Z-curve walk, in a fresh interpreter"""
    assert "no-knn-sorted" not in os.environ.get("LPD_DEBUG", ""), "the walk in bound order is the path under test"
    out = str(tmp_path_factory.mktemp("knn_sorted_walk") / "z.npz")
    env = dict(os.environ, LPD_DEBUG=",".join(filter(None, [os.environ.get("LPD_DEBUG"), "no-knn-sorted"])))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knn_sorted_walk_ref.py"), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_indices_equal_the_oracle(cuda, name):
    B, N, k = ref.CASES[name]
    got = sorted_run(name)[name + "__idx"]
    x = ref.cloud(name)
    clouds = list(range(1, B)) if name in ("identical", "nonfinite") else list(range(B))
    oidx, _ = orc.knn_np(x[clouds], k)
    tie = orc.knn_tie_rows(x[clouds], k)
    assert tie.mean() < 0.01, tie.mean()
    diff = (got[clouds] != oidx).any(-1) & ~tie
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} rows differ; first: {np.argwhere(diff)[:3].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_every_bit_equals_the_z_curve_walk(cuda, z_curve, name):
    got = sorted_run(name)
    B, N, k = ref.CASES[name]
    assert (name + "__idx16" in got) == (k == 20 and N % 32 == 0)
    for key, val in got.items():
        want = z_curve[key]
        assert val.shape == want.shape and val.dtype == want.dtype
        diff = val != want
        assert not diff.any(), f"{key}: {int(diff.sum())} of {diff.size} words differ; first: {np.argwhere(diff)[:3].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ref.ORDER_CASES)
def test_walk_order_matches_the_host(cuda, name):
    B, N, k = ref.CASES[name]
    nt = N // 32
    raw, table = stats_run(name)
    # row col of wave W carries walk positions col, 32 + col, 64 + col, 96 + col in slots 12 .. 15
    got = raw.reshape(B, nt, 32, k)[:, :, :, 12:16].transpose(0, 1, 3, 2).reshape(B, nt, 128)
    want = ref.walk_order(table)
    diff = got != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} positions differ; first: {np.argwhere(diff)[:3].tolist()}"
    tests = raw.reshape(B, nt, 32, k)[:, :, 0, 11]
    assert (tests >= 1).all() and (tests <= nt).all()


@pytest.mark.gpu
def test_two_clusters_end_the_walk(cuda):
    B, N, k = ref.CASES["clusters"]
    nt, a = N // 32, ref.CLUSTER_TILES
    raw, _ = stats_run("clusters")
    w = raw.reshape(B, nt, 32, k)[:, :, 0, :]
    tests, visited = w[:, :, 11], w[:, :, 0]
    print("bound tests per wave, first / second cluster:", tests[:, :a].mean(), tests[:, a:].mean(), "visited:", visited[:, :a].mean(), visited[:, a:].mean())
    assert (tests[:, :a] <= a).all() and 2 * a < nt, "a wave of the first cluster tests its own tiles: fewer than half the cloud's"
    assert (tests[:, a:] <= nt - a).all(), "a wave of the second cluster tests its own tiles"
    assert (visited <= tests).all()
