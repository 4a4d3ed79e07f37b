"""The launches folded into their neighbours around the xyz kNN search, each against the launches it replaces, compared as bytes:
the Z-order sort that also leaves the search's operands and tile statistics in its workspace (ops.morton_sort_knn against
ops.morton_sort + the prep and tile-statistics launches of lpd_knn_pm), the search that writes the packed uint16 neighbour lists from
its own final merge (ops.knn_pm16 against ops.knn_pm + ops.pack_idx16), and the whole eval forward with the folds on against the same
forward with them switched off (LPD_DEBUG=no-knn-pack16,no-sort-knn, a fresh interpreter: the library reads the switches once)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import front_of_searches_ref as fos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tie_rows(B, N, C, seed):
    """point-major rows [B*N, C] in which every fourth point of a cloud repeats its predecessor: the squared distances of a query to
    the two copies tie exactly, so the order inside the lists (and the merge of the half-lists) falls to the index"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((B, N, C), generator=g) * 2 - 1)
    x[:, 1::4] = x[:, 0::4]
    return x.reshape(B * N, C).contiguous()


def _regions(B, N, k, ws):
    """the regions of an xyz-search workspace that are in place before the walk, located by lpd_knn_pm_layout -> {name: int32 view}"""
    import ctypes
    from lpdnet_hip import _lib
    lib = _lib.load()
    xx, xp, xb, tiles = (ctypes.c_void_p() for _ in range(4))
    assert lib.lpd_knn_pm_layout(B, 3, N, k, ctypes.c_void_p(ws.data_ptr()), ctypes.byref(xx), ctypes.byref(xp), ctypes.byref(xb),
                                 ctypes.byref(tiles)) == 0
    assert tiles.value, "the best-first search runs on these sizes"
    off = lambda p: (p.value - ws.data_ptr()) // 4
    nbt = B * (N // 32)
    w = ws.view(torch.int32).cpu().numpy()
    t0 = off(tiles)
    return {"xx": w[off(xx):off(xx) + B * N], "xp": w[off(xp):off(xp) + B * N * 4], "cenp": w[t0:t0 + nbt * 4],
            "cnorm": w[t0 + nbt * 4:t0 + nbt * 5], "rad": w[t0 + nbt * 5:t0 + nbt * 6], "txmax": w[t0 + nbt * 6:t0 + nbt * 7]}


def _clouds(kind, B, N):
    g = torch.Generator().manual_seed(1000 + N + B)
    x = torch.rand((B, N, 3), generator=g) * 2 - 1
    if kind == "duplicates":           # many equal points: equal Morton codes, the index decides
        x = x[:, torch.randint(0, 7, (N,), generator=g)]
    elif kind == "identical":          # box scale 0; every tile's radius is the 1e-30 floor (or the rounding of its centroid)
        x = x[:, :1].expand(B, N, 3).clone()
    elif kind == "huge":               # one coordinate of 3e38: its squared norm overflows, txmax of its tile becomes +inf
        x[0, N // 3, 1] = 3e38
    return x.unsqueeze(1).contiguous()


# B, N: two tiles with a padded sort | not a power of two: the padding words must sort last | E = 2 with padding | the product's E = 4 | E = 8
@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,N", [("random", 1, 64), ("random", 2, 96), ("random", 1, 1056), ("random", 3, 4096), ("random", 1, 8192),
                                      ("duplicates", 2, 4096), ("identical", 2, 96), ("huge", 2, 1056)])
def test_sort_leaves_the_xyz_search_operands(cuda, kind, B, N):
    from lpdnet_hip import _lib, ops
    k = 20
    assert ops.morton_sort_knn_applies(N, k), "the fold is the path under test (is LPD_DEBUG set?)"
    x = _clouds(kind, B, N).to(cuda)
    # today's launches: the sort, then lpd_knn_pm on the sorted rows with a workspace of its own
    want_x, want_perm = ops.morton_sort(x, want_perm=True)
    lib = _lib.load()
    ws_ref = torch.zeros((ops.knn_workspace_floats(B, 3, N, k),), dtype=torch.float32, device=cuda)
    idx_ref = torch.empty((B, N, k), dtype=torch.int32, device=cuda)
    rows = want_x.reshape(B * N, 3)
    assert lib.lpd_knn_pm(rows.data_ptr(), 3, B, 3, N, k, idx_ref.data_ptr(), ws_ref.data_ptr(), 0, torch.cuda.current_stream().cuda_stream) == 0
    got_x, ws, perm = ops.morton_sort_knn(x, k, want_perm=True)
    assert torch.equal(got_x.view(torch.int32), want_x.view(torch.int32)) and torch.equal(perm, want_perm)
    want, got = _regions(B, N, k, ws_ref), _regions(B, N, k, ws)
    for name in want:
        assert np.array_equal(got[name], want[name]), (name, int((got[name] != want[name]).sum()), got[name].size)
    assert torch.equal(ops.knn_prepared(ws, B, N, k, C=3), idx_ref)
    assert torch.equal(ops.knn_pm(rows, B, N, k), idx_ref)
    if kind == "huge":
        assert (want["txmax"] == np.float32(np.inf).view(np.int32)).sum() == 1
    if kind == "identical":
        assert (want["rad"].view(np.float32) < 1e-4).all()
    # the packed lists from the prepared workspace
    none, i16 = ops.knn_pm16(None, B, N, k, want_idx=False, ws=ws)
    assert none is None and torch.equal(i16, ops.pack_idx16(idx_ref))


# B, N: (1, 64) and (1, 4096) run four waves per query tile (wave 0 merges four lists), (8, 4096) one wave per tile
@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("B,N", [(1, 64), (1, 4096), (8, 4096)])
def test_walk_writes_the_packed_lists(cuda, B, N, C):
    from lpdnet_hip import ops
    assert ops.knn_pm16_fused(C, N, 20), "the search's own packed store is the path under test (is LPD_DEBUG set?)"
    x = tie_rows(B, N, C, 100 + N + C).to(cuda)
    want_idx = ops.knn_pm(x, B, N, 20)
    want16 = ops.pack_idx16(want_idx)
    # both forms requested
    idx, i16 = ops.knn_pm16(x, B, N, 20, want_idx=True)
    assert idx is not None and idx.dtype == torch.int32 and i16.dtype == torch.int16 and i16.shape == want16.shape
    assert torch.equal(idx, want_idx)
    assert np.array_equal(i16.cpu().numpy().view(np.uint8), want16.cpu().numpy().view(np.uint8))
    # the packed form alone: no int32 lists are written
    none, i16b = ops.knn_pm16(x, B, N, 20, want_idx=False)
    assert none is None
    assert np.array_equal(i16b.cpu().numpy().view(np.uint8), want16.cpu().numpy().view(np.uint8))
    # the fixture does what it is for: ties are in the lists (a point's copy is at distance 0, like the point itself)
    nb = want_idx.view(B, N, 20)[:, 1::4, :2].cpu().numpy()
    me = np.arange(N)[1::4]
    assert (np.sort(nb, axis=-1) == np.stack([me - 1, me], axis=-1)[None]).all()


@pytest.mark.gpu
def test_packed_lists_outside_the_guard(cuda):
    """the ascending scan (impl 4) has no packed store: both forms still come back (search, then the pack launch), and asking for the
    packed form alone is refused at the C entry"""
    from lpdnet_hip import _lib, ops
    B, N = 2, 96
    x = tie_rows(B, N, 3, 7).to(cuda)
    assert not ops.knn_pm16_fused(3, N, 20, impl=4)
    want_idx = ops.knn_pm(x, B, N, 20, impl=4)
    idx, i16 = ops.knn_pm16(x, B, N, 20, want_idx=False, impl=4)
    assert torch.equal(idx, want_idx) and torch.equal(i16, ops.pack_idx16(want_idx))
    lib = _lib.load()
    ws = torch.empty((ops.knn_workspace_floats(B, 3, N),), dtype=torch.float32, device=cuda)
    rc = lib.lpd_knn_pm16(x.data_ptr(), 3, B, 3, N, 20, None, i16.data_ptr(), ws.data_ptr(), 4, None)
    assert rc != 0 and b"lpd_knn_pm16" in lib.lpd_last_error()
    rc = lib.lpd_knn_pm16(x.data_ptr(), 3, 1, 3, 80, 20, idx.data_ptr(), i16.data_ptr(), ws.data_ptr(), 0, None)      # N % 32 != 0
    assert rc != 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_whole_forward_equals_the_forward_without_the_fold(cuda, tmp_path):
    from lpdnet_hip import ops
    assert ops.knn_pm16_fused(3, 4096, 20) and ops.morton_sort_knn_applies(4096, 20), "the default path is the one under test (is LPD_DEBUG set?)"
    got = fos.forwards()
    out = str(tmp_path / "off.npz")
    env = dict(os.environ, LPD_DEBUG="no-knn-pack16,no-sort-knn")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_of_searches_ref.py"), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as want:
        assert sorted(want.files) == sorted(got)
        for name in got:
            assert got[name].shape[1] == 256 and np.isfinite(got[name]).all()
            assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["b2"], got["b2_again"])
    assert np.array_equal(got["b32_stream0_rep0"], got["b32_stream0_rep1"]) and np.array_equal(got["b32_stream1_rep0"], got["b32_stream1_rep1"])
