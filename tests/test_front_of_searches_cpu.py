"""Host-side arithmetic of the launches in front of and behind the two kNN searches, against numpy restatements (no GPU):
the address of a neighbour inside lpd_pack_idx16's blocked uint16 lists -- the arithmetic the search's packed store uses
(lpd_idx16_offset) -- and the offsets of the regions of a lpd_knn_pm workspace (lpd_knn_pm_layout, csrc/lpd_knn_ws.h) in closed
form; the workspace sizes, layouts and route answers (lpd_knn_pm16_fused, lpd_morton_sort_knn_applies) over a grid of sizes against
what the library recorded before the layout and the routing were written once (tests/golden/make_knn_host_golden.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest


def packed_positions(M, k=20):
    """numpy restatement of pack_idx16_kernel's layout (csrc/lpd_edge.hip): per 32 rows 1280 bytes =
    [32 x 16 B: neighbours 0-7 | 32 x 16 B: neighbours 8-15 | 32 x 8 B: neighbours 16-19]; -> uint16 position of (row, neighbour)"""
    assert k == 20
    m = np.arange(M, dtype=np.int64)[:, None]
    s = np.arange(k, dtype=np.int64)[None, :]
    quad = s // 4                                                  # the kernel moves one quad (4 neighbours, a uint2) per thread
    blk = (m >> 5) * 160                                           # uint2 units
    p = m & 31
    u2 = np.where(quad < 4, blk + (quad >> 1) * 64 + p * 2 + (quad & 1), blk + 128 + p)
    return u2 * 4 + (s & 3)                                        # uint16 units


def pack_idx16_np(idx):
    """int32 [M, 20] -> the blocked uint16 lists (values 16 * index mod 2^16) as a flat uint16 array"""
    M, k = idx.shape
    out = np.zeros(M * k, dtype=np.uint16)
    out[packed_positions(M, k).ravel()] = ((idx.astype(np.int64) << 4) & 0xffff).astype(np.uint16).ravel()
    return out


@pytest.mark.parametrize("M", [32, 64, 96, 4096, 5 * 640])
def test_packed_block_offsets_match_the_layout(M):
    from lpdnet_hip import _lib
    lib = _lib.load()
    pos = packed_positions(M)
    got = np.array([[lib.lpd_idx16_offset(m, s) for s in range(20)] for m in range(M)], dtype=np.int64)
    assert np.array_equal(got, pos * 2)
    assert np.array_equal(np.sort(got.ravel()), np.arange(M * 20) * 2), "every uint16 of the M/32 blocks is written exactly once"
    # a query's three pieces are contiguous and aligned: 16 B + 16 B + 8 B
    for s0, n, align in ((0, 8, 16), (8, 8, 16), (16, 4, 8)):
        assert (got[:, s0] % align == 0).all() and (got[:, s0:s0 + n] - got[:, s0:s0 + 1] == np.arange(n)[None, :] * 2).all()
    # the 32 queries of a wave (rows 32 w .. 32 w + 31) fill exactly one 1280-byte block
    assert np.array_equal(got.reshape(M // 32, 32 * 20).min(axis=1), np.arange(M // 32) * 1280)
    assert np.array_equal(got.reshape(M // 32, 32 * 20).max(axis=1), np.arange(M // 32) * 1280 + 1278)


def test_packed_block_offsets_far_rows_and_bad_arguments():
    from lpdnet_hip import _lib
    lib = _lib.load()
    m = (1 << 33) + 37                                             # byte offsets past 2^32: 64-bit arithmetic
    assert lib.lpd_idx16_offset(m, 0) == (m >> 5) * 1280 + (m & 31) * 16
    assert lib.lpd_idx16_offset(m, 19) == (m >> 5) * 1280 + 1024 + (m & 31) * 8 + 6
    assert lib.lpd_idx16_offset(-1, 0) == -1 and lib.lpd_idx16_offset(0, 20) == -1 and lib.lpd_idx16_offset(0, -1) == -1


def test_pack_restatement_round_trips():
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 4096, size=(96, 20), dtype=np.int32)
    packed = pack_idx16_np(idx)
    assert np.array_equal(packed[packed_positions(96)], (idx * 16).astype(np.uint16))


def pm_layout(lib, B, C, N, k, base):
    """lpd_knn_pm_layout at an integer base address (pointer arithmetic: nothing is dereferenced) -> (rc, xx, xp, xb, tiles), None = null"""
    xx, xp, xb, tiles = (ctypes.c_void_p() for _ in range(4))
    rc = lib.lpd_knn_pm_layout(B, C, N, k, ctypes.c_void_p(base), ctypes.byref(xx), ctypes.byref(xp), ctypes.byref(xb), ctypes.byref(tiles))
    return rc, xx.value, xp.value, xb.value, tiles.value


@pytest.mark.parametrize("B,C,N,k", [(1, 3, 64, 20), (3, 3, 4096, 20), (2, 64, 4096, 20), (5, 64, 640, 20), (2, 3, 96, 20), (3, 64, 16384, 20),
                                     (1, 64, 16416, 20), (3, 33, 100, 7), (1, 64, 96, 20)])
def test_workspace_layout_offsets(B, C, N, k):
    """xx [B*N] | xp [B*N][2 cp] | tile statistics: centroids [B*nt][2 cp], |c|^2, radius, max |x|^2 ([B*nt] each, 4 floats of guard) |
    walk-length estimates, launch order (int32 [B*nt] each, 4 of guard) | with the bound pass (cp = 32, nt <= 512): the bf16 image at the
    next 16-byte boundary, the bound table, 16 floats of slack | 8 floats of slack = lpd_knn_workspace_floats"""
    from lpdnet_hip import _lib
    lib = _lib.load()
    base = 1 << 20
    rc, xx, xp, xb, tiles = pm_layout(lib, B, C, N, k, base)
    assert rc == 0
    cp = 2 if C <= 4 else 32
    nt = (N + 31) // 32
    assert xx == base and xp == base + 4 * B * N
    assert tiles == xp + 4 * B * N * 2 * cp
    end_of_order = tiles + 4 * (B * nt * (2 * cp + 5) + 8)
    bound = cp == 32 and nt <= 512
    def up16(a):
        return (a + 15) // 16 * 16
    prep_writes_xb = bound and C == 64 and N % 32 == 0             # (the space is reserved for every cp = 32 search with nt <= 512)
    assert xb == (up16(end_of_order) if prep_writes_xb else None)
    end = end_of_order + 4 * 8 + (4 * (B * nt * 32 * 40 + B * nt * nt * 16 + 16) if bound else 0)      # whatever the padding in front of xb
    assert base + 4 * lib.lpd_knn_workspace_floats(B, C, N, k) == end
    # a base 4 bytes past a 16-byte boundary: the bf16 image is aligned as an ADDRESS, everything else moves with the base
    assert pm_layout(lib, B, C, N, k, base + 4) == (0, xx + 4, xp + 4, up16(end_of_order + 4) if prep_writes_xb else None, tiles + 4)


# ---- the host-side answers of the kNN entry points, pinned to the commit before their layout and routing were written once -------
HOST_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_host_layout.npz")
HOST_BASE = 1 << 20
HOST_IMPLS = [0, 4, 5, 6, 0 | 256, 4 | 256, 5 | 256, 6 | 256]      # | 256: LPD_KNN_PM_PREPARED
HOST_GRID = [(B, C, N, k) for B in (1, 3, 64) for C in (1, 3, 4, 5, 33, 63, 64, 65, 130)
             for N in (20, 64, 96, 100, 4096, 4128, 16384, 16416, 65536, 65568) for k in (1, 7, 20, 21, 33, 64) if k <= N]


def host_values(lib):
    """what tests/golden/make_knn_host_golden.py records and the tests below compare: per grid point the workspace size, the return code
    and the four regions of lpd_knn_pm_layout as byte offsets from the base (-1: null) at an aligned base and at one 4 bytes further,
    lpd_knn_pm16_fused per impl; lpd_morton_sort_knn_applies per (N, k)"""
    def offsets(B, C, N, k, base):
        r = pm_layout(lib, B, C, N, k, base)
        return [r[0]] + [-1 if p is None else p - base for p in r[1:]]
    nk = sorted({(N, k) for _, _, N, k in HOST_GRID})
    return {"grid": np.array(HOST_GRID, dtype=np.int64),
            "ws_floats": np.array([lib.lpd_knn_workspace_floats(*g) for g in HOST_GRID], dtype=np.int64),
            "layout": np.array([offsets(*g, HOST_BASE) for g in HOST_GRID], dtype=np.int64),
            "layout_odd_base": np.array([offsets(*g, HOST_BASE + 4) for g in HOST_GRID], dtype=np.int64),
            "fused": np.array([[lib.lpd_knn_pm16_fused(C, N, k, impl) for impl in HOST_IMPLS] for _, C, N, k in HOST_GRID], dtype=np.int64),
            "nk": np.array(nk, dtype=np.int64),
            "sort_knn_applies": np.array([lib.lpd_morton_sort_knn_applies(N, k) for N, k in nk], dtype=np.int64)}


def host_mismatches(lib, suffix):
    """names of the recorded arrays (golden keys end in `suffix`) that this library does not reproduce exactly"""
    gold = np.load(HOST_GOLDEN)
    got = host_values(lib)
    return [name for name, v in got.items() if not np.array_equal(v, gold[name + suffix])]


def test_host_layout_and_routes_match_the_recorded_parent():
    from lpdnet_hip import _lib
    assert "knn-pre" not in os.environ.get("LPD_DEBUG", ""), "the default layout is the one recorded"
    assert host_mismatches(_lib.load(), "") == []


def test_host_layout_without_the_bound_pass_matches_the_recorded_parent():
    """LPD_DEBUG=no-knn-pre drops the bf16 image and the bound table from the workspace; the library reads the switch once, so a
    fresh interpreter asks (host arithmetic only: no GPU call)"""
    code = "import test_front_of_searches_cpu as t; from lpdnet_hip import _lib; bad = t.host_mismatches(_lib.load(), '_no_knn_pre'); print('mismatches', bad); raise SystemExit(1 if bad else 0)"
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LPD_DEBUG="no-knn-pre", PYTHONPATH=os.pathsep.join([here, os.path.join(os.path.dirname(here), "lpd-net-pytorch_amd")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches []" in r.stdout, r.stdout + r.stderr
