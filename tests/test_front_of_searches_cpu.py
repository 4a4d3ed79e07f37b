"""Host-side arithmetic of the launches in front of and behind the two kNN searches, against numpy restatements (no GPU):
the address of a neighbour inside lpd_pack_idx16's blocked uint16 lists -- the arithmetic the search's packed store uses
(lpd_idx16_offset) -- and the offsets of the regions of a lpd_knn_pm workspace (lpd_knn_pm_layout)."""
import ctypes

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


@pytest.mark.parametrize("B,C,N,k", [(1, 3, 64, 20), (3, 3, 4096, 20), (2, 64, 4096, 20), (5, 64, 640, 20), (2, 3, 96, 20)])
def test_workspace_layout_offsets(B, C, N, k):
    """xx [B*N] | xp [B*N][2 cp] | tile statistics: centroids [B*nt][2 cp], |c|^2, radius, max |x|^2 ([B*nt] each), all inside
    lpd_knn_workspace_floats"""
    from lpdnet_hip import _lib
    lib = _lib.load()
    base = 1 << 20                                                 # the layout is pointer arithmetic: nothing is dereferenced
    xx, xp, xb, tiles = (ctypes.c_void_p() for _ in range(4))
    rc = lib.lpd_knn_pm_layout(B, C, N, k, ctypes.c_void_p(base), ctypes.byref(xx), ctypes.byref(xp), ctypes.byref(xb), ctypes.byref(tiles))
    assert rc == 0
    cp = 2 if C <= 4 else 32
    nt = (N + 31) // 32
    assert xx.value == base and xp.value == base + 4 * B * N
    assert tiles.value == xp.value + 4 * B * N * 2 * cp
    end_of_stats = tiles.value + 4 * B * nt * (2 * cp + 3)
    total = base + 4 * lib.lpd_knn_workspace_floats(B, C, N, k)
    assert end_of_stats <= total
    if xb.value:                                                   # the bf16 image of the bound pass lies behind the statistics, 16-byte aligned
        assert C == 64 and xb.value % 16 == 0 and end_of_stats <= xb.value < total
