"""Shared by tests/test_knn_sorted_walk_cpu.py, tests/test_knn_sorted_walk_gpu.py and the fresh interpreter the latter starts with
LPD_DEBUG=no-knn-sorted: the numpy statement of the walk in bound order (image, key, stop rule: csrc/lpd_knn.hip, knn7_kernel<SORTED>),
the seeded clouds, and the searches whose output the two walks must agree on bit for bit.   python tests/knn_sorted_walk_ref.py OUT.npz"""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

C = 64
INF_BITS = 0x7f80

# name: (B, N, k).  The single-wave kernel runs where B * ceil(N / 32) > 512 (below that four waves share a query tile), so the
# shapes are small clouds in larger batches.
CASES = {
    "nt2": (260, 64, 20),             # the smallest walk; most lanes hold no tile
    "nt3": (180, 96, 20),             # odd count, one register of the order nearly empty
    "nt13": (40, 416, 20),            # the bound test's own size
    "nt65": (9, 2080, 20),            # the order crosses from the first register into the second
    "nt128": (5, 4096, 20),           # both registers full: the product's shape
    "partial": (20, 1000, 20),        # 32 tiles, the last one partial: branchy body, padded queries excluded from the stop test
    "nt13_k5": (40, 416, 5),          # short neighbourhood in the 20-entry lists
    "clusters": (40, 416, 20),        # every cloud: tiles 0 .. 5 around -25 e0, tiles 6 .. 12 around +25 e0 (50 standard deviations apart)
    "identical": (40, 416, 20),       # cloud 0: 416 copies of one point (every bound equal, every pd tied); the others random
    "nonfinite": (40, 416, 20),       # cloud 0: one inf (point 5, tile 0) and one NaN (point 300, tile 9) coordinate; the others random
}
CLUSTER_TILES = 6                     # tiles of the first cluster
ORDER_CASES = ("nt13", "nt65", "nt128")


@functools.lru_cache(maxsize=None)
def cloud(name):
    """Seeded inputs [B, N, 64] fp32 (read-only)."""
    B, N, _ = CASES[name]
    x = np.random.default_rng(8100 + sorted(CASES).index(name)).standard_normal((B, N, C)).astype(np.float32)
    if name == "clusters":
        x[:, :CLUSTER_TILES * 32, 0] -= 25.0
        x[:, CLUSTER_TILES * 32:, 0] += 25.0
    elif name == "identical":
        x[0] = x[0, 0]
    elif name == "nonfinite":
        x[0, 5, 3] = np.inf
        x[0, 300, 7] = np.nan
    x.setflags(write=False)
    return x


# ---- the walk in bound order, in numpy ---------------------------------------------------------------------------------------
def bits_to_f32(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def image(u):
    """16-bit image of a table entry (bf16 bit pattern): unsigned ascending order of the image = descending order of the floats."""
    u = np.asarray(u).astype(np.uint32) & 0xffff
    return np.where(u & 0x8000, u, 0x7fff - u).astype(np.uint32)


def keys(table):
    """table [..., T, 32] uint16 (one wave's rows: candidate tile, query) -> keys [..., T] uint32: score image << 8 | tile."""
    t = np.asarray(table).view(np.uint16) if np.asarray(table).dtype == np.int16 else np.asarray(table)
    score = image(t).min(-1)
    return (score << 8) | np.arange(t.shape[-2], dtype=np.uint32)


def walk_order(table, slots=128):
    """the sorted keys of every wave, padded with 0xffffffff to the kernel's 128 positions, as the int32 the statistics variant writes"""
    k = np.sort(keys(table), axis=-1)
    pad = np.full(k.shape[:-1] + (slots - k.shape[-1],), 0xffffffff, np.uint32)
    return np.concatenate([k, pad], -1).view(np.int32)


def stop_position(sorted_keys, thr_min):
    """first walk position whose score, as a float, is below thr_min (len(sorted_keys) if none): the walk ends in front of it"""
    score = bits_to_f32(image(np.asarray(sorted_keys, np.uint32) >> 8))
    with np.errstate(invalid="ignore"):
        below = score < np.float32(thr_min)
    return int(np.argmax(below)) if below.any() else len(sorted_keys)


# ---- the searches (GPU) ---------------------------------------------------------------------------------------------------------
def searches(name):
    """lpd_knn_pm -> idx int32 [B, N, k]; lpd_knn_pm16 with the int32 lists dropped -> the packed uint16 blocks (k = 20, whole tiles)"""
    import torch
    from lpdnet_hip import ops
    B, N, k = CASES[name]
    rows = torch.from_numpy(np.array(cloud(name)).reshape(B * N, C)).cuda()
    out = {name + "__idx": ops.knn_pm(rows, B, N, k).cpu().numpy()}
    if k == 20 and N % 32 == 0:
        assert ops.knn_pm16_fused(C, N, k), "the search's own packed store is the path under test (is LPD_DEBUG set?)"
        none, i16 = ops.knn_pm16(rows, B, N, k, want_idx=False)
        assert none is None
        out[name + "__idx16"] = i16.cpu().numpy().view(np.uint16)
    return out


def statistics(name):
    """the statistics variant (impl 5) with a workspace of its own -> (raw int32 [B, N, k], bound table uint16 [B, nt, nt, 32])"""
    import torch
    from lpdnet_hip import ops
    B, N, k = CASES[name]
    nt = (N + 31) // 32
    lib = ops._lib.load()
    rows = torch.from_numpy(np.array(cloud(name)).reshape(B * N, C)).cuda()
    raw = torch.zeros((B, N, k), dtype=torch.int32, device="cuda")
    ws = torch.zeros((ops.knn_workspace_floats(B, C, N, k),), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ops._lib.check(lib.lpd_knn_pm(p(rows), C, B, C, N, k, p(raw), p(ws), 5, ops._stream()), "lpd_knn_pm")
    xx, xp, xb, tiles = (ctypes.c_void_p() for _ in range(4))
    ops._lib.check(lib.lpd_knn_pm_layout(B, C, N, k, p(ws), ctypes.byref(xx), ctypes.byref(xp), ctypes.byref(xb), ctypes.byref(tiles)),
                   "lpd_knn_pm_layout")
    assert xb.value, "the low-precision pass does not run at this size"
    first = (xb.value - ws.data_ptr()) // 2 + B * nt * 32 * 80
    count = B * nt * nt * 32
    assert (xb.value - ws.data_ptr()) % 2 == 0 and (first + count) * 2 <= ws.numel() * 4
    torch.cuda.synchronize()
    table = ws.view(torch.int16)[first:first + count].cpu().numpy().view(np.uint16).reshape(B, nt, nt, 32)
    return raw.cpu().numpy(), table


if __name__ == "__main__":
    res = {}
    for case in CASES:
        res.update(searches(case))
    np.savez(sys.argv[1], **res)
