"""The low-precision bound table of the 64-channel kNN search (knn7_bound_kernel), read back from the workspace.

The kernel's candidate-tile loop is software-pipelined (two accumulator sets, epilogue of tile T under the MFMAs of tile T + 1,
peeled first tile, drained last tile, a tail for ranges that are no multiple of the operand ring).  The table it writes must not
have moved by a bit, so this file checks, at the smallest sizes at which each of its paths runs:

  shape            nt    path
  B = 2, N = 416   13    odd tile count (the last wave's second query tile does not exist), one range, a 1-tile tail
  B = 1, N = 1024  32    2 candidate ranges of 16
  B = 3, N = 2048  64    4 ranges
  B = 1, N = 4096  128   8 ranges of 16: the one-cloud launch
  B = 1, N = 4128  129   ranges of 20 with a 9-tile last range; the search reads the bounds from global memory

  * bit identity (first two shapes): the table equals tests/golden/knn_bound_table.npz, which holds what the sequential kernel of
    the commit before the pipeline wrote for the same seeded inputs (tests/golden/make_knn_bound_golden.py).
  * bound property (all shapes, every finite entry u of query q against candidate tile T):
        max_{c in T} pd64(q, c)  <=  u  <=  that maximum + 2 err + one bf16 ulp of u
    pd64 = 2 q.c - |q|^2 - |c|^2 in fp64, no tolerance on the lower side; err = 2 (7.9e-3 |q| |c|_max + xx_max 2^-17 + E0) is the
    error term documented at the kernel.  test_emulated_table_lies_in_the_window (CPU) evaluates the kernel's formula in numpy
    (bf16-rounded operands, the two-term split of -xx / 2, fp32 bound expression) and asserts that ITS table lies inside the same
    window, so the window is neither empty nor fitted to the GPU's output.
  * +inf entries (0x7f80, "visit the tile") only where the emulation is +inf as well.  The diagonal entries T == W are +inf by
    construction -- the tile holds the query itself, pd = 0, and the bound of 0 plus a positive slack is positive -- so the
    share that must be ZERO on random clouds is that of the off-diagonal entries; the diagonal is asserted to be +inf in the
    emulation, not assumed.
  * special inputs at N = 416: a cloud of identical points (every product errs the same way); a cloud with one inf and one NaN
    coordinate, where every entry of the affected candidate tiles and query rows must be +inf.
  * indices: the search that consumed the table equals orc.knn_np on every tie-free row; the excluded rows are under 1 %
    (also asserted for the oracle alone, on the CPU).
"""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

from oracle import lpd_oracle as orc

C, K = 64, 20
INF_BITS = 0x7f80
SHAPES = {"b2_n416": (2, 416), "b1_n1024": (1, 1024), "b3_n2048": (3, 2048), "b1_n4096": (1, 4096), "b1_n4128": (1, 4128)}
GOLDEN_SHAPES = ("b2_n416", "b1_n1024")
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_bound_table.npz")


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(name):
    """Seeded inputs [B, N, 64] fp32 (read-only)."""
    if name == "identical":                      # cloud 0: 416 copies of one point; cloud 1: random
        x = np.random.default_rng(7001).standard_normal((2, 416, C)).astype(np.float32)
        x[0] = x[0, 0]
    elif name == "nonfinite":                    # cloud 0: one inf (point 5, tile 0) and one NaN (point 300, tile 9); cloud 1: random
        x = np.random.default_rng(7002).standard_normal((2, 416, C)).astype(np.float32)
        x[0, 5, 3] = np.inf
        x[0, 300, 7] = np.nan
    else:
        B, N = SHAPES[name]
        x = np.random.default_rng(7100 + sorted(SHAPES).index(name)).standard_normal((B, N, C)).astype(np.float32)
    x.setflags(write=False)
    return x


def input_digest(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8)


# ---- references (fp64) and the numpy statement of the kernel's formula ------------------------------------------------------
def bits_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _bf16_round(v):
    """fp32 -> nearest-even bf16, returned as fp32."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def window(name):
    """(max pd64 over each candidate tile, err) as fp64 [B, W, T, 32] of the finite clouds; non-finite clouds are left NaN."""
    x = cloud(name)
    B, N, _ = x.shape
    nt = N // 32
    mx = np.full((B, nt, nt, 32), np.nan)
    err = np.full((B, nt, nt, 32), np.nan)
    for b in range(B):
        if not np.isfinite(x[b]).all():
            continue
        xd = x[b].astype(np.float64)
        xx = (xd * xd).sum(-1)
        pd = 2.0 * (xd @ xd.T) - xx[:, None] - xx[None, :]
        mx[b] = pd.reshape(nt, 32, nt, 32).max(-1).transpose(0, 2, 1)
        txmax = xx.reshape(nt, 32).max(-1)
        e0 = 8.0 * (C + 8) * 2.0 ** -23 * txmax.max()
        qn = np.sqrt(xx).reshape(nt, 1, 32)
        err[b] = 2.0 * (7.9e-3 * qn * np.sqrt(txmax)[None, :, None] + (txmax * 2.0 ** -17)[None, :, None] + e0)
    mx.setflags(write=False)
    err.setflags(write=False)
    return mx, err


@functools.lru_cache(maxsize=None)
def emulated_table(name):
    """The kernel's formula in numpy: uint16 [B, W, T, 32]."""
    f32 = np.float32
    x = cloud(name)
    B, N, _ = x.shape
    nt = N // 32
    out = np.empty((B, nt, nt, 32), np.uint16)
    with np.errstate(all="ignore"):
        for b in range(B):
            xx = (x[b] * x[b]).sum(-1, dtype=f32)
            txmax = xx.reshape(nt, 32).max(-1)
            if np.isnan(xx).any():
                txmax[:] = np.nan                                    # the device's running maximum need not keep a NaN; its E0 is non-finite either way
            smax = txmax.max()
            e0 = f32(f32(f32(8.0) * f32(C + 8) * f32(1.1920929e-7)) * smax) + f32(1e-30)
            xb = _bf16_round(x[b]).astype(np.float64)
            half = f32(-0.5) * xx
            hi = _bf16_round(half)
            lo = _bf16_round(half - hi)
            s = (xb @ xb.T + hi.astype(np.float64)[None, :] + lo.astype(np.float64)[None, :]).astype(f32)     # [q, c]
            m = s.reshape(nt, 32, nt, 32).max(-1).transpose(0, 2, 1)                                         # [W, T, q]
            kq = ((np.sqrt(xx) * f32(1.0001) + f32(1e-30)) * f32(7.9e-3)).reshape(nt, 1, 32)
            nct = (np.sqrt(txmax) * f32(1.0001))[None, :, None]
            ct = (f32(2.0) * (txmax * f32(7.62939453125e-6) + e0))[None, :, None]
            ub = (f32(2.0) * m - xx.reshape(nt, 1, 32)) + (f32(2.0) * (kq * nct) + ct)
            ub = (ub + np.abs(ub) * f32(9.5367431640625e-7)).astype(f32)
            bits = np.ascontiguousarray(ub).view(np.uint32) >> 16
            out[b] = np.where(ub <= 0, bits, INF_BITS).astype(np.uint16)
    out.setflags(write=False)
    return out


def assert_in_window(name, table, what):
    """Both sides of the bound property for every finite entry of the finite clouds; returns the mask of +inf entries."""
    mx, err = window(name)
    inf = table == INF_BITS
    u = bits_to_f32(table).astype(np.float64)
    assert not np.isnan(u).any() and not (np.isinf(u) & ~inf).any(), f"{what}: entries that are neither finite nor 0x7f80"
    chk = ~inf & ~np.isnan(mx)
    assert chk.any(), f"{what}: the window is checked on no entry"
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(u), 2.0 ** -126))) - 7)
    with np.errstate(invalid="ignore"):                              # +inf and NaN entries are masked out below
        low = u - mx
        high = u - (mx + 2.0 * err + ulp)
    print(f"{what} {name}: finite {int(chk.sum())} of {chk.size}; min (u - max pd64) {low[chk].min():.3e}; "
          f"max (u - upper limit) {high[chk].max():.3e}; mean 2 err {2.0 * err[chk].mean():.3e}")
    assert (low[chk] >= 0).all(), f"{what}: {int((low[chk] < 0).sum())} entries below the exact maximum, worst {low[chk].min():.3e}"
    assert (high[chk] <= 0).all(), f"{what}: {int((high[chk] > 0).sum())} entries above the window, worst {high[chk].max():.3e}"
    return inf


def assert_inf_where_emulated(name, table, random_clouds):
    emu_inf = emulated_table(name) == INF_BITS
    inf = table == INF_BITS
    assert not (inf & ~emu_inf).any(), f"{int((inf & ~emu_inf).sum())} +inf entries where the emulated bound is finite"
    diag = np.eye(table.shape[1], dtype=bool)
    for b in random_clouds:
        assert emu_inf[b][diag].all(), "emulation: a query's own tile must carry a positive bound"
        off = inf[b] & ~diag[:, :, None]
        assert not off.any(), f"cloud {b}: {int(off.sum())} off-diagonal entries say 'visit' on a random cloud"


# ---- CPU: the window and the oracle, without a GPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES) + ["identical"])
def test_emulated_table_lies_in_the_window(name):
    table = emulated_table(name)
    assert_in_window(name, table, "emulation")
    assert_inf_where_emulated(name, table, random_clouds=range(table.shape[0]) if name in SHAPES else [1])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_oracle_tie_rows_under_one_percent(name):
    tie = orc.knn_tie_rows(cloud(name), K)
    assert tie.mean() < 0.01, tie.mean()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_run(name):
    """One search through lpd_knn_pm with a workspace this file owns -> (idx [B, N, K] int32, table int16 [B, nt, nt, 32])."""
    import torch
    from lpdnet_hip import ops
    x = cloud(name)
    B, N, _ = x.shape
    nt = N // 32
    dev = torch.device("cuda:0")
    lib = ops._lib.load()
    rows = torch.from_numpy(np.array(x).reshape(B * N, C)).to(dev)         # a copy: the cached input is read-only
    idx = torch.empty((B, N, K), dtype=torch.int32, device=dev)
    ws = torch.zeros((ops.knn_workspace_floats(B, C, N, K),), dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ops._lib.check(lib.lpd_knn_pm(p(rows), C, B, C, N, K, p(idx), p(ws), 0, ops._stream()), "lpd_knn_pm")
    xx, xp, xb, tiles = (ctypes.c_void_p() for _ in range(4))
    ops._lib.check(lib.lpd_knn_pm_layout(B, C, N, K, p(ws), ctypes.byref(xx), ctypes.byref(xp), ctypes.byref(xb), ctypes.byref(tiles)),
                   "lpd_knn_pm_layout")
    assert xb.value, "the low-precision pass does not run at this size"
    first = (xb.value - ws.data_ptr()) // 2 + B * nt * 32 * 80
    count = B * nt * nt * 32
    assert (xb.value - ws.data_ptr()) % 2 == 0 and (first + count) * 2 <= ws.numel() * 4
    torch.cuda.synchronize()
    table = ws.view(torch.int16)[first:first + count].cpu().numpy().reshape(B, nt, nt, 32)
    got = idx.cpu().numpy()
    table.setflags(write=False)
    got.setflags(write=False)
    return got, table


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_SHAPES)
def test_table_bit_identical_to_the_sequential_kernel(cuda, name):
    with np.load(GOLDEN_FILE) as z:
        want, digest = z["table_" + name], z["input_sha256_" + name]
    assert np.array_equal(digest, input_digest(cloud(name))), "the seeded inputs are not the ones the fixture was recorded on"
    _, table = device_run(name)
    diff = table != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} entries differ; first {np.argwhere(diff)[:3].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_table_bounds_every_tile(cuda, name):
    _, table = device_run(name)
    table = table.view(np.uint16)
    assert_in_window(name, table, "device")
    assert_inf_where_emulated(name, table, random_clouds=range(table.shape[0]))


@pytest.mark.gpu
def test_identical_points(cuda):
    _, table = device_run("identical")
    table = table.view(np.uint16)
    assert_in_window("identical", table, "device")
    assert_inf_where_emulated("identical", table, random_clouds=[1])


@pytest.mark.gpu
def test_inf_and_nan_coordinates(cuda):
    _, table = device_run("nonfinite")
    table = table.view(np.uint16)
    assert (table[0, :, 0] == INF_BITS).all() and (table[0, :, 9] == INF_BITS).all(), "candidate tiles of the inf / NaN point"
    assert (table[0, 0, :, 5] == INF_BITS).all() and (table[0, 9, :, 300 % 32] == INF_BITS).all(), "query rows of the inf / NaN point"
    assert_in_window("nonfinite", table, "device")                  # cloud 1 (finite) keeps its bounds
    off = (table[1] == INF_BITS) & ~np.eye(13, dtype=bool)[:, :, None]
    assert not off.any(), "the finite cloud of the batch must not be affected"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_indices_equal_the_oracle(cuda, name):
    got, _ = device_run(name)
    x = cloud(name)
    oidx, _ = orc.knn_np(x, K)
    tie = orc.knn_tie_rows(x, K)
    assert tie.mean() < 0.01, tie.mean()
    diff = (got != oidx).any(-1) & ~tie
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} rows differ; first: {np.argwhere(diff)[:3].tolist()}"
