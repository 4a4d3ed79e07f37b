"""Op-level parity of the HIP kernels (through the C-ABI) against the oracle.  -m gpu only.

Tolerances: kNN indices bit-exact on tie-free rows; the fp32 kernels of THIS module within 1e-5 of an fp64 torch-CPU evaluation of
the same formula in the norm-relative measure `_rel` = max |a - b| / max |b| over the whole tensor (the end-to-end gate of BASELINE.json
is 1e-4).  That measure cannot see one wrong row or one wrong small element of a softmax or a VLAD descriptor, so the head tests below
carry an element-wise check (`_elem`) beside it, and the modules that run the kernels at their launch sizes measure every element
against its own scale: tests/test_launch_sizes_gpu.py, tests/test_train_bwd_ops_gpu.py and tests/test_fwd_ops_gpu.py scale each error by
the fp64 sum |term| of that element and bound it by a float32 evaluation of the same formula.  The GEMM family (csrc/lpd_gemm.hip,
csrc/lpd_gemm_t.hip, csrc/lpd_gemm_p8.hip) has that measure in tests/test_gemm_routes_gpu.py: every route of the dispatch at its smallest
shape, on inputs with graded row and column scales, each case asserting the ops.PROFILE label of the route it names; the GEMM tests
below keep the norm-relative gate at larger shapes.
"""
import os

import numpy as np
import pytest
import torch

from oracle import lpd_oracle as orc
from oracle import synth

pytestmark = pytest.mark.gpu


def _ops():
    from lpdnet_hip import ops
    return ops


def _rel(a, b):
    a = a.double().cpu()
    b = b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _elem(a, b, scale=None):
    """max over the elements of |a - b| / scale (default |b|: element-wise relative)"""
    a, b = a.double().cpu(), b.double().cpu()
    s = b.abs() if scale is None else scale.double().cpu()
    return ((a - b).abs() / s.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------ kNN
@pytest.mark.parametrize("C,N,k,B", [(3, 4096, 20, 2), (64, 4096, 20, 2), (3, 100, 7, 3), (5, 333, 20, 2),
                                      (64, 1000, 20, 1), (3, 16384, 64, 1), (130, 512, 32, 1), (3, 64, 64, 1),
                                      (64, 2048, 64, 1), (64, 16384, 64, 1), (3, 5000, 33, 2)])
@pytest.mark.parametrize("impl", [0, 1, 2, 6])
def test_knn_bit_exact_vs_oracle(cuda, C, N, k, B, impl):
    """impl 0: product dispatch (best-first walk / ascending scan, MFMA tiles + queued selection); 1: VALU fmaf cross-check; 2: first-generation
    MFMA kernel (the path of 64 < C <= 256); 6: best-first tile order with exact skip bounds, forced.  Other values are refused."""
    if impl == 1 and (k > 20 or N > 4096):
        pytest.skip("VALU cross-check path is built for k <= 20 and is slow")
    if impl == 6 and (k > 64 or C > 64):
        pytest.skip("the best-first kernel is built for k <= 64, C <= 64")
    ops = _ops()
    x_pm = synth.cloud(1000 + C + N, B, N, C)
    oidx, _ = orc.knn_np(x_pm, k)
    tie = orc.knn_tie_rows(x_pm, k)
    x_cm = torch.from_numpy(np.ascontiguousarray(x_pm.transpose(0, 2, 1))).to(cuda)
    idx = ops.knn(x_cm, k, impl=impl).cpu().numpy()
    if impl == 0 and (C, N) == (3, 100):
        with pytest.raises(Exception):      # removed experimental paths (impl 3, timing ablations) are an argument error now
            ops.knn(x_cm, k, impl=3)
    rows_equal = (idx == oidx).all(-1)
    bad = ~rows_equal & ~tie
    assert bad.sum() == 0, f"{bad.sum()} tie-free rows differ (of {bad.size}); first: {np.argwhere(bad)[:3].tolist()}"
    # tie rows must still hold the right SET of pd values: compare as sets where no boundary tie exists
    assert rows_equal.mean() > 0.99
    if impl in (0, 6) and C <= 64 and k <= 64:     # point-major entry (no transposes): the same bits, also from a column slice
        buf = torch.zeros((B * N, C + 5), device=cuda) if C <= 4 else torch.zeros((B * N, 72), device=cuda)
        off = 0 if C > 4 else 2
        buf[:, off:off + C] = torch.from_numpy(x_pm.reshape(B * N, C)).to(cuda)
        got = ops.knn_pm(buf[:, off:off + C], B, N, k, impl=impl).cpu().numpy()
        assert (got == idx).all()


@pytest.mark.parametrize("impl", [0, 4, 2])
@pytest.mark.parametrize("C,N,k", [(3, 1024, 20), (3, 4096, 20), (64, 700, 20), (3, 6000, 64), (64, 5000, 64), (64, 4500, 20), (3, 900, 40), (2, 777, 20), (1, 300, 9)])
def test_knn_exact_ties_lower_index_first(cuda, C, N, k, impl):
    """Clouds on a coarse lattice with duplicated points: thousands of exact pd ties, inside the lists and at the k-th
    boundary.  Every row must equal the oracle's (value descending, lower index first) -- for the best-first kernel this
    exercises both insertion rules (candidates from tiles above / below the wave's own); the k = 64 / N > 4096 cases run its
    large-cloud instantiations (bounds on the fly, 64-entry lists)."""
    if impl == 2 and k > 20 and C > 4:
        pytest.skip("first-generation kernel: slow at this size")
    ops = _ops()
    g = np.random.default_rng(C + N)
    x_pm = (g.integers(-4, 5, size=(2, N, C)) / 4.0).astype(np.float32)
    x_pm[:, N // 2:N // 2 + 40] = x_pm[:, 3:43]                       # exact duplicates far apart in index
    oidx, _ = orc.knn_np(x_pm, k)
    x_cm = torch.from_numpy(np.ascontiguousarray(x_pm.transpose(0, 2, 1))).to(cuda)
    got = ops.knn(x_cm, k, impl=impl).cpu().numpy()
    assert (got == oidx).all(), f"{(got != oidx).any(-1).sum()} rows differ"
    if impl == 0:
        got_pm = ops.knn_pm(torch.from_numpy(x_pm.reshape(-1, C)).to(cuda).contiguous(), 2, N, k).cpu().numpy()
        assert (got_pm == oidx).all()


def _zsort(x):
    """x [B, N, 3] -> the same clouds with their points in Z-curve (Morton) order on a 1024^3 grid of each cloud's bounding box: the order
    lpd_morton_sort gives the model's clouds, in which 8 consecutive points are a compact box and the leaf-box search really prunes."""
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        p = x[b].astype(np.float64)
        lo, hi = p.min(0), p.max(0)
        g = np.clip(((p - lo) / np.maximum(hi - lo, 1e-30) * 1023.0), 0, 1023).astype(np.uint64)
        key = np.zeros(len(p), dtype=np.uint64)
        for bit in range(10):
            for a in range(3):
                key |= ((g[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
        out[b] = x[b][np.argsort(key, kind="stable")]
    return out


@pytest.mark.parametrize("N,k,B", [(4096, 20, 3), (16384, 64, 1), (1000, 20, 2), (520, 7, 2), (72, 64, 2), (16384, 20, 1), (2048, 33, 2)])
@pytest.mark.parametrize("case", ["uniform", "surface", "clusters", "lattice", "offset", "huge", "dupes"])
def test_knn_on_z_ordered_clouds(cuda, N, k, B, case):
    """The xyz search on clouds in Z-curve order -- the model's order (lpd_morton_sort), where the best-first walk's tile bounds decide
    most tiles (on unordered clouds every tile spans the cloud and nearly everything is visited).  Every row equals the oracle's,
    ties by lower index: uniform volumes, a LiDAR-like surface (ground plane + walls: empty space and dense sheets), tight clusters at
    mixed separations, a coarse lattice (exact ties inside the lists and at the k-th boundary), a cloud far from the origin (pd
    quantised at ulp(|x|^2): the slack E0 dominates the bounds), large coordinates, duplicated points."""
    ops = _ops()
    g = np.random.default_rng(N + k + len(case))
    x = g.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    if case == "surface":
        x[:, : N // 2, 2] = (-0.9 + 0.01 * g.normal(0, 1, (B, N // 2))).astype(np.float32)
        x[:, N // 2: 3 * N // 4, 0] = (0.7 + 0.005 * g.normal(0, 1, (B, 3 * N // 4 - N // 2))).astype(np.float32)
    elif case == "clusters":
        nc = max(1, N // 50)
        cen = g.normal(0, 1, (B, nc, 1, 3)) * g.choice([0.05, 0.3, 2.0], (B, nc, 1, 1))
        pts = (cen + 0.02 * g.normal(0, 1, (B, nc, 50, 3))).reshape(B, nc * 50, 3)
        x[:, : nc * 50] = pts[:, :N].astype(np.float32)
    elif case == "lattice":
        x = (g.integers(-4, 5, size=(B, N, 3)) / 4.0).astype(np.float32)
    elif case == "offset":
        x = (x + np.float32(100.0)).astype(np.float32)
    elif case == "huge":
        x = (x * np.float32(3e4)).astype(np.float32)
    elif case == "dupes":
        x[:, N // 2:] = x[:, : N - N // 2]
    x = _zsort(x)
    oidx, _ = orc.knn_np(x, k)
    tie = orc.knn_tie_rows(x, k)
    rows = torch.from_numpy(x.reshape(-1, 3)).to(cuda)
    got = ops.knn_pm(rows, B, N, k).cpu().numpy()
    bad = (got != oidx).any(-1)
    if case in ("lattice", "offset", "dupes"):      # the oracle's tie rule is the contract: every row
        assert bad.sum() == 0, f"{bad.sum()} rows differ; first: {np.argwhere(bad)[:3].tolist()}"
    else:
        assert (bad & ~tie).sum() == 0, f"{(bad & ~tie).sum()} tie-free rows differ; first: {np.argwhere(bad & ~tie)[:3].tolist()}"
    assert (got == ops.knn_pm(rows, B, N, k, impl=4).cpu().numpy()).all()           # best-first walk == ascending scan
    x_cm = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(cuda)    # ... == the channel-major entry
    assert (ops.knn(x_cm, k).cpu().numpy() == got).all()


def test_knn_many_small_clouds(cuda):
    """More work items per XCD than one sorting chunk of the longest-first launch order holds (1100 clouds x 8 tiles =
    8800 items, 1100 per XCD > 1024): best-first == ascending scan, row for row."""
    ops = _ops()
    B, N, k = 1100, 256, 20
    g = torch.Generator().manual_seed(3)
    rows = (torch.rand(B * N, 3, generator=g) * 2 - 1).to(cuda)
    a = ops.knn_pm(rows, B, N, k, impl=0)
    b = ops.knn_pm(rows, B, N, k, impl=4)
    assert torch.equal(a, b)


@pytest.mark.parametrize("impl", [0, 4])
@pytest.mark.parametrize("case", ["offset", "huge", "tiny", "identical", "line", "clusters", "shells", "halfulp"])
@pytest.mark.parametrize("C", [3, 64])
def test_knn_ill_conditioned_clouds(cuda, case, impl, C):
    """Inputs on which the fp32 pd evaluation is badly conditioned or fully degenerate: a cloud far from the origin
    (catastrophic cancellation: pd is quantised at ulp(|x|^2) ~ 1e-3, ties everywhere), very large and very small scales,
    all points identical, all points on a line.  The skip bounds of the best-first kernel must stay conservative (their
    slack scales with max |x|^2) and the tie rule must hold: every row equals the oracle's.  C = 64: the tile bounds come from
    the low-precision pass (bf16 operands, error bound 7.9e-3 |q||c|): far from the origin that bound is useless -- and must be;
    identical points put every product at the maximum rounding error in the same direction (this case caught a bound that was half
    the true one)."""
    ops = _ops()
    g = np.random.default_rng(7)
    N = 2048
    x = g.uniform(-1, 1, (2, N, C)).astype(np.float32)
    if case == "offset":
        x = (x + np.float32(100.0)).astype(np.float32)
    elif case == "huge":
        x = (x * np.float32(3e4)).astype(np.float32)
    elif case == "tiny":
        x = (x * np.float32(1e-4)).astype(np.float32)
    elif case == "identical":
        x[:] = np.float32(0.37)
    elif case == "line":
        x[:, :, 1:] = 0
    elif case == "clusters":     # tile-aligned tight clusters at mixed separations: the regime where tile bounds decide most skips
        cen = g.normal(0, 1, (2, N // 32, 1, C)) * g.choice([0.05, 0.3, 2.0], (2, N // 32, 1, 1))
        x = (cen + 0.02 * g.normal(0, 1, (2, N // 32, 32, C))).reshape(2, N, C).astype(np.float32)
    elif case == "shells":       # every point at (almost) the same distance from every other: thresholds and bounds nearly touch
        x = g.normal(0, 1, (2, N, C))
        x = (x / np.linalg.norm(x, axis=-1, keepdims=True) * (1.0 + 1e-4 * g.normal(0, 1, (2, N, 1)))).astype(np.float32)
    elif case == "halfulp":      # every coordinate just below a bf16 rounding tie (maximal rounding error, all in one direction),
        # in tile-aligned clusters that differ only in bits bf16 does not keep
        base = g.choice([0.25, 0.5, 1.0, 2.0], (2, N // 32, 1, C)) * (1.0 + g.integers(0, 128, (2, N // 32, 1, C)) / 128.0)
        bits = base.astype(np.float32).view(np.uint32) | np.uint32(0x7F00)            # low mantissa 0x7Fxx: rounds DOWN by ~u/2 ... u
        x = (bits + g.integers(0, 0x100, (2, N // 32, 32, C)).astype(np.uint32)).view(np.float32).reshape(2, N, C)
        x = (x * g.choice([-1.0, 1.0], (2, 1, 1, C)).reshape(2, 1, C)).astype(np.float32)
    oidx, _ = orc.knn_np(x, 20)
    got = ops.knn_pm(torch.from_numpy(x.reshape(-1, C)).to(cuda), 2, N, 20, impl=impl).cpu().numpy()
    assert (got == oidx).all(), f"{(got != oidx).any(-1).sum()} rows differ"
    if case == "identical":
        assert (got == np.arange(20)).all()


@pytest.mark.parametrize("tag", ["knn_c3_n4096_k20", "knn_c64_n4096_k20", "knn_c3_n16384_k64", "knn_c3_n100_k7"])
def test_knn_vs_reference_golden(cuda, golden_dir, tag):
    ops = _ops()
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    C, N, k, stride = int(g["C"]), int(g["N"]), int(g["k"]), int(g["row_stride"])
    x_pm = synth.cloud(int(g["cloud_seed"]), 1, N, C)
    x_cm = torch.from_numpy(np.ascontiguousarray(x_pm.transpose(0, 2, 1))).to(cuda)
    idx = ops.knn(x_cm, k).cpu().numpy()[0][::stride]
    ok = (idx == g["idx"].astype(np.int32)).all(-1)
    bad = ~ok & ~g["tie"]
    assert bad.sum() == 0, f"{bad.sum()} tie-free rows differ from the reference"


def test_morton_sort_is_a_permutation_and_improves_locality(cuda):
    ops = _ops()
    pts = torch.from_numpy(synth.cloud(12, 3, 4096)).to(cuda)
    out, perm = ops.morton_sort(pts, want_perm=True)
    p = perm.cpu().long()
    assert (torch.sort(p, dim=1)[0] == torch.arange(4096)).all()                 # a permutation per cloud
    assert torch.equal(out.cpu(), torch.gather(pts.cpu(), 1, p.unsqueeze(-1).expand(-1, -1, 3)))
    # consecutive points are close after sorting, far before
    d_sorted = (out[:, 1:] - out[:, :-1]).norm(dim=-1).mean().item()
    d_raw = (pts[:, 1:] - pts[:, :-1]).norm(dim=-1).mean().item()
    assert d_sorted < 0.25 * d_raw
    # kNN on the sorted cloud = relabelled kNN of the original cloud (tie-free rows)
    idx_s = ops.knn(out.transpose(1, 2).contiguous(), 20).cpu().long()
    idx_o = ops.knn(pts.transpose(1, 2).contiguous(), 20).cpu().long()
    relabelled = torch.gather(p, 1, idx_s.reshape(3, -1)).reshape(3, 4096, 20)      # sorted-row r, neighbours in original ids
    expect = torch.gather(idx_o, 1, p.unsqueeze(-1).expand(-1, -1, 20))             # original kNN rows in sorted order
    same = (torch.sort(relabelled, dim=-1)[0] == torch.sort(expect, dim=-1)[0]).all(-1).float().mean().item()
    assert same > 0.995   # equal up to rows with (near-)ties: pd depends on summation order only through ties


def _morton_order_np(pts):
    """numpy restatement of lpd_morton.hip: fp32 bounding box, 10 bits per axis, stable order by (top bits of the 30-bit code, index):
    the sort word holds 32 - log2(1024 E) code bits, E = keys per thread of the instantiation that serves N."""
    mn, mx = pts.min(0), pts.max(0)
    with np.errstate(divide="ignore"):
        scale = np.where(mx > mn, np.float32(1023.0) / (mx - mn).astype(np.float32), np.float32(0)).astype(np.float32)
    q = np.clip((pts - mn).astype(np.float32) * scale, 0, 1023).astype(np.uint32)

    def spread(v):
        v = v & 0x3ff
        v = (v | (v << 16)) & 0x030000ff
        v = (v | (v << 8)) & 0x0300f00f
        v = (v | (v << 4)) & 0x030c30c3
        return (v | (v << 2)) & 0x09249249
    key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    n = pts.shape[0]
    ib = 10 if n <= 1024 else 11 if n <= 2048 else 12 if n <= 4096 else 13 if n <= 8192 else 14
    return np.argsort(key >> (ib - 2), kind="stable")


@pytest.mark.parametrize("N", [1, 37, 1000, 1024, 1500, 4096, 5000, 16384])
def test_morton_sort_order(cuda, N):
    """Every instantiation of the sorting network (1..16 keys per thread, ragged N, duplicate points = equal keys) against
    the numpy order, element for element."""
    ops = _ops()
    pts = synth.cloud(N + 3, 2, N).copy()
    if N > 40:
        pts[:, 7] = pts[:, 3]; pts[:, N - 1] = pts[:, 3]          # duplicated points: equal keys, index decides
    out, perm = ops.morton_sort(torch.from_numpy(pts).to(cuda), want_perm=True)
    for b in range(2):
        want = _morton_order_np(pts[b])
        assert np.array_equal(perm[b].cpu().numpy(), want.astype(np.int32)), (N, b)
        assert np.array_equal(out[b].cpu().numpy(), pts[b][want])


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K,ak,bk", [(256, 128, 64, False, False), (1000, 200, 96, False, True), (128, 64, 32, False, False),
                                          (77, 513, 128, False, False), (512, 64, 1024, False, True), (300, 1024, 512, False, False),
                                          (132, 72, 64, True, True), (1024, 64, 4096, True, True),
                                          (200, 64, 100, True, True), (96, 40, 52, False, False), (64, 64, 600, False, True)])
@pytest.mark.parametrize("exact", [True, False], ids=["f32mfma", "bf16x3"])
def test_gemm_modes(cuda, M, N, K, ak, bk, exact):
    """exact: f32-input MFMA (one rounding per FMA); otherwise the split-bf16 three-product form, whose error against
    fp64 is bounded here at 3e-5 of the output range (measured ~5e-6)."""
    ops = _ops()
    tol = 1e-5 if exact else 3e-5
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((K, M) if ak else (M, K), generator=g)
    Bm = torch.randn((K, N) if bk else (N, K), generator=g)
    bias, scale, shift = torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    Al = A.t() if ak else A
    Bl = Bm if bk else Bm.t()
    ref = (Al.double() @ Bl.double() + bias.double()) * scale.double() + shift.double()
    ref = torch.where(ref > 0, ref, ref * 0.01)
    out = ops.gemm(A.to(cuda), Bm.to(cuda), a_kmajor=ak, b_kmajor=bk, bias=bias.to(cuda), scale=scale.to(cuda),
                   shift=shift.to(cuda), act=ops.ACT_LEAKY, exact=exact)
    assert _rel(out, ref) < tol
    raw = ops.gemm(A.to(cuda), Bm.to(cuda), a_kmajor=ak, b_kmajor=bk, exact=exact)
    assert _rel(raw, Al.double() @ Bl.double()) < tol
    with ops.exact_gemm():      # the context form of exact=True gives the same bits
        again = ops.gemm(A.to(cuda), Bm.to(cuda), a_kmajor=ak, b_kmajor=bk)
    assert torch.equal(again, raw) == exact or not exact


@pytest.mark.parametrize("M,N,K,splits", [(1, 256, 4096, 16), (17, 200, 5000, 20), (32, 256, 65536, 256), (44, 256, 8200, 32),
                                          (64, 72, 3000, 12), (65, 256, 4096, 16),
                                          (1, 256, 65536, 512), (2, 256, 16384, 64), (3, 512, 8292, 40), (4, 256, 65536, 256), (9, 256, 16384, 128),
                                          (5, 512, 8292, 40), (31, 256, 8200, 40), (32, 256, 65536, 512), (24, 256, 65536, 512)])
def test_gemm_splitk_few_rows(cuda, M, N, K, splits):
    """Few rows against a k-major weight matrix (NetVLAD hidden projection, per-cloud layers): the column-streaming split-K
    kernel for M <= 64 (M = 65: the MFMA kernel), the weight-stream kernels for N % 256 == 0, K >= 8192 -- M <= 4 on the VALU, 5 .. 32 rows
    through the f32-input MFMA (every row count class, a ragged last k-slice, two column blocks) --, ragged K / N, epilogue applied by
    the slab reduction, output slice."""
    ops = _ops()
    g = torch.Generator().manual_seed(M * 7 + N)
    A = torch.randn(M, K + 4, generator=g)[:, :K]
    W = torch.randn(K, N + 8, generator=g)[:, 4:4 + N] / K ** 0.5
    bias, sc, sh = torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    ref = torch.clamp((A.double() @ W.double() + bias.double()) * sc.double() + sh.double(), min=0)
    Ad = torch.zeros(M, K + 4, device=cuda); Ad[:, :K] = A.to(cuda)
    Wd = torch.zeros(K, N + 8, device=cuda); Wd[:, 4:4 + N] = W.to(cuda)
    buf = torch.full((M, N + 8), 7.0, device=cuda)
    ops.gemm(Ad[:, :K], Wd[:, 4:4 + N], b_kmajor=True, bias=bias.to(cuda), scale=sc.to(cuda), shift=sh.to(cuda), act=ops.ACT_RELU,
             splits=splits, exact=True, out=buf[:, 4:4 + N])
    assert _rel(buf[:, 4:4 + N], ref) < 2e-6
    assert (buf[:, :4] == 7).all() and (buf[:, 4 + N:] == 7).all()


@pytest.mark.parametrize("exact", [True, False], ids=["f32mfma", "bf16x3"])
def test_gemm_splitk_and_batched(cuda, exact):
    ops = _ops()
    tol = 1e-5 if exact else 3e-5
    g = torch.Generator().manual_seed(5)
    A = torch.randn(6, 8192, generator=g)
    W = torch.randn(8192, 256, generator=g) / 90
    sc, sh = torch.randn(256, generator=g), torch.randn(256, generator=g)
    prof = ops.PROFILE = {}
    try:
        out = ops.gemm(A.to(cuda), W.to(cuda), b_kmajor=True, scale=sc.to(cuda), shift=sh.to(cuda), splits=16, exact=exact)
    finally:
        ops.PROFILE = None
    # 6 rows are below the wrapper's floor for the split form (M >= 128 and N >= 128): BOTH ids run split-K on the f32-input kernel here;
    # split-K on the split-bf16 kernel is tests/test_gemm_routes_gpu.py (x3/nt_K192_splits3 and its neighbours)
    assert list(prof) == ["gemm[6x256x8192]"], list(prof)
    ref = (A.double() @ W.double()) * sc.double() + sh.double()
    assert _rel(out, ref) < tol
    # batched, A stored k-major (NetVLAD aggregation shape): [b][n][f]^T @ [b][n][c]
    X = torch.randn(3, 512, 256, generator=g)
    Act = torch.rand(3, 512, 64, generator=g)
    prof = ops.PROFILE = {}
    try:
        out = ops.gemm(X.to(cuda), Act.to(cuda), a_kmajor=True, b_kmajor=True, exact=exact)
    finally:
        ops.PROFILE = None
    assert list(prof) == ["gemm[256x64x512]" if exact else "gemmx3[256x64x512]"], list(prof)
    ref = torch.matmul(X.double().transpose(1, 2), Act.double())
    assert out.shape == (3, 256, 64)
    assert _rel(out, ref) < tol


def test_gemm_output_slice_and_strided_input(cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(9)
    X = torch.randn(256, 192, generator=g)
    W = torch.randn(128, 64, generator=g)
    buf = torch.zeros(256, 512, device=cuda)
    ops.gemm(X.to(cuda)[:, 64:128], W.to(cuda), b_kmajor=False, out=buf[:, 128:256])
    ref = X[:, 64:128].double() @ W.double().t()
    assert _rel(buf[:, 128:256], ref) < 1e-5
    assert buf[:, :128].abs().max().item() == 0 and buf[:, 256:].abs().max().item() == 0


# ------------------------------------------------------------------ edge kernels
def _edge_inputs(B, N, C, k, seed):
    g = torch.Generator().manual_seed(seed)
    P = torch.randn(B * N, C, generator=g)
    Q = torch.randn(B * N, C, generator=g)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)]).to(torch.int32)
    scale = torch.randn(C, generator=g)
    shift = torch.randn(C, generator=g)
    return P, Q, idx, scale, shift


def _gather(P, idx, B, N):
    rows = (idx.long() + (torch.arange(B) * N).view(B, 1, 1)).view(B * N, -1)
    return P[rows]  # [M,k,C]


@pytest.mark.parametrize("C,N,k,B", [(256, 512, 20, 2), (128, 256, 20, 3), (64, 200, 20, 2), (256, 128, 64, 1), (64, 96, 5, 1)])
def test_edge_gather_max(cuda, C, N, k, B):
    ops = _ops()
    P, Q, idx, scale, shift = _edge_inputs(B, N, C, k, C + N + k)
    e = scale.double() * (_gather(P, idx, B, N).double() + Q.double().unsqueeze(1)) + shift.double()
    e = torch.where(e > 0, e, e * 0.01)
    ref = e.max(dim=1)[0]
    out = ops.edge_gather_max(P.to(cuda), Q.to(cuda), idx.to(cuda), N, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY)
    assert _rel(out, ref) < 1e-5
    # P and Q as column halves of one GEMM output, result into a slice of the concat buffer
    PQ = torch.cat([P, Q], dim=1).to(cuda)
    buf = torch.zeros(B * N, 2 * C + 64, device=cuda)
    ops.edge_gather_max(PQ[:, :C], PQ[:, C:], idx.to(cuda), N, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY,
                        out=buf[:, 64:64 + C])
    assert _rel(buf[:, 64:64 + C], ref) < 1e-5
    # no centre term, no affine: plain neighbourhood max
    out2 = ops.edge_gather_max(P.to(cuda), None, idx.to(cuda), N)
    assert _rel(out2, _gather(P, idx, B, N).max(dim=1)[0]) == 0.0


@pytest.mark.parametrize("C,N,B,act", [(256, 512, 2, 2), (128, 1000, 3, 1), (64, 37, 2, 0), (256, 4096, 2, 2), (64, 3000, 1, 2)])
def test_edge_gather_max_cloud_resident_is_bit_identical(cuda, C, N, B, act):
    """lpd_edge_gather_max16 (LDS-resident cloud slice, uint16 indices) == lpd_edge_gather_max, bit for bit; ragged N,
    point counts that are not multiples of 32 or 512, output into a column slice, and the no-centre-term form."""
    ops = _ops()
    k = 20
    P, Q, idx, scale, shift = _edge_inputs(B, N, C, k, C + N)
    PQ = torch.cat([P, Q], dim=1).to(cuda)
    idx = idx.to(cuda)
    idx16 = ops.pack_idx16(idx)
    for q in (PQ[:, C:], None):
        want = ops.edge_gather_max(PQ[:, :C], q, idx, N, scale=scale.to(cuda), shift=shift.to(cuda), act=act, slope=0.01)
        buf = torch.full((B * N, C + 8), -7.0, device=cuda)
        ops.edge_gather_max16(PQ[:, :C], q, idx16, N, scale=scale.to(cuda), shift=shift.to(cuda), act=act, slope=0.01, out=buf[:, 4:4 + C])
        assert torch.equal(buf[:, 4:4 + C], want)
        assert (buf[:, :4] == -7.0).all() and (buf[:, 4 + C:] == -7.0).all()
    plain = ops.edge_gather_max16(PQ[:, :C], None, idx16, N)
    assert torch.equal(plain, _gather(P, idx.cpu(), B, N).max(dim=1)[0].to(cuda))
    with pytest.raises(ops._lib.LpdHipError):
        ops.edge_gather_max16(PQ[:, :C], None, idx16, N, act=ops.ACT_SIGMOID)


@pytest.mark.parametrize("N,layout", [(4096, "panels"), (4000, "rows"), (3600, "panels")])
def test_kagg_persistent_workgroups(cuda, N, layout):
    """Enough (cloud, slice) items for the persistent form (>= 3 per CU: 24 clouds x 32 slices) on 8-pass clouds, ragged last
    pass included: bit-identical to the direct gather kernel; P/Q/out as cloud panels or row-major."""
    ops = _ops()
    B, C, k = 24, 256, 20
    g = torch.Generator().manual_seed(N)
    idx = torch.randint(0, N, (B * N, k), generator=g, dtype=torch.int32).to(cuda)
    P = torch.randn(B * N, C, generator=g).to(cuda)
    Q = torch.randn(B * N, C, generator=g).to(cuda)
    scale, shift = (torch.rand(C, generator=g) - 0.3).to(cuda), torch.randn(C, generator=g).to(cuda)
    want = ops.edge_gather_max(P, Q, idx, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01)
    i16 = ops.pack_idx16(idx)
    if layout == "panels":
        pq = ops.panels_empty(B, N, 2 * C, cuda)
        pq[:, :C // 8] = ops.rows_to_panels(P, B)
        pq[:, C // 8:] = ops.rows_to_panels(Q, B)
        out = ops.panels_empty(B, N, C, cuda)
        ops.edge_gather_max16(pq[:, :C // 8], pq[:, C // 8:], i16, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01, out=out)
        assert torch.equal(ops.panels_to_rows(out), want)
    else:
        out = torch.empty(B * N, C, device=cuda)
        ops.edge_gather_max16(P, Q, i16, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01, out=out)
        assert torch.equal(out, want)


@pytest.mark.parametrize("CM,CO,N,k,B,useQ", [(128, 128, 256, 20, 2, True), (64, 64, 200, 20, 2, True), (64, 64, 128, 20, 1, False),
                                               (128, 128, 100, 7, 1, True), (128, 128, 192, 64, 1, True), (64, 64, 130, 64, 2, False)])
@pytest.mark.parametrize("exact", [True, False], ids=["f32mfma", "bf16x3"])
def test_edge_mlp(cuda, CM, CO, N, k, B, useQ, exact):
    ops = _ops()
    P, Q, idx, s1, b1 = _edge_inputs(B, N, CM, k, CM + N + k)
    g = torch.Generator().manual_seed(3)
    W2 = torch.randn(CO, CM, generator=g) / (CM ** 0.5)
    s2, b2 = torch.randn(CO, generator=g), torch.randn(CO, generator=g)
    y1 = s1.double() * (_gather(P, idx, B, N).double() + (Q.double().unsqueeze(1) if useQ else 0)) + b1.double()
    y1 = torch.where(y1 > 0, y1, y1 * 0.01)                       # [M,k,CM]
    z = torch.matmul(y1, W2.double().t()) * s2.double() + b2.double()
    z = torch.where(z > 0, z, z * 0.01)
    ref = z.max(dim=1)[0]
    out = ops.edge_mlp(P.to(cuda), Q.to(cuda) if useQ else None, idx.to(cuda), N, s1.to(cuda), b1.to(cuda), W2.to(cuda),
                       s2.to(cuda), b2.to(cuda), exact=exact)
    assert _rel(out, ref) < (2e-5 if exact else 4e-5)


# ------------------------------------------------------------------ misc
def test_linear_smallk_transpose_softmax_colmax_mul(cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1000, 3, generator=g)
    w = torch.randn(64, 3, generator=g)
    bias, sc, sh = torch.randn(64, generator=g), torch.randn(64, generator=g), torch.randn(64, generator=g)
    ref = torch.clamp((x.double() @ w.double().t() + bias.double()) * sc.double() + sh.double(), min=0)
    out = ops.linear(x.to(cuda), w.to(cuda), bias=bias.to(cuda), scale=sc.to(cuda), shift=sh.to(cuda), act=ops.ACT_RELU)
    assert _rel(out, ref) < 1e-6
    t = torch.randn(3, 100, 70, generator=g)
    assert torch.equal(ops.transpose(t.to(cuda)).cpu(), t.transpose(1, 2).contiguous())
    a = torch.randn(777, 64, generator=g) * 3
    sm = ops.softmax_affine(a.to(cuda), sc.to(cuda), sh.to(cuda))
    sm64 = torch.softmax(a.double() * sc.double() + sh.double(), dim=-1)
    assert _rel(sm, sm64) < 1e-6
    # every element against its own value (the softmax of 64 logits of spread 3 x 1.5 stays far above the smallest normal float): four
    # times what float32 torch gives from the same inputs, and every row sums to 1
    floor = max(_elem(torch.softmax(a * sc + sh, dim=-1), sm64), 2.0 ** -23)
    assert _elem(sm, sm64) <= 4 * floor and (sm.double().sum(1) - 1).abs().max().item() <= 4 * floor
    cm = ops.colmax(t.reshape(300, 70).to(cuda), 3, 100)
    assert torch.equal(cm.cpu(), t.max(dim=1)[0])
    assert torch.equal(ops.mul(a.to(cuda), a.to(cuda)).cpu(), a * a)


def test_vlad_finalize(cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(2)
    B, N, F, K = 3, 200, 128, 64
    vraw = torch.randn(B, F, K, generator=g)
    act = torch.softmax(torch.randn(B, N, K, generator=g), dim=-1)
    cw2 = torch.randn(F, K, generator=g)
    v = vraw.double() - act.double().sum(dim=1, keepdim=True) * cw2.double()
    v = v / v.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    v = v.reshape(B, F * K)
    v = v / v.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    out = ops.vlad_finalize(vraw.to(cuda), act.to(cuda), cw2.to(cuda))
    assert _rel(out, v) < 1e-5
    # element-wise, each against its value plus the terms of its residual under the two normalisations (1e-5 of THAT, not of max |v|)
    r = vraw.double() - act.double().sum(dim=1, keepdim=True) * cw2.double()
    terms = (vraw.double().abs() + (act.double().sum(dim=1, keepdim=True) * cw2.double()).abs()) * (v.reshape(B, F, K) / r).abs()
    assert _elem(out, v, v.abs() + terms.reshape(B, F * K)) < 1e-5


@pytest.mark.parametrize("ncols", [64, 40])
def test_softmax_with_cluster_sums_feeds_vlad_finalize(cuda, ncols):
    """softmax_affine(colsum_rows=N) = softmax_affine + the per-cloud column sums (a_sum); vlad_finalize(ws=...) on them
    matches the two-pass form."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    B, N, F = 3, 208, 96
    a = (torch.randn(B * N, ncols, generator=g) * 3).to(cuda)
    sc, sh = torch.randn(ncols, generator=g).to(cuda), torch.randn(ncols, generator=g).to(cuda)
    plain = ops.softmax_affine(a, sc, sh)
    fused, ws = ops.softmax_affine(a, sc, sh, colsum_rows=N)
    assert _rel(fused, plain) < 1e-6      # (the 64-column kernel sums a row in a different order)
    # element-wise, both forms against fp64: four times what float32 torch gives from the same inputs
    sm64 = torch.softmax(a.double().cpu() * sc.double().cpu() + sh.double().cpu(), dim=-1)
    floor = max(_elem(torch.softmax(a.cpu() * sc.cpu() + sh.cpu(), dim=-1), sm64), 2.0 ** -23)
    assert _elem(fused, sm64) <= 4 * floor and _elem(plain, sm64) <= 4 * floor
    assert ws.shape == (B, 2 * ncols) and ws[:, ncols:].abs().max().item() == 0
    assert _rel(ws[:, :ncols], plain.double().view(B, N, ncols).sum(1)) < 1e-6
    # every column sum against the fp64 sum of its own (positive) terms: N 2^-24 bounds a float32 sum of N positive terms in any order
    assert _elem(ws[:, :ncols], fused.double().view(B, N, ncols).sum(1)) <= N * 2.0 ** -24
    with pytest.raises(ValueError):
        ops.softmax_affine(a, sc, sh, colsum_rows=N - 8)
    if ncols == 64:
        vraw = torch.randn(B, F, 64, generator=g).to(cuda)
        cw2 = torch.randn(F, 64, generator=g).to(cuda)
        two_pass = ops.vlad_finalize(vraw, plain.view(B, N, 64), cw2)
        one_pass = ops.vlad_finalize(vraw, plain.view(B, N, 64), cw2, ws=ws)
        assert _rel(one_pass, two_pass) < 1e-6
        assert _elem(one_pass, two_pass, two_pass.abs() + two_pass.abs().mean()) < 1e-5   # element-wise; small elements against the mean magnitude (cancellation in vraw - a_sum cw2)


@pytest.mark.parametrize("B,D,mode", [(32, 256, "bn"), (5, 200, "bias"), (1, 24, "plain")])
def test_gating_context(cuda, B, D, mode):
    """h * sigmoid(affine(h @ Wg)) in one launch (util/PointNetVlad.py:103-115) against fp64."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + D)
    h = torch.randn(B, D + 4, generator=g)[:, :D]
    Wg = torch.randn(D, D, generator=g) / D ** 0.5
    bias, sc, sh = torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    z = h.double() @ Wg.double()
    kw = {}
    if mode == "bn":
        z = z * sc.double() + sh.double(); kw = dict(scale=sc.to(cuda), shift=sh.to(cuda))
    elif mode == "bias":
        z = z + bias.double(); kw = dict(bias=bias.to(cuda))
    ref = h.double() * torch.sigmoid(z)
    hd = torch.zeros(B, D + 4, device=cuda); hd[:, :D] = h.to(cuda)
    out = ops.gating(hd[:, :D], Wg.to(cuda), **kw)
    assert _rel(out, ref) < 2e-6


def test_errors_are_loud(cuda):
    from lpdnet_hip import LpdHipError
    ops = _ops()
    with pytest.raises(LpdHipError):
        ops.knn(torch.zeros(1, 3, 64), 4)                    # CPU tensor: no fallback
    with pytest.raises(LpdHipError):
        ops.knn(torch.zeros(1, 3, 8, device=cuda), 9)        # k > N
    with pytest.raises(LpdHipError):
        ops.gemm(torch.zeros(4, 50, device=cuda), torch.zeros(50, 8, device=cuda))  # leading dim not a multiple of 4


@pytest.mark.parametrize("C,N,B,k", [(256, 512, 2, 20), (128, 1000, 3, 20), (64, 96, 2, 7)])
def test_gather_sum_rows_is_the_transpose_of_the_neighbour_gather(cuda, C, N, B, k):
    """CSR transposed graph + gather-sum == the atomic scatter (lpd_scatter_add_rows) == a dense reference, including rows
    nobody points to (must come out zero) and accumulation into a column slice."""
    ops = _ops()
    g = torch.Generator().manual_seed(C + N)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(N)]) for _ in range(B)]).to(torch.int32)
    idx[:, :, 0] = idx[:, :1, 0]                       # a hub: every point of a cloud lists the same first neighbour
    M = B * N
    dU = torch.randn(M * k, C, generator=g)
    ref = torch.zeros(M, C, dtype=torch.float64)
    rows = (idx.long() + (torch.arange(B) * N).view(B, 1, 1)).reshape(-1)
    ref.index_add_(0, rows, dU.double())
    graph = ops.GraphT(idx.to(cuda), N)
    assert int(graph.rowptr[-1]) == M * k and int(graph.rowptr[0]) == 0
    e = graph.edges.cpu().long()
    assert torch.equal(torch.sort(e)[0], torch.arange(M * k))                       # a permutation of the edge ids
    buf = torch.full((M, C + 8), 3.0, device=cuda)
    ops.gather_sum_rows(dU.to(cuda), graph, buf[:, 4:4 + C])
    assert _rel(buf[:, 4:4 + C], ref) < 3e-6   # fp32 sums in edge-arrival order (the CSR fill uses int atomics)
    assert (buf[:, :4] == 3.0).all() and (buf[:, 4 + C:] == 3.0).all()
    ops.gather_sum_rows(dU.to(cuda), graph, buf[:, 4:4 + C], accumulate=True)
    assert _rel(buf[:, 4:4 + C], 2 * ref) < 3e-6
    old = ops.scatter_add_rows(dU.to(cuda), idx.to(cuda), torch.zeros(M, C, device=cuda), N)
    assert _rel(old, ref) < 3e-6


@pytest.mark.parametrize("M,N,K,bk", [(4096, 512, 1024, True), (2048, 256, 128, True), (1500, 64, 1024, True), (3000, 200, 136, True),
                                       (1024, 72, 148, True), (4096, 1024, 512, False), (2100, 300, 264, False), (1111, 136, 300, False),
                                       (2050, 64, 288, True), (1300, 64, 520, False)])
def test_gemm_weight_fragment_path(cuda, M, N, K, bk):
    """Row-major activations times a weight matrix take lpd_gemm_x3w (B fragments prepared once, never staged in LDS):
    same contract and error bound as the generic split-bf16 kernel; epilogue, output slice, accumulation, ragged N / K."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K + 4, generator=g)[:, :K]
    W = torch.nn.Parameter(torch.randn((K, N) if bk else (N, K), generator=g).to(cuda) / K ** 0.5)
    bias, scale, shift = torch.randn(N, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)
    Wl = (W.detach().cpu() if bk else W.detach().cpu().t()).double()
    ref = (A.double() @ Wl + bias.double()) * scale.double() + shift.double()
    ref = torch.where(ref > 0, ref, ref * 0.01)
    Ad = torch.zeros(M, K + 4, device=cuda)
    Ad[:, :K] = A.to(cuda)
    prof = ops.PROFILE = {}
    try:
        buf = torch.zeros(M, N + 8, device=cuda)
        with torch.no_grad():
            ops.gemm(Ad[:, :K], W, b_kmajor=bk, bias=bias.to(cuda), scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY,
                     out=buf[:, 4:4 + N])
            assert _rel(buf[:, 4:4 + N], ref) < 3e-5
            assert buf[:, :4].abs().max().item() == 0 and buf[:, 4 + N:].abs().max().item() == 0
            raw = ops.gemm(Ad[:, :K], W, b_kmajor=bk)
            ops.gemm(Ad[:, :K], W, b_kmajor=bk, out=raw, accumulate=True)
            assert _rel(raw, 2 * (A.double() @ Wl)) < 3e-5
            W.mul_(2.0)                                         # an in-place parameter update (optimizer step, load_state_dict) bumps
                                                                # _version and so invalidates the cached fragments
            raw2 = ops.gemm(Ad[:, :K], W, b_kmajor=bk)
            assert _rel(raw2, 2 * (A.double() @ Wl)) < 3e-5
    finally:
        ops.PROFILE = None
    assert any(k.startswith("gemmx3w") for k in prof), list(prof)


@pytest.mark.parametrize("B,N,k,act", [(3, 1024, 20, 2), (2, 4096, 20, 1), (1, 5120, 20, 2), (2, 256, 64, 0)])
def test_lpdnet_front_fused(cuda, B, N, k, act):
    """lpd_lpdnet_front (conv1 -> conv2 + the kNN operands of their output in one launch) against the separate exact-fp32 layers:
    F0 to fp32 rounding (the summation order of conv2 differs), and the graph lpd_knn_pm builds from the prepared operands is
    EXACTLY the graph of the fused kernel's own F0 (prepared and unprepared entries agree bit for bit)."""
    ops = _ops()
    g = torch.Generator().manual_seed(5 + N)
    xyz = (torch.rand(B * N, 3, generator=g) * 2 - 1).to(cuda)
    W1 = torch.randn(64, 3, generator=g).to(cuda)
    W2 = (torch.randn(64, 64, generator=g) / 8).to(cuda)
    s1, b1, s2, b2 = (torch.randn(64, generator=g).to(cuda) for _ in range(4))
    f0, ws = ops.lpdnet_front(xyz, W1, s1, b1, W2, s2, b2, B, N, k, act=act, slope=0.2)
    with ops.exact_gemm():
        f1 = ops.linear(xyz, W1, scale=s1, shift=b1, act=act, slope=0.2)
        ref = ops.linear(f1, W2, scale=s2, shift=b2, act=act, slope=0.2)
    want = xyz.double() @ W1.double().t() * s1.double() + b1.double()
    want = want if act == 0 else torch.where(want > 0, want, want * (0.0 if act == 1 else 0.2))
    want = want @ W2.double().t() * s2.double() + b2.double()
    want = want if act == 0 else torch.where(want > 0, want, want * (0.0 if act == 1 else 0.2))
    assert _rel(f0, want) < 2e-6 and _rel(ref, want) < 2e-6
    idx_prepared = ops.knn_prepared(ws, B, N, k)
    idx_plain = ops.knn_pm(f0, B, N, k)
    assert torch.equal(idx_prepared, idx_plain)
    oidx, _ = orc.knn_np(f0.view(B, N, 64).cpu().numpy(), k)
    rows_ok = (idx_prepared.cpu().numpy() == oidx).all(-1)
    ties = orc.knn_tie_rows(f0.view(B, N, 64).cpu().numpy(), k)
    assert rows_ok[~ties].all()


@pytest.mark.parametrize("K,N,act", [(128, 512, 2), (64, 128, 1), (128, 160, 0)])
def test_gemm_x3t_panels(cuda, K, N, act):
    """lpd_gemm_x3t (short reduction, cloud panels in and out, computed transposed: the SN1 projection): fp32-grade against a
    float64 product, every epilogue term, A and C as panel sub-ranges of wider buffers, untouched neighbours; exact mode and
    LPD_DEBUG=x3t=0 keep the generic kernels."""
    ops = _ops()
    g = torch.Generator().manual_seed(41 + K + N)
    Bc, Np = 5, 384
    M = Bc * Np
    X = torch.randn(M, K, generator=g).to(cuda) * 3.0
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    bi, sc, sh = (torch.randn(N, generator=g).to(cuda) for _ in range(3))
    ref = ((X.double() @ W.double().t()) + bi.double()) * sc.double() + sh.double()
    ref = ref if act == 0 else torch.where(ref > 0, ref, ref * (0.0 if act == 1 else 0.2))
    big = ops.panels_empty(Bc, Np, K + 64, cuda)
    big.fill_(float("nan"))
    big[:, 8:8 + K // 8] = ops.rows_to_panels(X, Bc)
    wide = ops.panels_empty(Bc, Np, N + 128, cuda)
    wide.fill_(-7.0)
    prof = ops.PROFILE = {}
    try:
        ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, bias=bi, scale=sc, shift=sh, act=act, slope=0.2, a_panels=True,
                 out=wide[:, 8:8 + N // 8], out_panels=True)
        plain = ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, a_panels=True, out_panels=True)
    finally:
        ops.PROFILE = None
    assert sum(k.startswith("gemmx3t") for k in prof) == 1 and len(prof[f"gemmx3t[{M}x{N}x{K}]"]) == 2, list(prof)
    assert _rel(ops.panels_to_rows(wide[:, 8:8 + N // 8]), ref) < 2e-5
    assert _rel(ops.panels_to_rows(plain), X.double() @ W.double().t()) < 2e-5
    assert bool((wide[:, :8] == -7.0).all()) and bool((wide[:, 8 + N // 8:] == -7.0).all())
    # the same call on the generic kernels (switch off / exact mode): same values to rounding
    ops.X3T_PANELS = False
    try:
        gen = ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, a_panels=True, out_panels=True)
    finally:
        ops.X3T_PANELS = True
    assert _rel(ops.panels_to_rows(plain), ops.panels_to_rows(gen).double()) < 2e-5
    prof = ops.PROFILE = {}
    try:
        ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, a_panels=True, out_panels=True, exact=True)
    finally:
        ops.PROFILE = None
    assert not any(k.startswith("gemmx3t") for k in prof), list(prof)


@pytest.mark.parametrize("exact", [True, False], ids=["f32mfma", "bf16x3"])
def test_cloud_panel_operands(cuda, exact):
    """Cloud-panel buffers [B, C/8, N, 8] through GEMM (A and C, also as panel sub-ranges of wider buffers), the fused edge
    MLP (out) and the cloud-resident K-agg (P, Q, out in every combination): bit-identical to the row-major results (only
    the addressing changes)."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    Bc, Np, K, N = 3, 512, 128, 512
    M = Bc * Np
    X = torch.randn(M, K, generator=g).to(cuda)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    sc, sh = torch.randn(N, generator=g).to(cuda), torch.randn(N, generator=g).to(cuda)
    want = ops.gemm(X, W, b_kmajor=False, scale=sc, shift=sh, act=ops.ACT_LEAKY, exact=exact)
    big = ops.panels_empty(Bc, Np, K + 64, cuda)              # A as a panel sub-range of a wider buffer
    big[:, 8:8 + K // 8] = ops.rows_to_panels(X, Bc)
    ops.X3T_PANELS = False      # (the transposed short-reduction kernel sums in another order: test_gemm_x3t_panels)
    try:
        got = ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, scale=sc, shift=sh, act=ops.ACT_LEAKY, exact=exact, a_panels=True, out_panels=True)
    finally:
        ops.X3T_PANELS = True
    assert got.shape == (Bc, N // 8, Np, 8)
    assert torch.equal(ops.panels_to_rows(got), want)
    wide = ops.panels_empty(Bc, Np, N + 128, cuda)
    ops.gemm(X, W, b_kmajor=False, scale=sc, shift=sh, act=ops.ACT_LEAKY, exact=exact, out=wide[:, 16:], out_panels=True)
    assert torch.equal(ops.panels_to_rows(wide[:, 16:]), want)
    rowm = ops.gemm(big[:, 8:8 + K // 8], W, b_kmajor=False, scale=sc, shift=sh, act=ops.ACT_LEAKY, exact=exact, a_panels=True)
    assert torch.equal(rowm, want)
    # deep reduction (K >= 256): the prepared-fragment kernel, both block shapes, ragged column blocks (N = 320)
    K2, N2 = 512, 320
    X2 = torch.randn(M, K2, generator=g).to(cuda)
    Wd = (torch.randn(N2, K2, generator=g) / K2 ** 0.5).to(cuda)
    sc2, sh2 = torch.randn(N2, generator=g).to(cuda), torch.randn(N2, generator=g).to(cuda)
    xp = ops.rows_to_panels(X2, Bc)
    ref2 = (X2.double() @ Wd.double().t()) * sc2.double() + sh2.double()
    ref2 = torch.where(ref2 > 0, ref2, ref2 * 0.01)
    for impl in (0, 2, 3):
        ops.X3W_IMPL = impl
        prof = ops.PROFILE = {}
        try:
            want2 = ops.gemm(X2, Wd, b_kmajor=False, scale=sc2, shift=sh2, act=ops.ACT_LEAKY, exact=exact)
            assert _rel(want2, ref2) < (2e-6 if exact else 3e-5)
            got2 = ops.gemm(xp, Wd, b_kmajor=False, scale=sc2, shift=sh2, act=ops.ACT_LEAKY, exact=exact, a_panels=True, out_panels=True)
            assert torch.equal(ops.panels_to_rows(got2), want2), impl
            assert torch.equal(ops.gemm(xp, Wd, b_kmajor=False, scale=sc2, shift=sh2, act=ops.ACT_LEAKY, exact=exact, a_panels=True), want2), impl
            acc2 = ops.gemm(X2, Wd, b_kmajor=False, exact=exact, out=got2.clone(), out_panels=True, accumulate=True)
            assert _rel(ops.panels_to_rows(acc2), ref2 + X2.double() @ Wd.double().t()) < (2e-6 if exact else 3e-5), impl
        finally:
            ops.X3W_IMPL, ops.PROFILE = 0, None
        assert exact or any(k.startswith("gemmx3w") for k in prof), list(prof)
    # K-agg: every combination of cloud-panel / row-major P, Q, out
    B_, Nq, C, k = 2, 768, 256, 20
    P, Q, idx, scale, shift = _edge_inputs(B_, Nq, C, k, 5)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    ref = ops.edge_gather_max(P, Q, idx, Nq, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY)
    i16 = ops.pack_idx16(idx)
    pqbuf = ops.panels_empty(B_, Nq, 2 * C, cuda)             # P and Q as the two panel halves of one buffer (like the pipeline)
    pqbuf[:, :C // 8] = ops.rows_to_panels(P, B_)
    pqbuf[:, C // 8:] = ops.rows_to_panels(Q, B_)
    for lay in range(8):
        p_ = pqbuf[:, :C // 8] if lay & 1 else P
        q_ = pqbuf[:, C // 8:] if lay & 2 else Q
        o_ = ops.panels_empty(B_, Nq, C, cuda) if lay & 4 else torch.empty(B_ * Nq, C, device=cuda)
        ops.edge_gather_max16(p_, q_, i16, Nq, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY, out=o_)
        assert torch.equal(ops.panels_to_rows(o_) if lay & 4 else o_, ref), lay
    # edge MLP into a panel sub-range
    P2, Q2, idx2, s1, b1 = _edge_inputs(2, 256, 128, 20, 9)
    W2 = (torch.randn(128, 128, generator=g) / 11).to(cuda)
    s2, b2 = torch.randn(128, generator=g).to(cuda), torch.randn(128, generator=g).to(cuda)
    args = (P2.to(cuda), Q2.to(cuda), idx2.to(cuda), 256, s1.to(cuda), b1.to(cuda), W2, s2, b2)
    rowm = ops.edge_mlp(*args, exact=exact)
    pan = ops.panels_empty(2, 256, 512, cuda)
    ops.edge_mlp(*args, exact=exact, out=pan[:, 16:32])
    assert torch.equal(ops.panels_to_rows(pan[:, 16:32]), rowm)


# ------------------------------------------------------------------ training path, second generation
def _bn_for(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C)
    bn.weight.data.copy_(torch.rand(C, generator=g) - 0.3)      # ~30 % negative scales: the min-selection path
    bn.bias.data.copy_(torch.randn(C, generator=g) * 0.1)
    return bn


@pytest.mark.parametrize("C,N,k,B", [(256, 512, 20, 2), (128, 300, 20, 3), (64, 128, 7, 2), (256, 256, 64, 1), (256, 4096, 20, 2), (64, 1000, 20, 1),
                                     # launches of fewer than 8 blocks in the backward gather (lpd_xcd_sweep): M <= 56 / 112 / 224 rows at C = 256 / 128 / 64
                                     (256, 32, 7, 1), (256, 24, 5, 2), (128, 64, 7, 1), (128, 36, 20, 3), (64, 32, 5, 2), (64, 200, 20, 1)])
def test_split_form_edge_stage_equals_the_materialised_one(cuda, C, N, k, B):
    """lpd_edge_split_fwd / _bwd (no [M*k, C] edge tensor; closed-form BatchNorm sums, one pass over the transposed graph)
    against the materialised formulation edge_build -> group_max -> edge_bn_bwd -> gather_sum_rows: outputs, arg-max,
    batch statistics, running statistics, dP, dQ, dgamma, dbeta."""
    ops = _ops()
    M = B * N
    P, Q, idx, _, _ = _edge_inputs(B, N, C, k, 5 * C + N + k)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    g = torch.Generator().manual_seed(C + k)
    dOut = torch.randn(M, C + 8, generator=g).to(cuda)[:, 4:4 + C]        # a strided view, like dcat[:, 256:512]
    act, slope = ops.ACT_LEAKY, 0.01
    bn_a, bn_b = _bn_for(C, 3).to(cuda).train(), _bn_for(C, 3).to(cuda).train()
    # materialised reference (validated against the oracle by the training tests)
    U, st_a = ops.edge_build(P, Q, idx, N, bn=bn_a)
    out_a = torch.empty(M, C, device=cuda)
    arg_a = ops.group_max(U, k, st_a.scale, st_a.shift, act, slope, out_a)
    dQ_a = torch.empty(M, C, device=cuda)
    dU, dg_a, db_a = ops.edge_bn_bwd(dOut, arg_a, k, U, st_a, act, slope, dQ=dQ_a)
    dP_a = torch.empty(M, C, device=cuda)
    ops.gather_sum_rows(dU, ops.GraphT(idx, N), dP_a)
    # split form (k = 20, N <= 4096: on cloud-resident slices; the wave-per-point kernel must give the same S / usel / arg bit for bit)
    S, usel, arg_b, st_b = ops.edge_split_fwd(P, Q, idx, N, bn_b)
    if k == 20:
        import ctypes
        from lpdnet_hip import _lib
        lib = _lib.load()
        assert lib.lpd_edge_split_fwd16_applies(N, C, k)
        S0, u0, a0 = torch.empty_like(S), torch.empty_like(usel), torch.empty_like(arg_b)
        sums0 = torch.empty(2, C, dtype=torch.float64, device=cuda)
        idc = idx.reshape(-1, k).contiguous()
        rc = lib.lpd_edge_split_fwd(P.data_ptr(), P.stride(0), Q.data_ptr(), Q.stride(0), idc.data_ptr(), bn_b.weight.data_ptr(), S0.data_ptr(),
                                    u0.data_ptr(), a0.data_ptr(), M, N, C, k, sums0[0].data_ptr(), sums0[1].data_ptr(), ops._stat_ws(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert torch.equal(S0, S) and torch.equal(u0, usel) and torch.equal(a0, arg_b)
    out_b = ops.affine_act(usel, st_b.scale, st_b.shift, act, slope)
    buf = torch.zeros(M, 2 * C + 8, device=cuda)
    dg_b, db_b = ops.edge_split_bwd(dOut, usel, arg_b, S, P, Q, ops.GraphT(idx, N), st_b, act, slope, k, dP=buf[:, 4:4 + C],
                                    dQ=buf[:, 4 + C:4 + 2 * C])
    assert torch.equal(arg_a, arg_b)
    for a, b in ((st_a.mean, st_b.mean), (st_a.invstd, st_b.invstd), (st_a.scale, st_b.scale), (st_a.shift, st_b.shift)):
        assert _rel(b, a) < 1e-5
    assert _rel(bn_b.running_mean, bn_a.running_mean) < 1e-5 and _rel(bn_b.running_var, bn_a.running_var) < 1e-5
    assert int(bn_b.num_batches_tracked) == 1
    assert _rel(out_b, out_a) < 1e-5
    assert _rel(buf[:, 4:4 + C], dP_a) < 2e-5 and _rel(buf[:, 4 + C:4 + 2 * C], dQ_a) < 2e-5
    assert _rel(dg_b, dg_a) < 1e-5 and _rel(db_b, db_a) < 1e-5
    assert (buf[:, :4] == 0).all() and (buf[:, 4 + 2 * C:] == 0).all()
    if C == 256:      # bf16 storage: the gathered rows (G, Q) are bf16 copies -- the statistics stay exact, dP / dQ carry one rounding per term
        buf16 = torch.zeros_like(buf)
        dg_h, db_h = ops.edge_split_bwd(dOut, usel, arg_b, S, P, Q, ops.GraphT(idx, N), st_b, act, slope, k, dP=buf16[:, 4:4 + C],
                                        dQ=buf16[:, 4 + C:4 + 2 * C], half=True)
        assert torch.equal(dg_h, dg_b) and torch.equal(db_h, db_b)
        assert _rel(buf16[:, 4:4 + C], dP_a) < 6e-3 and _rel(buf16[:, 4 + C:4 + 2 * C], dQ_a) < 6e-3
        assert not torch.equal(buf16, buf)
        out16 = torch.zeros(M, 2 * C + 16, dtype=torch.bfloat16, device=cuda)      # ... and dP / dQ themselves as bf16 rows (half & 2)
        dg_o, db_o = ops.edge_split_bwd(dOut, usel, arg_b, S, P, Q, ops.GraphT(idx, N), st_b, act, slope, k, dP=out16[:, 8:8 + C],
                                        dQ=out16[:, 8 + C:8 + 2 * C], half=True)
        assert torch.equal(dg_o, dg_b) and torch.equal(out16[:, 8:8 + 2 * C], buf16[:, 4:4 + 2 * C].to(torch.bfloat16))
        assert (out16[:, :8] == 0).all() and (out16[:, 8 + 2 * C:] == 0).all()


def test_bf16_storage_edge_kernels(cuda):
    """The bf16-storage kernels of the DG1 -> DG2 chain against their fp32 counterparts evaluated on the same (rounded) values:
    statistics, selections and gradients must agree to fp32 accuracy -- only the STORED tensors are bf16."""
    ops = _ops()
    C, N, k, B = 128, 320, 20, 2
    M = B * N
    P, Q, idx, _, _ = _edge_inputs(B, N, C, k, 77)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    act, slope = ops.ACT_LEAKY, 0.01
    bn_a, bn_b = _bn_for(C, 5).to(cuda).train(), _bn_for(C, 5).to(cuda).train()
    U16, st16 = ops.edge_build_bf16(P, Q, idx, N, bn_a)
    U32 = ops.edge_build(P, Q, idx, N)
    assert U16.dtype == torch.bfloat16 and torch.equal(U16, U32.to(torch.bfloat16))          # round to nearest even
    Ur = U16.float()
    st32 = ops.bn_train_stats(Ur, bn_b)
    assert _rel(st16.mean, st32.mean) < 1e-5 and _rel(st16.invstd, st32.invstd) < 1e-5
    # Y = act(BN(U)) + max over k in one pass
    out16 = torch.empty(M, C, device=cuda)
    Y16, arg16 = ops.edge_act_max_bf16(U16, k, st32, act, slope, out16)
    out32 = torch.empty(M, C, device=cuda)
    arg32 = ops.group_max(Ur, k, st32.scale, st32.shift, act, slope, out32)
    Y32 = ops.affine_act(Ur, st32.scale, st32.shift, act, slope)
    assert torch.equal(arg16, arg32) and _rel(out16, out32) < 1e-6 and torch.equal(Y16, Y32.to(torch.bfloat16))
    # z = Y W^T on the bf16 MFMA (weight split hi + lo), dY = dZ W, dW = dZ^T Y
    g = torch.Generator().manual_seed(9)
    W = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    Z16 = ops.gemm_bf16s(Y16, W)
    Zref = Y16.double() @ W.double().t()
    assert _rel(Z16.double(), Zref) < 6e-3                       # bf16 rounding of the stored result (2^-9 relative)
    assert _rel(Z16, Zref.float().to(torch.bfloat16)) < 8e-3
    dY16 = ops.gemm_bf16s(Z16, W, b_kmajor=True)
    assert _rel(dY16.double(), Z16.double() @ W.double()) < 6e-3
    dW = ops.gemm_tn_bf16(Z16, Y16)
    assert _rel(dW, Z16.double().t() @ Y16.double()) < 1e-5      # fp32 accumulation of exact bf16 products
    # statistics + raw selection of Z in one pass
    bn_z1, bn_z2 = _bn_for(C, 6).to(cuda).train(), _bn_for(C, 6).to(cuda).train()
    sel, argz, stz = ops.group_sel_stats_bf16(Z16, k, bn_z1)
    stz32 = ops.bn_train_stats(Z16.float(), bn_z2)
    assert _rel(stz.mean, stz32.mean) < 1e-5 and _rel(stz.invstd, stz32.invstd) < 1e-5
    x2a = ops.affine_act(sel, stz.scale, stz.shift, act, slope)
    x2b = torch.empty(M, C, device=cuda)
    argzb = ops.group_max(Z16.float(), k, stz32.scale, stz32.shift, act, slope, x2b)
    assert torch.equal(argz, argzb) and _rel(x2a, x2b) < 1e-5
    # backward through max + act + BN on bf16 tensors
    dOut = torch.randn(M, C, generator=g).to(cuda)
    dense = torch.randn(M * k, C, generator=g).to(cuda).to(torch.bfloat16)
    dQ16 = torch.empty(M, C, device=cuda)
    dX16, dg16, db16 = ops.edge_bn_bwd_bf16(dOut, arg16, k, U16, st32, act, slope, dense=dense.clone(), dQ=dQ16)
    dQ32 = torch.empty(M, C, device=cuda)
    dX32, dg32, db32 = ops.edge_bn_bwd(dOut, arg16, k, Ur, st32, act, slope, dense=dense.float(), dQ=dQ32)
    assert _rel(dg16, dg32) < 1e-5 and _rel(db16, db32) < 1e-5 and _rel(dQ16, dQ32) < 1e-5
    assert torch.equal(dX16, dX32.to(torch.bfloat16))
    dX16b, dg16b, db16b = ops.edge_bn_bwd_bf16(dOut, argz, k, Z16, stz, act, slope)            # sparse form (no dense gradient)
    dX32b, dg32b, db32b = ops.edge_bn_bwd(dOut, argz, k, Z16.float(), stz, act, slope)
    assert torch.equal(dX16b, dX32b.to(torch.bfloat16))
    # the same with the raw selected values the forward kept (no gather from the edge tensor): bit-identical
    dX16c, dg16c, db16c = ops.edge_bn_bwd_bf16(dOut, argz, k, Z16, stz, act, slope, xsel=sel)
    assert torch.equal(dX16c, dX16b) and torch.equal(dg16c, dg16b) and torch.equal(db16c, db16b)
    argzc, selc = ops.group_max(Z16.float(), k, stz.scale, stz.shift, act, slope, torch.empty(M, C, device=cuda), keep_sel=True)
    assert torch.equal(argzc, argz) and torch.equal(selc, sel)
    dX32c, dg32c, db32c = ops.edge_bn_bwd(dOut, argz, k, Z16.float(), stz, act, slope, xsel=selc)
    assert torch.equal(dX32c, dX32b) and torch.equal(dg32c, dg32b) and torch.equal(db32c, db32b)
    # DG2 backward without the dZ tensor (csrc/lpd_train3.hip): dW = dZ^T Y from one pass over Y (arg-max product + Gram matrix),
    # dY = dZ W with dZ generated in the operand loader -- against fp64 on the same stored tensors, and against the dZ path
    assert ops.dg2_bwd_fused_applies(M, k, C)
    dpre16, red = ops.bn_sel_bwd_reduce(dOut, sel, stz, act, slope)
    assert torch.equal(red[0].float(), db16b) and torch.equal(red[1].float(), dg16b)
    z64, y64 = Z16.double(), Y16.double()
    pre = stz.scale.double() * sel.double() + stz.shift.double()
    dpre = dOut.double() * torch.where(pre > 0, 1.0, slope)
    assert torch.equal(dpre16, dpre.float().to(torch.bfloat16))
    D = torch.zeros(M, k, C, dtype=torch.float64, device=cuda)
    D.scatter_(1, argz.long().view(M, 1, C), dpre16.double().view(M, 1, C))            # the kernels use the bf16 dpre
    m1, m2 = red[0] / (M * k), red[1] / (M * k)
    xhat = (z64 - stz.mean.double()) * stz.invstd.double()
    dZ = stz.scale.double() * (D.view(M * k, C) - m1 - xhat * m2)
    dW_new = ops.edge_dw_sel_bf16(Y16, argz, dpre16, k, W, stz, red)
    dW_old = ops.gemm_tn_bf16(dX16b, Y16)
    dW_ref = dZ.t() @ y64
    # the Gram form sums the UNROUNDED z = Y W^T where the dZ path holds z rounded to bf16 and dZ rounded to bf16
    dW_ref_u = (stz.scale.double() * (D.view(M * k, C) - m1 - ((y64 @ W.double().t()) - stz.mean.double()) * stz.invstd.double() * m2)).t() @ y64
    assert _rel(dW_new, dW_ref_u) < 2e-5, _rel(dW_new, dW_ref_u)
    assert _rel(dW_new, dW_ref) < 3e-4 and _rel(dW_old, dW_ref) < 8e-3, (_rel(dW_new, dW_ref), _rel(dW_old, dW_ref))   # measured 7e-5 / 3.9e-3
    dY_new = ops.gemm_bf16s_bnbwd(Z16, argz, dpre16, k, W, stz, red)
    dY_old = ops.gemm_bf16s(dX16b, W, b_kmajor=True)
    dY_ref = dZ @ W.double()
    assert _rel(dY_new.double(), dY_ref) < 6e-3 and _rel(dY_old.double(), dY_ref) < 8e-3, (_rel(dY_new.double(), dY_ref), _rel(dY_old.double(), dY_ref))
    gt = ops.GraphT(idx, N)
    a = torch.empty(M, C, device=cuda)
    b = torch.empty(M, C, device=cuda)
    ops.gather_sum_rows_bf16(dX16, gt, a)
    ops.gather_sum_rows(dX16.float(), gt, b)
    assert _rel(a, b) < 1e-6


def test_single_product_bf16_gemm_entry(cuda):
    """lpd_gemm_bf16x1 / lpd_gemm_x3w(impl | 16): operands rounded to bf16, fp32 accumulation -- equal to the product of the
    bf16-rounded operands to fp32 accuracy, and ~4e-3 from the fp32 product."""
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    A = torch.randn(512, 256, generator=g).to(cuda)
    W = (torch.randn(384, 256, generator=g) / 16).to(cuda)
    ref_r = A.to(torch.bfloat16).double() @ W.to(torch.bfloat16).double().t()
    ops._FAST.depth += 1
    try:
        out = ops.gemm(A, W, b_kmajor=False)                      # M >= 1024 not met: generic kernel
        out_w = ops.gemm(torch.cat([A, A]), W, b_kmajor=False)    # M = 1024, K = 256: prepared-fragment kernel
    finally:
        ops._FAST.depth -= 1
    assert _rel(out, ref_r) < 1e-5 and _rel(out_w[:512], ref_r) < 1e-5
    assert 1e-4 < _rel(out, A.double() @ W.double().t()) < 2e-2
    assert _rel(ops.gemm(A, W, b_kmajor=False), A.double() @ W.double().t()) < 2e-5      # outside the region: three products


@pytest.mark.parametrize("C,N,k,B,graph", [(256, 16384, 64, 1, "local"), (128, 5000, 20, 2, "local"), (256, 2048, 64, 2, "random"),
                                           (64, 9000, 32, 1, "random"), (256, 4100, 64, 1, "local")])
def test_windowed_kagg_is_bit_identical(cuda, C, N, k, B, graph):
    """lpd_edge_gather_maxw (Z-order window of 4095 rows in LDS, out-of-window neighbours from L2) == lpd_edge_gather_max, bit for
    bit: graphs whose neighbours are near in index (mostly LDS hits, misses at the window borders), uniformly random graphs
    (almost every gather of a multi-window cloud is a miss), ragged last windows, one-window clouds, output into a column
    slice, negative scales, the no-centre-term form."""
    ops = _ops()
    g = torch.Generator().manual_seed(N + k)
    M = B * N
    if graph == "local":
        off = torch.randint(-600, 601, (M, k), generator=g)
        base = torch.arange(N).repeat(B).view(M, 1)
        idx = (base + off).clamp_(0, N - 1).to(torch.int32)
        idx[:, 0] = base[:, 0]
    else:
        idx = torch.randint(0, N, (M, k), generator=g, dtype=torch.int32)
    idx = idx.to(cuda)
    PQ = torch.randn(M, 2 * C, generator=g).to(cuda)
    scale, shift = (torch.rand(C, generator=g) - 0.3).to(cuda), torch.randn(C, generator=g).to(cuda)
    i16_plain = ops.pack_idx16w(idx)
    i16 = ops.pack_idx16w(idx, N)          # out-of-window neighbours first (the product setting: N known)

    def unpack(t):                         # blocked [M32 / 32][k / 4][32 points][4] -> [M, k]
        M32 = t.shape[0]
        return t.view(M32 // 32, k // 4, 32, 4).permute(0, 2, 1, 3).reshape(M32, k)[:M].to(torch.int32) & 0xffff
    assert torch.equal(unpack(i16_plain), idx)
    # partitioned: the neighbours outside the point's window first, each part in its kNN order
    rows, ic = unpack(i16).cpu(), idx.cpu()
    w0 = (((torch.arange(M) % N) // 4095) * 4095).view(-1, 1)
    mo = ((ic - w0) < 0) | ((ic - w0) >= 4095)
    order = torch.argsort((~mo).to(torch.int8), dim=1, stable=True)
    assert torch.equal(rows, torch.gather(ic, 1, order))
    for q in (PQ[:, C:], None):
        want = ops.edge_gather_max(PQ[:, :C], q, idx, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01)
        for packed in (i16, i16_plain):
            buf = torch.full((M, C + 8), -7.0, device=cuda)
            ops.edge_gather_maxw(PQ[:, :C], q, packed, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01, out=buf[:, 4:4 + C])
            assert torch.equal(buf[:, 4:4 + C], want)
            assert (buf[:, :4] == -7.0).all() and (buf[:, 4 + C:] == -7.0).all()
    if N % 128 == 0:      # cloud-panel operands
        pq = ops.panels_empty(B, N, 2 * C, cuda)
        pq[:, :C // 8] = ops.rows_to_panels(PQ[:, :C].contiguous(), B)
        pq[:, C // 8:] = ops.rows_to_panels(PQ[:, C:].contiguous(), B)
        out = ops.panels_empty(B, N, C, cuda)
        ops.edge_gather_maxw(pq[:, :C // 8], pq[:, C // 8:], i16, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01, out=out)
        want = ops.edge_gather_max(PQ[:, :C], PQ[:, C:], idx, N, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.01)
        assert torch.equal(ops.panels_to_rows(out), want)


@pytest.mark.parametrize("M,KA,KB", [(8192, 128, 64), (20000, 256, 128), (4096 + 37, 1024, 512), (70000, 512, 128),
                                     # the next three satisfy gemm_tn_256(), but tn_tr_tb() takes them first: gemm_tn_tr_kernel<false, 256>.
                                     # gemm_tn_x3_256_kernel runs under LPD_DEBUG=tn-tr=0 only (tests/tn_routes.py, tests/test_tn_routes_gpu.py)
                                     (16384, 1024, 512), (8352, 256, 256), (33 * 1024 + 32, 512, 256),
                                     (16384, 512, 64), (2048, 256, 192)])
def test_gemm_tn_weight_gradient_kernel(cuda, M, KA, KB):
    """lpd_gemm_tn: dW = A^T B over the rows (register-transposed staging, split-bf16): fp32-grade against fp64, ragged row
    counts, column-slice operands, and agreement with the generic k-major product.  Products with KA % 256 == 0 over whole 32-row
    chunks and M >= 2048 run on the transposed-read kernel (gemm_tn_tr_kernel: 256-, 128- and 64-wide b tiles, odd and even chunk
    counts per split, a short last split), everything else on gemm_tn_x3_kernel<128 | 64>: here (8192, 128, 64), the two shapes with
    M % 32 != 0, every `rows = M - 100` call and every batched call (fp32 rows, batched, stay off the transposed-read kernel).  No
    shape of this test reaches gemm_tn_x3_256_kernel; tests/tn_routes.py states the route of a shape, tests/test_tn_routes_gpu.py runs
    each route per element against float64."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + KA)
    wide = torch.randn(M, KA + KB + 8, generator=g).to(cuda)
    A, B = wide[:, 4:4 + KA], wide[:, 4 + KA:4 + KA + KB]
    ref = A.double().t() @ B.double()
    got = ops.gemm_tn(A, B)
    assert _rel(got, ref) < 2e-5
    got_r = ops.gemm_tn(A, B, rows=M - 100)
    assert _rel(got_r, A[:M - 100].double().t() @ B[:M - 100].double()) < 2e-5
    old = ops.gemm(A.contiguous(), B.contiguous(), a_kmajor=True, b_kmajor=True, splits=8)
    assert _rel(got, old) < 2e-5
    if M <= 20000:      # batched form (the NetVLAD pooling: one problem per cloud)
        nb = 3
        A3 = torch.randn(nb, M // 4, KA, generator=g).to(cuda)
        B3 = torch.randn(nb, M // 4, KB, generator=g).to(cuda)
        got3 = ops.gemm_tn(A3, B3)
        assert got3.shape == (nb, KA, KB)
        assert _rel(got3, torch.einsum("bma,bmc->bac", A3.double(), B3.double())) < 2e-5


# ------------------------------------------------------------------ split-bf16 planes + lpd_gemm_p8 (conv3 of the eval path)
def _split_ref(x):
    """hi = bf16(x), lo = bf16(x - hi) as torch computes them (round to nearest even)"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


@pytest.mark.parametrize("Bc,Np,K,N,act,panels", [(2, 256, 512, 1024, 2, False), (3, 512, 64, 256, 1, True), (1, 768, 512, 512, 0, True),
                                                  (9, 256, 96, 256, 2, False), (32, 256, 512, 1024, 2, True)])
def test_gemm_p8_split_panels(cuda, Bc, Np, K, N, act, panels):
    """lpd_gemm_p8 (256 x 256 tiles, LDS-DMA ring, persistent workgroups; pre-split bf16 cloud-panel A, prepared weight fragments)
    against a float64 product: fp32-grade (three products per term), every epilogue term, row-major and cloud-panel C, tile counts
    below / at / above one tile per workgroup, K from 2 to 16 ring K-tiles; 10 repeated launches are bit-identical (a race in the
    DMA ring shows up as run-to-run differences); lpd_split_panels reproduces torch's hi / lo rounding bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(7 + Bc + Np + K + N)
    M = Bc * Np
    X = (torch.randn(M, K, generator=g) * 2.0).to(cuda)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    sc, sh = torch.randn(N, generator=g).to(cuda), torch.randn(N, generator=g).to(cuda)
    S = ops.split_panels(ops.rows_to_panels(X, Bc))
    hi, lo = _split_ref(X)
    to_rows = lambda P: P.permute(0, 2, 1, 3).reshape(M, K)
    assert torch.equal(to_rows(S[0]), hi) and torch.equal(to_rows(S[1]), lo)
    ref = (X.double() @ W.double().t()) * sc.double() + sh.double()
    ref = ref if act == 0 else torch.where(ref > 0, ref, ref * (0.0 if act == 1 else 0.05))
    for impl in (5, 6):
        ops.P8_IMPL = impl
        try:
            if panels:
                wide = ops.panels_empty(Bc, Np, N + 64, cuda)
                wide.fill_(-7.0)
                out = ops.gemm_p8(S, W, scale=sc, shift=sh, act=act, slope=0.05, out=wide[:, 4:4 + N // 8], out_panels=True)
                rows = ops.panels_to_rows(out)
                assert bool((wide[:, :4] == -7.0).all()) and bool((wide[:, 4 + N // 8:] == -7.0).all())
            else:
                buf = torch.full((M, N + 8), -7.0, device=cuda)
                rows = ops.gemm_p8(S, W, scale=sc, shift=sh, act=act, slope=0.05, out=buf[:, 4:4 + N])
                assert bool((buf[:, :4] == -7.0).all()) and bool((buf[:, 4 + N:] == -7.0).all())
            assert _rel(rows, ref) < 2e-5
            first = rows.clone()
            for _ in range(10):
                again = ops.gemm_p8(S, W, scale=sc, shift=sh, act=act, slope=0.05, out_panels=panels)
                assert torch.equal(ops.panels_to_rows(again) if panels else again, first)
        finally:
            ops.P8_IMPL = 0
    bare = ops.gemm_p8(S, W)
    assert _rel(bare, X.double() @ W.double().t()) < 2e-5
    with pytest.raises(ValueError):
        ops.gemm_p8(S[:, :, :, :Np - 128], W)            # clouds must be multiples of 256 points


@pytest.mark.parametrize("C,N,B,hasq", [(256, 4096, 2, True), (128, 1024, 3, True), (64, 512, 2, False), (256, 3800, 1, True)])
def test_kagg_split_output_is_the_split_of_the_fp32_output(cuda, C, N, B, hasq):
    """lpd_edge_gather_max16s: the hi / lo planes the cloud-resident K-agg writes for conv3 are bit for bit bf16(x) and
    bf16(x - bf16(x)) of the fp32 result of lpd_edge_gather_max16 (persistent and one-item-per-workgroup forms), written into a
    panel sub-range of a wider pair of planes with untouched neighbours."""
    ops = _ops()
    P, Q, idx, scale, shift = _edge_inputs(B, N, C, 20, C + N + 3)
    Pp, Qp = ops.rows_to_panels(P.to(cuda), B), ops.rows_to_panels(Q.to(cuda), B)
    idx16 = ops.pack_idx16(idx.to(cuda))
    q = Qp if hasq else None
    want = ops.panels_to_rows(ops.edge_gather_max16(Pp, q, idx16, N, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY,
                                                    slope=0.01, out=ops.panels_empty(B, N, C, cuda)))
    wide = ops.split_panels_empty(B, N, C + 128, cuda)
    wide.fill_(3.0)
    got = ops.edge_gather_max16(Pp, q, idx16, N, scale=scale.to(cuda), shift=shift.to(cuda), act=ops.ACT_LEAKY, slope=0.01,
                                out=wide[:, :, 8:8 + C // 8])
    hi, lo = _split_ref(want)
    to_rows = lambda Pn: Pn.permute(0, 2, 1, 3).reshape(B * N, C)
    assert torch.equal(to_rows(got[0]), hi) and torch.equal(to_rows(got[1]), lo)
    assert bool((wide[:, :, :8] == 3.0).all()) and bool((wide[:, :, 8 + C // 8:] == 3.0).all())
    assert _rel(ops.split_to_rows(got), want) < 2e-5
    # row-major P | Q (the DG1 stage: halves of one projection output) into split planes
    PQ = torch.cat([P, Q], dim=1).to(cuda)
    got2 = ops.edge_gather_max16(PQ[:, :C], PQ[:, C:] if hasq else None, idx16, N, scale=scale.to(cuda), shift=shift.to(cuda),
                                 act=ops.ACT_LEAKY, slope=0.01, out=ops.split_panels_empty(B, N, C, cuda))
    assert torch.equal(to_rows(got2[0]), hi) and torch.equal(to_rows(got2[1]), lo)


@pytest.mark.parametrize("CM,N,B", [(128, 512, 2), (64, 256, 4)])
def test_edge_mlp_split_output_and_x3t_on_split_planes(cuda, CM, N, B):
    """lpd_edge_mlp_bf16x3s writes the x2 block as hi / lo planes (bit for bit the split of its fp32 output), and lpd_gemm_x3ts
    multiplies those planes: bit-identical to lpd_gemm_x3t on the fp32 panels (the same LDS images, the same products)."""
    ops = _ops()
    k = 20
    P, Q, idx, s1, b1 = _edge_inputs(B, N, CM, k, CM + N)
    g = torch.Generator().manual_seed(5)
    W2 = (torch.randn(CM, CM, generator=g) / CM ** 0.5).to(cuda)
    s2, b2 = torch.randn(CM, generator=g).to(cuda), torch.randn(CM, generator=g).to(cuda)
    args = (P.to(cuda), Q.to(cuda), idx.to(cuda), N, s1.to(cuda), b1.to(cuda), W2, s2, b2)
    want_p = ops.edge_mlp(*args, act=ops.ACT_LEAKY, slope=0.01, out=ops.panels_empty(B, N, CM, cuda))
    want = ops.panels_to_rows(want_p)
    wide = ops.split_panels_empty(B, N, CM + 64, cuda)
    wide.fill_(3.0)
    got = ops.edge_mlp(*args, act=ops.ACT_LEAKY, slope=0.01, out=wide[:, :, 4:4 + CM // 8])
    hi, lo = _split_ref(want)
    to_rows = lambda Pn: Pn.permute(0, 2, 1, 3).reshape(B * N, CM)
    assert torch.equal(to_rows(got[0]), hi) and torch.equal(to_rows(got[1]), lo)
    assert bool((wide[:, :, :4] == 3.0).all()) and bool((wide[:, :, 4 + CM // 8:] == 3.0).all())
    if N % 128 == 0:
        Wp = (torch.randn(2 * CM, CM, generator=g) / CM ** 0.5).to(cuda)
        a = ops.gemm(want_p, Wp, b_kmajor=False, a_panels=True, out_panels=True)
        b = ops.gemm_x3t_split(got, Wp)
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,k,B,act", [(512, 20, 2, "leaky"), (4096, 20, 2, "leaky"), (256, 7, 3, "relu"), (64, 20, 5, "leaky")])
def test_edge_mlp_with_the_dg1_kagg_riding_along(cuda, N, k, B, act):
    """lpd_edge_mlp_x1_bf16x3s: the fused DG1 -> DG2 stage on 32-point blocks that also writes x1 = max over k of the stage-1
    activation (the DG1-stage K-agg, util/lpdnet_model.py:249-250).  x2 is bit-identical to the 64-point kernel's planes (the same
    products in the same order); x1 equals the split of the fp64 evaluation act(s1 (sel P + Q) + b1) to one ulp of the 16-bit split
    (the standalone K-agg kernel rounds the same expression in a different order) and lpd_edge_gather_max16s to a unit of the lo plane;
    BatchNorm scales of both signs (max and min selection); the planes around the written ranges stay untouched."""
    ops = _ops()
    CM = 128
    P, Q, idx, s1, b1 = _edge_inputs(B, N, CM, k, 31 * N + k)
    g = torch.Generator().manual_seed(N + k)
    W2 = (torch.randn(CM, CM, generator=g) / CM ** 0.5).to(cuda)
    s2, b2 = torch.randn(CM, generator=g).to(cuda), torch.randn(CM, generator=g).to(cuda)
    code, slope = (ops.ACT_LEAKY, 0.01) if act == "leaky" else (ops.ACT_RELU, 0.0)
    args = (P.to(cuda), Q.to(cuda), idx.to(cuda), N, s1.to(cuda), b1.to(cuda), W2, s2, b2)
    assert ops.edge_mlp_x1_applies(B * N, N, CM, CM)
    wide = ops.split_panels_empty(B, N, 512, cuda)
    wide.fill_(3.0)
    x1v, x2v = wide[:, :, 0:16], wide[:, :, 16:32]
    ops.edge_mlp(*args, act=code, slope=slope, out=x2v, x1_out=x1v)
    want2 = ops.edge_mlp(*args, act=code, slope=slope, out=ops.split_panels_empty(B, N, CM, cuda))
    assert torch.equal(x2v, want2)
    assert bool((wide[:, :, 32:] == 3.0).all())
    # x1 against fp64
    Pd, Qd = P.double(), Q.double()
    nb = (idx.long() + (torch.arange(B).view(B, 1, 1) * N)).view(B * N, k)
    y = s1.double() * (Pd[nb] + Qd.unsqueeze(1)) + b1.double()                      # [M, k, C]
    ref = y.max(dim=1).values
    ref = torch.where(ref > 0, ref, ref * slope)
    got = ops.split_to_rows(x1v).double().cpu()
    assert _rel(got, ref) < 2e-5
    hi, lo = _split_ref(ref.float().to(cuda))
    to_rows = lambda Pn: Pn.permute(0, 2, 1, 3).reshape(B * N, CM)
    assert (to_rows(x1v[0]).float() - hi.float()).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()      # hi planes within an ulp
    # ... and against the standalone K-agg kernel on the same graph
    if k == 20:
        sep = ops.split_panels_empty(B, N, CM, cuda)
        ops.edge_gather_max16(args[0], args[1], ops.pack_idx16(args[2]), N, scale=args[4], shift=args[5], act=code, slope=slope, out=sep)
        assert _rel(ops.split_to_rows(sep), ops.split_to_rows(x1v)) < 2e-5      # (one unit of the lo plane: 2^-17 of the value)
    with pytest.raises(Exception):      # the x1 planes need the shape and strides of the x2 planes
        ops.edge_mlp(*args, act=code, slope=slope, out=x2v, x1_out=wide[:, :, 0:8])


@pytest.mark.parametrize("Bc,Np,K,N,panels", [(2, 256, 512, 1024, False), (5, 512, 128, 256, True), (32, 256, 512, 1024, False)])
def test_gemm_p8_fused_assignment_product(cuda, Bc, Np, K, N, panels):
    """lpd_gemm_p8_fused: conv3 and the NetVLAD assignment product of its output in one launch.  C is bit-identical to the plain
    kernel's; every partial plane parts[j] = C[:, 256 j : 256 j + 256] @ W2[256 j : 256 j + 256] to fp32 grade against float64;
    repeated launches are bit-identical; lpd_softmax_affine_parts = softmax of the affine of the summed planes + per-cloud sums."""
    ops = _ops()
    g = torch.Generator().manual_seed(11 + Bc + Np + K + N)
    M = Bc * Np
    X = (torch.randn(M, K, generator=g) * 2.0).to(cuda)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    W2 = torch.nn.Parameter((torch.randn(N, 64, generator=g) / N ** 0.5).to(cuda))
    sh = torch.randn(N, generator=g).to(cuda)
    S = ops.split_panels(ops.rows_to_panels(X, Bc))
    plain = ops.gemm_p8(S, W, shift=sh, act=ops.ACT_LEAKY, slope=0.01, out_panels=panels)
    out, parts = ops.gemm_p8(S, W, shift=sh, act=ops.ACT_LEAKY, slope=0.01, out_panels=panels, assign_w=W2.data)
    assert torch.equal(out, plain)
    rows = (ops.panels_to_rows(out) if panels else out).double()
    assert parts.shape == (N // 256, M, 64)
    for j in range(N // 256):
        ref = rows[:, 256 * j:256 * j + 256] @ W2.data[256 * j:256 * j + 256].double()
        assert _rel(parts[j], ref) < 2e-5, j
    for _ in range(5):
        o2, p2 = ops.gemm_p8(S, W, shift=sh, act=ops.ACT_LEAKY, slope=0.01, out_panels=panels, assign_w=W2.data)
        assert torch.equal(o2, out) and torch.equal(p2, parts)
    sc, b = (0.5 + torch.rand(64, generator=g)).to(cuda), torch.randn(64, generator=g).to(cuda)
    a, ws = ops.softmax_affine_parts(parts, sc, b, colsum_rows=Np)
    want = torch.softmax(parts.double().sum(0) * sc.double() + b.double(), dim=1)
    assert _rel(a, want) < 1e-5
    assert _rel(ws[:, :64], want.view(Bc, Np, 64).sum(1)) < 1e-5 and bool((ws[:, 64:] == 0).all())


@pytest.mark.parametrize("M,N,K", [(4096, 1024, 512), (5000, 128, 128), (2048 + 77, 256, 256)])
def test_gemm_epilogue_batchnorm_statistics(cuda, M, N, K):
    """lpd_gemm_x3w_stats: the train-mode BatchNorm statistics of a layer from its GEMM's epilogue equal those of the separate
    pass (lpd_colstats) over the same output -- scale / shift / mean / invstd to 1e-6, running statistics updated once -- for
    row counts that are not multiples of the 128-row blocks, and the product itself is the plain kernel's, bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    X = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(cuda)
    W = torch.nn.Parameter((torch.randn(N, K, generator=g) / K ** 0.5).to(cuda))
    bn1, bn2 = torch.nn.BatchNorm1d(N).to(cuda), torch.nn.BatchNorm1d(N).to(cuda)
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.copy_(torch.linspace(0.5, 1.5, N))
            bn.bias.copy_(torch.linspace(-0.2, 0.2, N))
    prof = ops.PROFILE = {}
    try:
        y, st = ops.linear_bn_stats(X, W.data, bn1)
    finally:
        ops.PROFILE = None
    assert any(k.startswith("gemmx3w+stats") for k in prof) and "colstats" not in prof, list(prof)
    y2 = ops.linear(X, W.data)
    st2 = ops.bn_train_stats(y2, bn2)
    assert torch.equal(y, y2) or _rel(y, y2) < 1e-6
    for a, b in ((st.scale, st2.scale), (st.shift, st2.shift), (st.mean, st2.mean), (st.invstd, st2.invstd),
                 (bn1.running_mean, bn2.running_mean), (bn1.running_var, bn2.running_var)):
        assert _rel(a, b) < 2e-6
    ref = X.double() @ W.data.double().t()
    assert _rel(st.mean, ref.mean(0)) < 1e-5 and _rel(st.invstd, 1.0 / torch.sqrt(ref.var(0, unbiased=False) + 1e-5)) < 1e-5
    assert int(bn1.num_batches_tracked) == 1


def test_dg2_backward_without_dz_fp32_storage(cuda):
    """fp32 storage: dW2 from one pass over Y1e (arg-max product + Gram matrix + column sums, split-bf16 products) and dY1e = dZ W2 with dZ
    generated in the operand loader (csrc/lpd_train3.hip (2f), (3f)) against fp64 and against the materialised dZ path."""
    ops = _ops()
    C, N, k, B = 128, 320, 20, 2
    M = B * N
    g = torch.Generator().manual_seed(11)
    Y = torch.relu(torch.randn(M * k, C, generator=g)).to(cuda) + 0.05
    W = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    Z = (Y.double() @ W.double().t()).float().contiguous()
    act, slope = ops.ACT_LEAKY, 0.01
    bn = _bn_for(C, 6).to(cuda).train()
    st = ops.bn_train_stats(Z, bn)
    out = torch.empty(M, C, device=cuda)
    arg, sel = ops.group_max(Z, k, st.scale, st.shift, act, slope, out, keep_sel=True)
    dOut = torch.randn(M, C, generator=g).to(cuda)
    assert ops.dg2_bwd_fused_applies(M, k, C)
    dpre, red = ops.bn_sel_bwd_reduce(dOut, sel, st, act, slope, dtype=torch.float32)
    dZ_old, dg_old, db_old = ops.edge_bn_bwd(dOut, arg, k, Z, st, act, slope, xsel=sel)
    assert torch.equal(red[0].float(), db_old) and torch.equal(red[1].float(), dg_old)
    pre = st.scale.double() * sel.double() + st.shift.double()
    dpre64 = dOut.double() * torch.where(pre > 0, 1.0, slope)
    assert _rel(dpre, dpre64) < 1e-6
    D = torch.zeros(M, k, C, dtype=torch.float64, device=cuda)
    D.scatter_(1, arg.long().view(M, 1, C), dpre64.view(M, 1, C))
    m1, m2 = red[0] / (M * k), red[1] / (M * k)
    dZ = st.scale.double() * (D.view(M * k, C) - m1 - (Z.double() - st.mean.double()) * st.invstd.double() * m2)
    assert _rel(dZ_old, dZ) < 1e-5
    dW_new = ops.edge_dw_sel_f32(Y, arg, dpre, k, W, st, red)
    assert _rel(dW_new, dZ.t() @ Y.double()) < 3e-5, _rel(dW_new, dZ.t() @ Y.double())
    dY_new = ops.gemm_f32s_bnbwd(Z, arg, dpre, k, W, st, red)
    assert _rel(dY_new, dZ @ W.double()) < 2e-5, _rel(dY_new, dZ @ W.double())


@pytest.mark.parametrize("M,N,K,bk,nb", [(16384, 256, 64, False, 1), (32768, 96, 128, True, 1), (4096, 1024, 128, False, 5), (2048, 64, 64, False, 9)])
def test_gemm_x3t_rows_short_reductions(cuda, M, N, K, bk, nb):
    """lpd_gemm_x3t_rows (transposed MFMA on row-major operands, result tiles through a wave-private LDS tile, per-problem weight fragments
    when batched): ops.gemm routes K in {64, 128} products over >= 16384 rows to it -- against fp64 and against the block kernel, with bias,
    BatchNorm affine, LeakyReLU and a strided A."""
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    shape_a = (nb, M, K + 8) if nb > 1 else (M, K + 8)
    A = torch.randn(shape_a, generator=g).to(cuda)[..., 4:4 + K]
    Wt = (torch.randn(((nb,) if nb > 1 else ()) + ((K, N) if bk else (N, K)), generator=g) / K ** 0.5).to(cuda)
    bias, scale, shift = torch.randn(N, generator=g).to(cuda), (torch.rand(N, generator=g) + 0.5).to(cuda), torch.randn(N, generator=g).to(cuda)
    kw = dict(a_kmajor=False, b_kmajor=bk) if nb > 1 else dict(b_kmajor=bk, bias=bias, scale=scale, shift=shift, act=ops.ACT_LEAKY, slope=0.2)
    assert ops.X3T_ROWS
    got = ops.gemm(A.contiguous() if nb > 1 else A, Wt, **kw)
    Wd = Wt.double() if bk else Wt.double().transpose(-1, -2)
    ref = A.double() @ Wd
    if nb == 1:
        ref = torch.nn.functional.leaky_relu((ref + bias.double()) * scale.double() + shift.double(), 0.2)
    assert _rel(got, ref) < 2e-5, _rel(got, ref)
    ops.X3T_ROWS = False
    try:
        old = ops.gemm(A.contiguous() if nb > 1 else A, Wt, **kw)
    finally:
        ops.X3T_ROWS = True
    assert _rel(got, old) < 2e-5


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,k,B", [(320, 20, 2), (256, 7, 3)])
def test_edge_mlp_train_equals_the_materialised_stage(cuda, bf16, N, k, B):
    """lpd_edge_mlp_train (train-mode DG1 -> DG2 stage in one launch, the raw edge tensor U1 never written; x1 and its arg-max from
    the split-form statistics pass) against the materialised chain edge_build -> act / max -> product -> statistics / selection:
    Y1e, Z, BatchNorm2 statistics, selected values and slots, x1 -- and the DG1 BatchNorm backward fed with Y1e (post-activation,
    pre-activation recovered) against the one fed with U1: dU1, dQ, dgamma, dbeta.  fp32 storage: three split-bf16 products on
    both sides; bf16 storage: the product takes the ROUNDED Y1e, the stored tensors equal the rounded fp32 ones."""
    ops = _ops()
    C, M = 128, B * N
    P, Q, idx, _, _ = _edge_inputs(B, N, C, k, 900 + N + k)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    act, slope = ops.ACT_LEAKY, 0.01
    g = torch.Generator().manual_seed(N)
    W2 = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    bn1a, bn1b, bn2a, bn2b = [_bn_for(C, 3 + i // 2).to(cuda).train() for i in range(4)]
    with torch.no_grad():
        bn2a.weight[::3].neg_()
        bn2b.weight.copy_(bn2a.weight)      # negative scales: the selection is a minimum there
        # |gamma1| >= 0.2: the post-activation form takes xhat = (pre - beta) / gamma, so a stored value's rounding reaches xhat as
        # 2^-9 |xhat + beta / gamma| (the raw form: 2^-9 |xhat + mu / sigma|) -- neither is the yardstick of the other for |gamma| << |beta|
        w1 = bn1a.weight
        w1.copy_(torch.where(w1.abs() < 0.2, torch.where(w1 < 0, -0.2, 0.2).to(w1), w1))
        bn1b.weight.copy_(w1)
    # ---- materialised reference, fp32 tensors
    U, st1 = ops.edge_build(P, Q, idx, N, bn=bn1a)
    x1_a = torch.empty(M, C, device=cuda)
    Y_a, arg1_a = ops.edge_act_max(U, k, st1, act, slope, out=x1_a)
    Yin = Y_a.to(torch.bfloat16).float() if bf16 else Y_a
    Z_a = ops.gemm(Yin, W2, b_kmajor=False)                                      # split-bf16 product (three terms)
    st2_a = ops.bn_train_stats(Z_a, bn2a)
    x2_a = torch.empty(M, C, device=cuda)
    arg2_a, zsel_a = ops.group_max(Z_a, k, st2_a.scale, st2_a.shift, act, slope, x2_a, keep_sel=True)
    # ---- one launch
    _, usel, arg1_b, st1b = ops.edge_split_fwd(P, Q, idx, N, bn=bn1b)
    x1_b = ops.affine_act(usel, st1b.scale, st1b.shift, act, slope)
    assert ops.edge_mlp_train_applies(M, N, k, C, act, slope)
    Y_b, Z_b, zsel_b, arg2_b, st2_b = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, bn2b, act, slope, bf16, z_bf16=bf16)
    if not bf16:      # the default of the fp32 storage mode: Z rounded to bf16, everything else as with fp32 Z
        bn2c = _bn_for(C, 4).to(cuda).train()
        with torch.no_grad():
            bn2c.weight.copy_(bn2a.weight)
        Y_c, Z_c, zsel_c, arg2_c, _ = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, bn2c, act, slope, False)
        assert Z_c.dtype == torch.bfloat16 and torch.equal(Z_c, Z_b.to(torch.bfloat16)) and torch.equal(Y_c, Y_b)
        assert torch.equal(zsel_c, zsel_b) and torch.equal(arg2_c, arg2_b)
    assert torch.equal(arg1_a, arg1_b) and _rel(x1_b, x1_a) < 1e-5
    assert _rel(st1b.mean, st1.mean) < 1e-5 and _rel(st1b.invstd, st1.invstd) < 1e-5
    if bf16:
        assert Y_b.dtype == torch.bfloat16 and Z_b.dtype == torch.bfloat16
        # the rounded fp32 value, up to one bf16 ulp where the fused kernel's fma and the chain's multiply + add round apart
        assert ((Y_b.float() - Y_a.to(torch.bfloat16).float()).abs() <= 2.0 ** -7 * Y_a.abs() + 1e-6).all()      # (+ values around 0)
        assert (Y_b.float() != Y_a.to(torch.bfloat16).float()).float().mean().item() < 0.01
        assert _rel(Z_b.float(), Z_a) < 2 ** -8
        tol = 3e-3          # statistics / selection of the fp32 accumulators against those of an independently rounded product
    else:
        assert _rel(Y_b, Y_a) < 1e-6 and _rel(Z_b, Z_a) < 2e-5
        tol = 2e-5
    assert _rel(st2_b.mean, st2_a.mean) < tol and _rel(st2_b.invstd, st2_a.invstd) < tol
    assert _rel(bn2b.running_mean, bn2a.running_mean) < tol and _rel(bn2b.running_var, bn2a.running_var) < tol
    assert _rel(zsel_b, zsel_a) < tol
    same = (arg2_a == arg2_b).float().mean().item()
    assert same > (0.995 if bf16 else 0.9995), same          # a near-tie between two slots may fall the other way
    # selected values are consistent with the stored Z: zsel[i][c] = Z[(i, arg2[i][c])][c] up to the storage rounding
    pick = torch.gather(Z_b.float().view(M, k, C), 1, arg2_b.long().unsqueeze(1)).squeeze(1)
    assert _rel(pick, zsel_b) < (2 ** -8 if bf16 else 1e-6)
    # ---- DG1 BatchNorm backward: post-activation form (Y1e) against the raw form (U1), same dense gradient
    dOut = torch.randn(M, C + 8, generator=g).to(cuda)[:, 4:4 + C]
    dense = torch.randn(M * k, C, generator=g).to(cuda)
    if bf16:
        dq_a, dq_b = torch.empty(M, C, device=cuda), torch.empty(M, C, device=cuda)
        U16 = U.to(torch.bfloat16)
        Y16 = ops.affine_act(U16.float(), st1.scale, st1.shift, act, slope).to(torch.bfloat16)      # Y of the SAME rounded U
        dU_a, dg_a, db_a = ops.edge_bn_bwd_bf16(dOut, arg1_a, k, U16, st1, act, slope, dense=dense.to(torch.bfloat16), dQ=dq_a)
        dU_b, dg_b, db_b = ops.edge_bn_bwd_bf16(dOut, arg1_a, k, Y16, st1, act, slope, dense=dense.to(torch.bfloat16), dQ=dq_b, post_bn=bn1a)
        assert _rel(dU_b.float(), dU_a.float()) < 2e-2 and _rel(dq_b, dq_a) < 2e-2 and _rel(dg_b, dg_a) < 2e-2 and _rel(db_b, db_a) < 1e-3
    else:
        dq_a, dq_b = torch.empty(M, C, device=cuda), torch.empty(M, C, device=cuda)
        dU_a, dg_a, db_a = ops.edge_bn_bwd(dOut, arg1_a, k, U, st1, act, slope, dense=dense.clone(), dQ=dq_a)
        dU_b, dg_b, db_b = ops.edge_bn_bwd(dOut, arg1_a, k, Y_a, st1, act, slope, dense=dense.clone(), dQ=dq_b, post_bn=bn1a)
        assert _rel(dU_b, dU_a) < 2e-4 and _rel(dq_b, dq_a) < 2e-4 and _rel(dg_b, dg_a) < 2e-4 and _rel(db_b, db_a) < 1e-5


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,k,B", [(320, 20, 2), (256, 16, 3), (64, 16, 1)])      # the last: fewer than 8 blocks in the gather pass (N % 64 == 0, k >= 16: the kernels' contract)
def test_edge_mlp_train_bwd_equals_the_chain(cuda, bf16, N, k, B):
    """lpd_edge_mlp_train_bwd + lpd_edge_dense_bwd_apply (DG2 dY1e product with dZ built in the operand loader, the gradient in front of
    BatchNorm1 and its reductions in the epilogue, dP / dQ in closed form from one gather pass) against the chain they replace:
    gemm_*_bnbwd -> edge_bn_bwd* (post-activation form) -> gather_sum_rows*: dP, dQ, dgamma1, dbeta1."""
    ops = _ops()
    C, M = 128, B * N
    P, Q, idx, _, _ = _edge_inputs(B, N, C, k, 1900 + N + k)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    act, slope = ops.ACT_LEAKY, 0.01
    g = torch.Generator().manual_seed(N + 1)
    W2 = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    bn1, bn2 = _bn_for(C, 3).to(cuda).train(), _bn_for(C, 4).to(cuda).train()
    with torch.no_grad():
        w1 = bn1.weight
        w1.copy_(torch.where(w1.abs() < 0.2, torch.where(w1 < 0, -0.2, 0.2).to(w1), w1))
    s1sum, usel, arg1, st1 = ops.edge_split_fwd(P, Q, idx, N, bn=bn1)
    Y, Z, zsel, arg2, st2 = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, bn2, act, slope, bf16)
    assert Z.dtype == torch.bfloat16                     # both storage modes keep Z as bf16 (only the backward's xhat2 m2 term reads it)
    Zc = Z if bf16 else ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, _bn_for(C, 4).to(cuda).train(), act, slope, False,
                                           z_bf16=False)[1]      # fp32 Z for the chain's fp32 product kernel
    dcat = torch.randn(M, 512, generator=g).to(cuda)
    dx1, dx2 = dcat[:, 0:128], dcat[:, 128:256]
    dt = torch.bfloat16 if bf16 else torch.float32
    dpre2, red2 = ops.bn_sel_bwd_reduce(dx2, zsel, st2, act, slope, dtype=dt)
    graph = ops.GraphT(idx, N)
    # ---- the chain
    dY = (ops.gemm_bf16s_bnbwd if bf16 else ops.gemm_f32s_bnbwd)(Zc, arg2, dpre2, k, W2, st2, red2)
    dq_a, dp_a = torch.empty(M, C, device=cuda), torch.empty(M, C, device=cuda)
    if bf16:
        dU, dg_a, db_a = ops.edge_bn_bwd_bf16(dx1, arg1, k, Y, st1, act, slope, dense=dY, dQ=dq_a, post_bn=bn1)
        ops.gather_sum_rows_bf16(dU, graph, dp_a)
    else:
        dU, dg_a, db_a = ops.edge_bn_bwd(dx1, arg1, k, Y, st1, act, slope, dense=dY, dQ=dq_a, post_bn=bn1)
        ops.gather_sum_rows(dU, graph, dp_a)
    # ---- two launches
    G, gsum, red1 = ops.edge_mlp_train_bwd(Z, arg2, dpre2, W2, st2, red2, Y, arg1, dx1, bn1, k, act, slope)
    buf = torch.zeros(M, 2 * C + 8, device=cuda)
    ops.edge_dense_bwd_apply(G, gsum, s1sum, P, Q, graph, st1, red1, k, dP=buf[:, 4:4 + C], dQ=buf[:, 4 + C:4 + 2 * C])
    r1 = red1.float()
    tol = 2e-2 if bf16 else 3e-4        # bf16: the chain rounds dY1e AND dU1 to bf16, the new form G only
    assert _rel(r1[0], db_a) < tol and _rel(r1[1], dg_a) < tol
    assert _rel(buf[:, 4:4 + C], dp_a) < tol and _rel(buf[:, 4 + C:4 + 2 * C], dq_a) < tol
    assert (buf[:, :4] == 0).all() and (buf[:, 4 + 2 * C:] == 0).all()
    assert _rel(gsum, G.float().view(M, k, C).sum(1)) < (1e-2 if bf16 else 1e-5)
    # ---- without Z (ops.EDGE_NOZ, bf16 storage): the forward stores none (same Y1e, statistics, selection), the backward takes the xhat2
    # term as Y1e K
    if not bf16:
        with pytest.raises(Exception):
            ops.edge_mlp_train_bwd(None, arg2, dpre2, W2, st2, red2, Y, arg1, dx1, bn1, k, act, slope)
        return
    bn2n = _bn_for(C, 4).to(cuda).train()
    Yn, Zn, zseln, arg2n, st2n = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, bn2n, act, slope, bf16, store_z=False)
    assert Zn is None and torch.equal(Yn, Y) and torch.equal(zseln, zsel) and torch.equal(arg2n, arg2) and torch.equal(st2n.scale, st2.scale)
    Gn, gsumn, red1n = ops.edge_mlp_train_bwd(None, arg2, dpre2, W2, st2, red2, Y, arg1, dx1, bn1, k, act, slope)
    bufn = torch.zeros_like(buf)
    ops.edge_dense_bwd_apply(Gn, gsumn, s1sum, P, Q, graph, st1, red1n, k, dP=bufn[:, 4:4 + C], dQ=bufn[:, 4 + C:4 + 2 * C])
    r1n = red1n.float()
    assert _rel(r1n[0], db_a) < tol and _rel(r1n[1], dg_a) < tol
    assert _rel(bufn[:, 4:4 + C], dp_a) < tol and _rel(bufn[:, 4 + C:4 + 2 * C], dq_a) < tol
    # the two backward forms differ by the rounding of the K product (bf16 x bf16 on the mean-sized term) against that of the stored Z
    assert _rel(Gn.float(), G.float()) < 8e-3, _rel(Gn.float(), G.float())
    assert _rel(gsumn, Gn.float().view(M, k, C).sum(1)) < 1e-2


def test_gemm_act_equals_affine_act_then_product(cuda):
    """lpd_gemm_x3w_act (BatchNorm affine + activation of the layer in front applied in the operand loader, the activated rows stored on
    the way) against affine_act followed by the prepared-fragment product: the activated map bit for bit, the product to split-bf16
    accuracy -- at the training step's shape class (K = 1024 -> 64 clusters) and with a ragged row count."""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for M in (4096, 1300):
        K, N = 1024, 64
        x = torch.randn(M, K, generator=g).to(cuda)
        w = torch.nn.Parameter((torch.randn(K, N, generator=g) / K ** 0.5).to(cuda))
        sc, sh = (0.5 + torch.rand(K, generator=g)).to(cuda), (0.3 * torch.randn(K, generator=g)).to(cuda)
        sc[::5] *= -1
        assert ops.gemm_act_applies(M, N, K)
        xa, c = ops.gemm_act(x, w.data, sc, sh, ops.ACT_LEAKY, 0.01)
        ref_a = ops.affine_act(x, sc, sh, ops.ACT_LEAKY, 0.01)
        ref_c = ops.gemm(ref_a, w.data, b_kmajor=True)
        assert torch.equal(xa, ref_a)
        assert _rel(c, ref_c) < 1e-6
        c64 = ref_a.double() @ w.data.double()
        assert _rel(c, c64) < 2e-5


def test_gemm_x3w_batched_per_problem_weights(cuda):
    """lpd_gemm_x3w_batched (one row-major A, a k-major weight per consecutive range of rows) against fp64 and against the generic
    batched kernel it replaces for the NetVLAD backward's dA[b] = x[b] . dV[b]."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    nb, M, K, N = 6, 4096, 1024, 64
    A = torch.randn(nb, M, K, generator=g).to(cuda)
    Bm = (torch.randn(nb, K, N, generator=g) / K ** 0.5).to(cuda)
    got = ops.gemm(A, Bm, a_kmajor=False, b_kmajor=True)
    want = torch.bmm(A.double(), Bm.double())
    assert got.shape == (nb, M, N) and _rel(got, want) < 2e-5
    prev, ops.X3W_BATCHED = ops.X3W_BATCHED, False
    try:
        old = ops.gemm(A, Bm, a_kmajor=False, b_kmajor=True)
    finally:
        ops.X3W_BATCHED = prev
    assert _rel(old, want) < 2e-5 and _rel(got, old) < 2e-5


def test_bf16_map_operators(cuda):
    """The bf16-storage training mode keeps the [B N, 1024] conv3 map, its activated form and both gradients as bfloat16
    (autograd.MAP_BF16).  Every kernel that reads or writes them, against fp64 on the SAME (already rounded) bf16 inputs -- a bf16 row is
    the hi image of the split product, so the products stay fp32-grade -- and the bf16 results within one rounding (2^-8 relative) of the
    fp32 kernel's."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    bf = torch.bfloat16

    def rounds_to(got16, want32):      # got is want rounded to bf16 (up to fp32 summation-order noise deciding a tie)
        assert got16.dtype == bf
        d = (got16.float() - want32).abs()
        assert bool((d <= want32.abs() * 2.0 ** -8 + 1e-6).all()), float((d / (want32.abs() + 1e-6)).max())

    # conv3 + statistics with a bf16 result (lpd_gemm_x3w_stats, c_bf16): statistics bit-identical to the fp32 launch's
    M, K, N = 4096 + 128, 512, 1024
    x = torch.randn(M, K, generator=g).to(cuda)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(cuda)
    bn_a, bn_b = torch.nn.BatchNorm1d(N).to(cuda), torch.nn.BatchNorm1d(N).to(cuda)
    y32, st32 = ops.linear_bn_stats(x, w, bn_a)
    y16, st16 = ops.linear_bn_stats(x, w, bn_b, out_bf16=True)
    rounds_to(y16, y32)
    assert torch.equal(st16.scale, st32.scale) and torch.equal(st16.shift, st32.shift) and torch.equal(bn_a.running_var, bn_b.running_var)

    # assignment product with the affine + activation in the loader: bf16 rows in, bf16 activated rows out (lpd_gemm_x3w_act flags 3)
    K2, N2 = 1024, 64
    wc = (torch.randn(K2, N2, generator=g) / K2 ** 0.5).to(cuda)
    sc, sh = (0.5 + torch.rand(K2, generator=g)).to(cuda), (0.3 * torch.randn(K2, generator=g)).to(cuda)
    sc[::5] *= -1
    for Mr in (4096, 1300):
        xr = y16[:Mr]
        xa16, c = ops.gemm_act(xr, wc, sc, sh, ops.ACT_LEAKY, 0.2, out_bf16=True)
        ref_a = ops.affine_act(xr.float(), sc, sh, ops.ACT_LEAKY, 0.2)
        assert torch.equal(xa16, ref_a.to(bf))                    # the same multiply-then-add, one rounding
        assert _rel(c, xa16.double() @ wc.double()) < 2e-5        # the product takes the STORED values
    feat16 = ops.gemm_act(y16, wc, sc, sh, ops.ACT_LEAKY, 0.2, out_bf16=True)[0]

    # pooling / weight gradients with bf16 rows as A (lpd_gemm_tn a_bf16).  M = 4224, KA = 1024: gemm_tn_tr_kernel<true, 64 | 128 | 256>;
    # rows = M - 100 is no multiple of 32: gemm_tn_x3_kernel<64 | 128, true>.  (tests/tn_routes.py states the routes.)
    for KB in (64, 128, 512):
        Bm = torch.randn(M, KB, generator=g).to(cuda)
        got = ops.gemm_tn(feat16, Bm)
        assert _rel(got, feat16.double().t() @ Bm.double()) < 2e-5
        got_r = ops.gemm_tn(feat16, Bm, rows=M - 100)
        assert _rel(got_r, feat16[:M - 100].double().t() @ Bm[:M - 100].double()) < 2e-5
    M2 = 16384
    big16 = torch.randn(M2, 1024, generator=g).to(cuda).to(bf)
    Bm = torch.randn(M2, 512, generator=g).to(cuda)
    assert _rel(ops.gemm_tn(big16, Bm), big16.double().t() @ Bm.double()) < 2e-5        # gemm_tn_tr_kernel<true, 256>, not gemm_tn_x3_256_kernel
    A3, B3 = big16.view(4, 4096, 1024), Bm[:, :64].contiguous().view(4, 4096, 64)
    assert _rel(ops.gemm_tn(A3, B3), torch.einsum("bma,bmc->bac", A3.double(), B3.double())) < 2e-5

    # dA[b] = x[b] . dV[b] with bf16 rows (lpd_gemm_x3w_batched a_bf16) and dX = dY W (lpd_gemm_x3w_bf16a), fresh and accumulating
    dV = (torch.randn(4, 1024, 64, generator=g) / 32).to(cuda)
    got = ops.gemm(A3, dV, a_kmajor=False, b_kmajor=True)
    assert got.dtype == torch.float32 and _rel(got, torch.bmm(A3.double(), dV.double())) < 2e-5
    w3 = (torch.randn(1024, 512, generator=g) / 32).to(cuda)          # [Co, Kin]: dX = dY W, k-major for this product
    dx = ops.gemm_bf16a(big16, w3, b_kmajor=True)
    want = big16.double() @ w3.double()
    assert _rel(dx, want) < 2e-5
    base = torch.randn(M2, 512, generator=g).to(cuda)
    acc = ops.gemm_bf16a(big16, w3, b_kmajor=True, out=base.clone(), accumulate=True)
    assert _rel(acc, want + base.double()) < 2e-5

    # the gradient of the map from the short batched product, stored as bf16 (lpd_gemm_x3t_rows c_bf16)
    ada = torch.randn(4, 4096, 128, generator=g).to(cuda)
    rhs = (torch.randn(4, 1024, 128, generator=g) / 11).to(cuda)
    d32 = ops.gemm(ada, rhs, a_kmajor=False, b_kmajor=False)
    d16 = ops.gemm(ada, rhs, a_kmajor=False, b_kmajor=False, out_bf16=True)
    assert torch.equal(d16, d32.to(bf))                            # the same accumulators, one rounding

    # BatchNorm + activation backward on bf16 tensors (lpd_bn_act_bwd_bf16) against the fp32 kernel on the widened inputs
    dY16, X16 = d16.view(M2, 1024), big16
    bn = torch.nn.BatchNorm1d(1024).to(cuda)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(1024, generator=g))
        bn.weight[::7] *= -1
        bn.bias.copy_(0.2 * torch.randn(1024, generator=g))
    st = ops.bn_train_stats(X16.float(), bn)
    for act in (ops.ACT_LEAKY, ops.ACT_RELU, ops.ACT_NONE):
        dx16, dg16, db16 = ops.bn_act_bwd_bf16(dY16, X16, st, act, 0.2)
        dx32, dg32, db32 = ops.bn_act_bwd(dY16.float(), X16.float(), st, act, 0.2)
        assert _rel(dg16, dg32) < 1e-5 and _rel(db16, db32) < 1e-5
        rounds_to(dx16, dx32)
    inplace = dY16.clone()
    ops.bn_act_bwd_bf16(inplace, X16, st, ops.ACT_LEAKY, 0.2, out=inplace)
    assert torch.equal(inplace, ops.bn_act_bwd_bf16(dY16, X16, st, ops.ACT_LEAKY, 0.2)[0])
    # what is not built says so
    with pytest.raises(ValueError):
        ops.gemm(ada, rhs.transpose(1, 2).contiguous(), a_kmajor=False, b_kmajor=True, out_bf16=True, splits=2)
    with pytest.raises(ValueError):
        ops.gemm(big16, w3, b_kmajor=True)


def test_bn_act_bwd_bf16_2048_columns_stays_inside_the_statistics_workspace(cuda):
    """lpd_bn_act_bwd_bf16 at C = 2048 (emb_dims = 2048): the statistics workspace holds 1024 columns per array and replica, so the
    reduction runs in two column panels.  Each half must equal the 1024-column call on that half (same kernels, same bits), and the
    workspace must come back all-zero: the next reduction on the stream is checked against a fresh computation."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    R, C = 2048 + 64, 2048
    bf = torch.bfloat16
    X = torch.randn(R, C, generator=g).to(cuda).to(bf)
    dY = (torch.randn(R, C, generator=g) / 7).to(cuda).to(bf)
    bn = torch.nn.BatchNorm1d(C).to(cuda)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.weight[::5] *= -1
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
    st = ops.bn_train_stats(X.float(), bn)
    dx, dg, db = ops.bn_act_bwd_bf16(dY, X, st, ops.ACT_LEAKY, 0.2)
    for h in (0, 1):
        sl = slice(h * 1024, (h + 1) * 1024)
        sth = ops.BNStats(st.scale[sl].contiguous(), st.shift[sl].contiguous(), st.mean[sl].contiguous(), st.invstd[sl].contiguous(), st.count)
        dxh, dgh, dbh = ops.bn_act_bwd_bf16(dY[:, sl].contiguous(), X[:, sl].contiguous(), sth, ops.ACT_LEAKY, 0.2)
        assert torch.equal(dg[sl], dgh) and torch.equal(db[sl], dbh)
        assert torch.equal(dx[:, sl], dxh)
    # fp64 reference of the two sums (the widened bf16 inputs are exact in fp64)
    pre = (st.scale.double() * X.double() + st.shift.double())
    dpre = dY.double() * torch.where(pre > 0, 1.0, 0.2)
    xhat = (X.double() - st.mean.double()) * st.invstd.double()
    assert _rel(db, dpre.sum(0)) < 1e-5 and _rel(dg, (dpre * xhat).sum(0)) < 1e-4
    # the workspace is all-zero again: a following reduction on the same stream is exact
    Y = torch.randn(4096, 1024, generator=g).to(cuda)
    bn2 = torch.nn.BatchNorm1d(1024).to(cuda)
    st2 = ops.bn_train_stats(Y, bn2)
    assert _rel(st2.mean, Y.double().mean(0)) < 1e-5
    ws = ops._STAT_WS[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
    assert float(ws.abs().max()) == 0.0


@pytest.mark.parametrize("a16", [False, True])
def test_operand_transform_without_a_stored_map(cuda, a16):
    """The NetVLAD head on the trunk's RAW last-layer output (ops.feat_in_loader_applies): the BatchNorm affine + activation is applied in
    the operand loaders of the assignment (lpd_gemm_x3w_act without a_out), the pooling and the assignment weight gradient
    (lpd_gemm_tn_act, batched and plain, strided B) and dA (lpd_gemm_x3w_batched with a_scale) -- each against the same product on the
    map lpd_gemm_x3w_act stores: equal bits for fp32 rows (the same multiply-then-add), and for bf16 rows (the same rounded map)."""
    ops = _ops()
    g = torch.Generator().manual_seed(21)
    nb, Np, E, K = 4, 4096, 1024, 64
    M = nb * Np
    raw = torch.randn(M, E, generator=g).to(cuda)
    if a16:
        raw = raw.to(torch.bfloat16)
    wc = (torch.randn(E, K, generator=g) / 32).to(cuda)
    sc, sh = (0.5 + torch.rand(E, generator=g)).to(cuda), (0.3 * torch.randn(E, generator=g)).to(cuda)
    sc[::5] *= -1
    aff = (sc, sh, ops.ACT_LEAKY, 0.2)
    assert ops.feat_in_loader_applies(nb, Np, E, K)
    stored, c_ref = ops.gemm_act(raw, wc, *aff, out_bf16=a16)
    none, c = ops.gemm_act(raw, wc, *aff, out_bf16=a16, store=False)
    assert none is None and torch.equal(c, c_ref)
    a = torch.softmax(torch.randn(M, K, generator=g), dim=1).to(cuda)
    pooled = ops.gemm_tn(raw.view(nb, Np, E), a.view(nb, Np, K), a_affine=aff)
    assert _rel(pooled, torch.einsum("bme,bmk->bek", stored.double().view(nb, Np, E), a.double().view(nb, Np, K))) < 2e-5
    if a16:      # the same kernel on the stored bf16 map: identical bits
        assert torch.equal(pooled, ops.gemm_tn(stored.view(nb, Np, E), a.view(nb, Np, K)))
    wide = torch.randn(M, 2 * K, generator=g).to(cuda)
    da0 = wide[:, K:]
    dwc = ops.gemm_tn(raw, da0, a_affine=aff)
    assert _rel(dwc, stored.double().t() @ da0.double()) < 2e-5
    dv = (torch.randn(nb, E, K, generator=g) / 32).to(cuda)
    da = ops.gemm(raw.view(nb, Np, E), dv, a_kmajor=False, b_kmajor=True, a_affine=aff)
    assert torch.equal(da, ops.gemm(stored.view(nb, Np, E), dv, a_kmajor=False, b_kmajor=True))
    with pytest.raises(ValueError):
        ops.gemm_tn(raw, wide, a_affine=aff)          # 128-wide B: not built


def test_bf16_point_feature_copy_operators(cuda):
    """bf16 storage keeps a bf16 COPY of the point features [x1 | x2 | x3] (autograd.CAT_BF16): the activation pass writes it beside the fp32
    rows (lpd_affine_act2), conv3 + statistics takes it as bf16 rows (two products per term, bf16 result), the conv3 weight gradient takes
    bf16 rows on BOTH sides (one product per term, exact in the operands)."""
    ops = _ops()
    g = torch.Generator().manual_seed(31)
    bf = torch.bfloat16
    M = 16384 + 128
    raw = torch.randn(M, 256, generator=g).to(cuda)
    sc, sh = (0.5 + torch.rand(256, generator=g)).to(cuda), (0.3 * torch.randn(256, generator=g)).to(cuda)
    cat, cat16 = torch.zeros(M, 512, device=cuda), torch.zeros(M, 512, dtype=bf, device=cuda)
    ops.affine_act(raw, sc, sh, ops.ACT_LEAKY, 0.2, out=cat[:, 256:512], out16=cat16[:, 256:512])
    want = ops.affine_act(raw, sc, sh, ops.ACT_LEAKY, 0.2)
    assert torch.equal(cat[:, 256:512], want) and torch.equal(cat16[:, 256:512], want.to(bf))
    assert (cat[:, :256] == 0).all() and (cat16[:, :256] == 0).all()
    cat[:, :256] = torch.randn(M, 256, generator=g).to(cuda)
    cat16[:, :256] = cat[:, :256].to(bf)
    # conv3 + statistics on the bf16 rows
    w = (torch.randn(1024, 512, generator=g) / 22).to(cuda)
    bn_a, bn_b = torch.nn.BatchNorm1d(1024).to(cuda), torch.nn.BatchNorm1d(1024).to(cuda)
    y16, st16 = ops.linear_bn_stats(cat16, w, bn_a, out_bf16=True)
    ref = cat16.double() @ w.double().t()
    assert y16.dtype == bf and float(((y16.double() - ref).abs() / (ref.abs() * 2.0 ** -8 + 1e-5)).max()) < 1.0
    mean_ref = ref.mean(0)
    assert _rel(st16.mean, mean_ref) < 1e-5 and _rel(st16.invstd, 1.0 / torch.sqrt(ref.var(0, unbiased=False) + bn_a.eps)) < 1e-5
    y32, st32 = ops.linear_bn_stats(cat16.float(), w, bn_b, out_bf16=True)      # the fp32-row kernel on the same values
    assert _rel(st16.scale, st32.scale) < 1e-5
    # weight gradient with bf16 rows on both sides: one product, exact in the operands
    dW = ops.gemm_tn(y16, cat16)
    assert _rel(dW, y16.double().t() @ cat16.double()) < 2e-6
    with pytest.raises(Exception):
        ops.gemm_tn(y16[:, :128].contiguous(), cat16[:, :128].contiguous())      # KA = 128: not built


@pytest.mark.gpu
def test_affine_act_bf16_only_output(cuda):
    """lpd_affine_act2 with a NULL fp32 destination (round 6: x1 and x3 of the bf16 training mode leave as bf16 rows only): the bf16 rows
    are the ones the two-output form writes, bit for bit, and nothing else is touched."""
    from lpdnet_hip import ops
    g = torch.Generator().manual_seed(5)
    X = torch.randn(4096, 128, generator=g).to(cuda)
    sc, sh = (torch.rand(128, generator=g) + 0.5).to(cuda), torch.randn(128, generator=g).to(cuda)
    both32 = torch.empty_like(X)
    wide = torch.zeros(4096, 512, dtype=torch.bfloat16, device=cuda)          # a column slice of a wider bf16 tensor, as in the trunk
    ops.affine_act(X, sc, sh, ops.ACT_LEAKY, 0.01, out=both32, out16=wide[:, 128:256])
    only = torch.full((4096, 512), 7.0, dtype=torch.bfloat16, device=cuda)
    r = ops.affine_act(X, sc, sh, ops.ACT_LEAKY, 0.01, out16=only[:, 128:256], only16=True)
    torch.cuda.synchronize()
    assert r.data_ptr() == only[:, 128:256].data_ptr()
    assert torch.equal(only[:, 128:256], wide[:, 128:256])
    assert (only[:, :128] == 7.0).all() and (only[:, 256:] == 7.0).all()
    assert torch.equal(wide[:, 128:256], both32.bfloat16())
    with pytest.raises(ValueError):
        ops.affine_act(X, sc, sh, ops.ACT_LEAKY, 0.01, only16=True)


@pytest.mark.gpu
def test_batch_pipelines_of_a_thread_share_their_streams(cuda):
    """harness.BatchPipeline takes its streams from one ring per (device, depth, host thread): a pipeline per call (PointNetVlad.forward
    makes one for every eval batch above 32 clouds) must not meet the caching allocator with fresh, empty per-stream pools each time."""
    import threading
    from lpdnet_hip import harness
    lin = torch.nn.Linear(4, 4).to(cuda)
    a, b = harness.BatchPipeline(lin, 2, cuda), harness.BatchPipeline(lin, 2, cuda)
    assert [s.cuda_stream for s in a.streams] == [s.cuda_stream for s in b.streams] and len(a.streams) == 2
    assert harness.BatchPipeline(lin, 1, cuda).streams == []
    other = []
    t = threading.Thread(target=lambda: other.append([s.cuda_stream for s in harness.BatchPipeline(lin, 2, cuda).streams]))
    t.start(); t.join()
    assert other and other[0] != [s.cuda_stream for s in a.streams]          # another host thread: its own ring
