"""Launch arithmetic of the size-dependent kernel paths, restated in Python, and the shapes at which the launch-size tests reach them.

Several kernels change what they do with the launch size alone:
  - the fused edge-MLP kernels (csrc/lpd_edge.hip em_tiles_per_block): a block walks ceil(tiles / 512) consecutive point tiles, at most 16,
    so that one resident round of blocks covers the launch; the last block may get fewer tiles (the `m0 >= g.M` exit);
  - the reduction kernels that end in fp64 atomics (csrc/lpd_common.h lpd_reduce_grid): at most 768 blocks, a grid-stride loop beyond;
  - the BatchNorm-backward products on the transposed operand loader (csrc/lpd_train3.hip): at most 256 (fp32) / 512 (bf16) blocks;
  - the training-path kernels of csrc/lpd_train.hip (grid_for: at most 4096 blocks, a grid-stride loop beyond), the slice count of
    lpd_vlad_finalize_bwd, the two paths of lpd_graph_transpose and the loops of lpd_dw_smallk;
  - the forward head, BatchNorm-apply, mining and loss kernels (csrc/lpd_misc.hip, lpd_affine_act of csrc/lpd_train.hip, csrc/lpd_loss.hip):
    the per-thread constants of affine_act, the chunk count of vlad_asum, the three softmax kernels, the loops of the gating kernel and the
    LDS sizes of hard_negatives / metric_loss (tests/test_fwd_ops_gpu.py runs them at the shapes of the FWD_* tables).
tests/test_launch_sizes_cpu.py checks every entry of the tables below against its stated regime, so a change of a heuristic shows which
cases stop covering what they claim; tests/test_launch_sizes_gpu.py, tests/test_train_bwd_ops_gpu.py and tests/test_fwd_ops_gpu.py run the
kernels at these shapes.
"""
EM_ROUND = 512        # blocks of one resident round of the fused edge-MLP kernels (two per CU)
EM_TMAX = 16          # most tiles a block walks (LPD_DEBUG=edge-mlp-tiles=n lowers it)
REDUCE_CAP = 768      # lpd_reduce_grid (LPD_DEBUG=reduce-grid=n)


def em_tiles_per_block(tiles, tmax=EM_TMAX):
    t = (tiles + EM_ROUND - 1) // EM_ROUND
    return max(1, min(t, tmax))


def em_launch(M, pts, tmax=EM_TMAX):
    """(tiles per block, grid, tiles of the last block) of a fused edge-MLP launch over M points in `pts`-point tiles"""
    tiles = (M + pts - 1) // pts
    t = em_tiles_per_block(tiles, tmax)
    grid = (tiles + t - 1) // t
    return t, grid, tiles - (grid - 1) * t


def grid_for(items, per_block, cap=4096):
    g = (items + per_block - 1) // per_block
    return max(1, min(g, cap))


def reduce_grid(wanted, cap=REDUCE_CAP):
    return max(1, min(wanted, cap))


def capped_launch(items, per_block, cap, gcap=4096):
    """(blocks wanted, blocks launched, ragged): ragged = the grid-stride walk ends in a part-filled stride"""
    wanted = grid_for(items, per_block, gcap)
    grid = min(wanted, cap)
    return wanted, grid, items % (grid * per_block) != 0


# ---- fused edge MLP: eval (edge_mlp_x3: 64-point tiles, 32-point tiles with the x1 planes) and train backward (32-point tiles;
# M % 32 == 0, and the gather pass of the backward needs N % 64 == 0 and k >= 16)
EDGE_SHAPES = {
    "t3": dict(B=5, N=8000, k=16),
    "t16": dict(B=65, N=4160, k=16),
}
# name -> {form: (tiles per block, grid, tiles of the last block)}
EDGE_REGIMES = {
    "t3": {"bwd": (3, 417, 2), "x1": (3, 417, 2), "x3": (2, 313, 1)},
    "t16": {"bwd": (16, 529, 2), "x1": (16, 529, 2), "x3": (9, 470, 4)},
}
EDGE_PTS = {"bwd": 32, "x1": 32, "x3": 64}


def edge_launch(name, form, tmax=EM_TMAX):
    s = EDGE_SHAPES[name]
    return em_launch(s["B"] * s["N"], EDGE_PTS[form], tmax)


# ---- reductions behind lpd_reduce_grid: rows per block of one grid-stride trip and the grid_for cap of each launch
def reduce_launches(op, C, R):
    """[(pass, items, per_block, grid_for cap)] of one call"""
    if op == "colstats":
        out, c0 = [], 0
        while c0 < C:
            w = 1024
            while w > C - c0:
                w >>= 1
            out.append((f"colstats[{c0}:{c0 + w}]", R, (256 // (w // 4)) * 8, 4096))
            c0 += w
        return out
    if op == "bn_act_bwd":
        return [("reduce", R, (256 // (C // 4)) * 8, 4096), ("apply", R * (C // 4), 256 * 4, 4096)]
    if op == "bn_act_bwd_bf16":
        w = min(C, 1024)
        panels = [(f"reduce[{c0}:{c0 + w}]", R, (256 // (w // 8)) * 8, 4096) for c0 in range(0, C, w)]
        return panels + [("apply", R * (C // 8), 256 * 4, 4096)]
    if op == "bn_sel_bwd_reduce":
        return [("reduce", R, (256 // (C // 4)) * 4, 4096)]
    if op == "edge_split_bwd":
        return [("reduce", R, (256 // (C // 4)) * 8, 2048)]
    raise KeyError(op)


# (op, C, rows): every pass of every call launches more than REDUCE_CAP blocks' worth of work, with a ragged last stride
REDUCE_ROWS = {64: 230_000, 128: 110_000, 1024: 14_000, 2048: 14_000}
REDUCE_CASES = ([(op, C, REDUCE_ROWS[C]) for op in ("colstats", "bn_act_bwd", "bn_act_bwd_bf16", "bn_sel_bwd_reduce") for C in (64, 128, 1024)]
                + [("bn_act_bwd_bf16", 2048, REDUCE_ROWS[2048])]
                # lpd_edge_split_bwd is built for C in {64, 128, 256}: B clouds of 4096 points
                + [("edge_split_bwd", 64, 25 * 4096), ("edge_split_bwd", 128, 13 * 4096), ("edge_split_bwd", 256, 7 * 4096)])
# the same operators at small sizes, run under LPD_DEBUG=reduce-grid=7 (long grid-stride loops) and under the default cap
REDUCE_SMALL_CAP = 7
REDUCE_SMALL_CASES = [("colstats", 64, 5000), ("colstats", 1024, 1000), ("bn_act_bwd", 128, 3001), ("bn_act_bwd", 1024, 999),
                      ("bn_act_bwd_bf16", 64, 6000), ("bn_act_bwd_bf16", 2048, 600), ("bn_sel_bwd_reduce", 128, 3001),
                      ("bn_sel_bwd_reduce", 1024, 701), ("edge_split_bwd", 64, 3 * 1024), ("edge_split_bwd", 256, 2 * 1024)]

# ---- the BatchNorm-backward products (E = M k rows of 32-row tiles): blocks = ceil(tiles / tiles per block), capped
BNBWD = {"f32": (8, 256), "bf16": (4, 512)}      # (tiles per block, block cap)
BNBWD_SHAPE = dict(M=30000, k=16)                 # E = 480 000 rows = 15 000 tiles: 7.3 / 7.3 strides, the last one part-filled


def bnbwd_launch(mode, M, k):
    tpb, cap = BNBWD[mode]
    tiles = (M * k + 31) // 32
    wanted = (tiles + tpb - 1) // tpb
    grid = min(wanted, cap)
    return wanted, grid, tiles % grid != 0


# ---- the training-path kernels of csrc/lpd_train.hip: grid_for caps every launch at GRID_CAP blocks and walks a grid-stride loop beyond
GRID_CAP = 4096
ACT_BLOCK = 4         # waves per block of the wave-per-point / wave-per-row kernels (edge_build, gather_sum_rows)


def chain_launch(kernel, M, C):
    """(blocks wanted, blocks launched, items, items per block and trip) of one launch of the materialised edge chain over M points of
    C channels (C in 64 / 128 / 256); the grid-stride walk takes items / (launched * per trip) trips"""
    q = C // 4
    rg = 256 // q                          # rows per block and trip of the edge_bn_bwd kernels
    if kernel == "edge_build":             # 64 / (C / 4) points per wave
        items, per_block, per_trip = M, ACT_BLOCK * (64 // q), ACT_BLOCK * (64 // q)
    elif kernel in ("group_max", "group_sum"):      # one thread per (point, column quad)
        items, per_block, per_trip = M * q, 256, 256
    elif kernel == "edge_bn_bwd_reduce":   # grid_for(M, 2 RG): two trips per block by design
        items, per_block, per_trip = M, 2 * rg, rg
    elif kernel == "edge_bn_bwd_apply":
        items, per_block, per_trip = M, rg, rg
    elif kernel == "gather_sum_rows":      # 256 / C rows per wave
        items, per_block, per_trip = M, ACT_BLOCK * (256 // C), ACT_BLOCK * (256 // C)
    else:
        raise KeyError(kernel)
    wanted = (items + per_block - 1) // per_block
    return wanted, grid_for(items, per_block, GRID_CAP), items, per_trip


CHAIN_KERNELS = ("edge_build", "group_max", "group_sum", "edge_bn_bwd_reduce", "edge_bn_bwd_apply", "gather_sum_rows")
# (B, N, k, C): the lpdnetorigin step (M = 180 224 points, E = 3 604 480 edge rows) and two wider layers; every kernel of the chain,
# the edge_bn_bwd reduction included, launches at the cap with a part-filled last trip (B = 5 at C = 256 would not: 2560 blocks)
CHAIN_SHAPES = {"c64": (44, 4096, 20, 64), "c128": (17, 4096, 20, 128), "c256": (9, 4096, 20, 256)}


def vlad_bwd_slices(B, F, KC=64):
    """slices per cloud of lpd_vlad_finalize_bwd; 0 = the one-block-per-cloud kernel with atomic dcw2"""
    G = 8
    while G > 1 and B * G * (1 + 2 * KC) > F * KC:
        G >>= 1
    if B * G * (1 + 2 * KC) <= F * KC and F >= 8 * G and B <= 65535:
        return G
    return 0


# (B, F) -> slices: every regime at F = 1024, and F < 8 G at one cloud
VLAD_BWD_CASES = {(44, 1024): 8, (66, 1024): 4, (130, 1024): 2, (300, 1024): 1, (520, 1024): 0, (1, 32): 0}


def graph_transpose_path(N):
    """lpd_graph_transpose: one LDS-atomic kernel for N <= 32768, else global-atomic count, scan and fill"""
    return "lds" if N <= 32768 else "global"


# name -> (B, N, k, path)
GRAPH_CASES = {"global": (2, 40000, 20, "global"), "train": (44, 4096, 20, "lds"), "stress": (2, 16384, 64, "lds")}


def dw_smallk_launch(M, Co):
    """(grid, stride, rows of the four-row unrolled loop per thread are whole: no tail) of lpd_dw_smallk"""
    rg = 256 // Co
    grid = grid_for(M, rg * 64, GRID_CAP)
    step = grid * rg
    return grid, step, M % (4 * step) == 0


DW_SMALLK_ROWS = {"exact": 180_224, "tail": 175_001}


# ---- tests/test_fwd_ops_gpu.py: the forward head, BatchNorm apply, mining and loss kernels
def affine_act_launch(R, C):
    """(blocks wanted, blocks launched, fixed_q) of lpd_affine_act / lpd_affine_act2: one float4 per thread and trip, four trips per
    block by design; fixed_q = the grid stride is a multiple of the C / 4 column quads, so a thread loads scale / shift once"""
    q = C // 4
    items = R * q
    wanted = (items + 1023) // 1024
    grid = grid_for(items, 1024, GRID_CAP)
    return wanted, grid, (grid * 256) % q == 0


# name -> (R, C, capped, fixed_q)
FWD_AFFINE_SHAPES = {
    "small": (3000, 64, False, True),
    "capped_pow2": (20001, 1024, True, True),
    "capped_reload": (420000, 40, True, False),
    "reload": (5461, 12, False, False),
    "c2048_odd_grid": (150, 2048, False, False),
}


def vlad_asum_chunks(N):
    """blocks per cloud of vlad_asum_kernel (lpd_vlad_finalize without a ready a_sum)"""
    return 16 if N >= 1024 else (N + 63) // 64


# N -> (chunks, rows of the last chunk, blocks that get no row at all)
def vlad_asum_split(N):
    g = vlad_asum_chunks(N)
    chunk = (N + g - 1) // g
    full = (N + chunk - 1) // chunk          # chunks that own at least one row
    return g, N - (full - 1) * chunk, g - full


FWD_VLAD_N = {63: "per64", 64: "per64", 65: "per64", 1023: "per64", 1024: "chunk16", 1030: "chunk16", 4096: "chunk16"}
FWD_VLAD_CASES = [(63, 96), (64, 1000), (65, 1024), (1023, 1000), (1024, 96), (1030, 1024), (4096, 1024), (4096, 1000)]     # (N, F), B = 44


def softmax_kernel(ncols, group_rows, aligned, parts=None):
    """which kernel lpd_softmax_affine / lpd_softmax_affine_parts launches; group_rows None = no column sums"""
    if parts is not None:
        if parts not in (1, 2, 4, 8) or ncols != 64 or group_rows is None or group_rows % 64 or not aligned:
            raise ValueError("lpd_softmax_affine_parts refuses")
        return f"colsum64<{parts}>"
    if ncols < 1 or ncols > 64:
        raise ValueError("ncols")
    if group_rows is None:
        return "rows"
    if group_rows % 16:
        raise ValueError("group_rows % 16")
    return "colsum64<1>" if (ncols == 64 and group_rows % 64 == 0 and aligned) else "colsum"


# (ncols, colsum_rows, aligned) -> kernel
FWD_SOFTMAX_CASES = {(64, None, True): "rows", (40, None, True): "rows", (1, None, True): "rows",
                     (64, 4096, True): "colsum64<1>", (64, 4096, False): "colsum", (40, 4096, True): "colsum", (1, 4096, True): "colsum",
                     (64, 208, True): "colsum"}
FWD_SOFTMAX_ROWS = (32 * 4096, 44 * 4096)


def gating_loops(D):
    """(column tiles of 256, k per quarter, the 8-unrolled loop leaves a tail in some quarter, trips of the hrow fill) of gating_kernel"""
    kper = (D + 3) // 4
    tail = any((min(kq * kper + kper, D) - kq * kper) % 8 for kq in range(4) if kq * kper < D)
    return (D + 255) // 256, kper, tail, (D + 1023) // 1024


# D -> (tiles, kper, tail, fill trips)
FWD_GATING_D = {256: (1, 64, False, 1), 300: (2, 75, True, 1), 1100: (5, 275, True, 2), 2048: (8, 512, False, 2)}
FWD_GATING_CASES = [(1, 256), (44, 256), (128, 256), (44, 300), (128, 300), (1, 1100), (44, 1100), (44, 2048)]     # (B, D)
GATING_DMAX = 8192


HARD_NEG_NC_MAX = 36864


def hard_negatives_lds_bytes(nc):
    """dynamic LDS of hard_negatives_kernel (one fp32 distance per candidate); None = refused by the host check"""
    return 4 * nc if 0 < nc <= HARD_NEG_NC_MAX else None


METRIC_LOSS_LDS_MAX = 60 * 1024


def metric_loss_lds_bytes(bq, P, Ng):
    """dynamic LDS of metric_loss_kernel: dpos [bq][P], dneg and d2 [bq][Ng], t1 and t2 [bq], two weights, four reduction slots"""
    return 4 * (bq * (P + 2 * Ng) + 2 * bq + 2 + 4)


# (bq, P, Ng): the largest launch the guard lets through at bq = 8, P = 2, and the first one it refuses
METRIC_LOSS_FITS = (8, 2, 957)
METRIC_LOSS_REFUSED = (8, 2, 958)


def quad_launch(kernel, M, C):
    """(blocks wanted, blocks launched) of group_max_bwd (one thread per point and column quad) / scatter_add_rows (one wave per point)"""
    if kernel == "group_max_bwd":
        items, per_block = M * (C // 4), 256
    elif kernel == "scatter_add_rows":
        items, per_block = M, ACT_BLOCK
    else:
        raise KeyError(kernel)
    return (items + per_block - 1) // per_block, grid_for(items, per_block, GRID_CAP)


# (M, C, k) -> capped
FWD_GROUP_MAX_BWD = {(70001, 64, 20): True, (3000, 256, 7): False}
