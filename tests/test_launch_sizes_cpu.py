"""The shapes of tests/test_launch_sizes_gpu.py reach the launch regimes they are there for (tests/launch_sizes.py restates the
launch arithmetic of csrc/).  No GPU needed: if a heuristic changes, this names the cases that stop covering what they claim."""
import pytest

import launch_sizes as ls


@pytest.mark.parametrize("name", sorted(ls.EDGE_SHAPES))
def test_edge_mlp_shapes_reach_the_tile_loop(name):
    s = ls.EDGE_SHAPES[name]
    M = s["B"] * s["N"]
    assert M % 32 == 0 and s["N"] % 64 == 0 and s["k"] >= 16            # the backward and its gather pass
    for form, want in ls.EDGE_REGIMES[name].items():
        t, grid, last = ls.edge_launch(name, form)
        assert (t, grid, last) == want, (form, (t, grid, last))
        assert t > 1 and 0 < last < t                                    # a tile loop whose last block runs short
        assert ls.edge_launch(name, form, tmax=1)[0] == 1                # LPD_DEBUG=edge-mlp-tiles=1 turns it off
    assert ls.edge_launch("t16", "bwd")[0] == ls.EM_TMAX and ls.edge_launch("t16", "bwd")[1] > ls.EM_ROUND   # the cap, past one round


def test_em_tiles_per_block_mirror():
    assert [ls.em_tiles_per_block(t) for t in (1, 256, 512, 513, 1024, 1025, 4096, 8192, 8193, 10 ** 6)] == [1, 1, 1, 2, 2, 3, 8, 16, 16, 16]
    assert ls.em_launch(32 * 4096, 32) == (8, 512, 8)                   # B = 32 x 4096 at 32-point tiles: divides exactly
    assert ls.em_launch(2 * 4096, 32) == (1, 256, 1)                    # the op tests' largest size (B = 2, N = 4096): no loop


@pytest.mark.parametrize("op,C,R", ls.REDUCE_CASES)
def test_reduction_shapes_pass_the_grid_cap(op, C, R):
    for name, items, per_block, gcap in ls.reduce_launches(op, C, R):
        wanted, grid, ragged = ls.capped_launch(items, per_block, ls.REDUCE_CAP, gcap)
        assert grid == ls.REDUCE_CAP and wanted > ls.REDUCE_CAP and ragged, (name, wanted, grid, ragged)


@pytest.mark.parametrize("op,C,R", ls.REDUCE_SMALL_CASES)
def test_small_reduction_shapes_stride_under_the_debug_cap(op, C, R):
    for name, items, per_block, gcap in ls.reduce_launches(op, C, R):
        wanted, grid, ragged = ls.capped_launch(items, per_block, ls.REDUCE_SMALL_CAP, gcap)
        assert grid == ls.REDUCE_SMALL_CAP and wanted >= 3 * ls.REDUCE_SMALL_CAP and ragged, (name, wanted, grid, ragged)
        assert ls.capped_launch(items, per_block, ls.REDUCE_CAP, gcap)[1] < ls.REDUCE_CAP      # the default cap launches them whole


@pytest.mark.parametrize("mode", sorted(ls.BNBWD))
def test_bnbwd_product_shape_passes_its_cap(mode):
    wanted, grid, ragged = ls.bnbwd_launch(mode, **ls.BNBWD_SHAPE)
    tpb, cap = ls.BNBWD[mode]
    assert grid == cap and ls.BNBWD_SHAPE["M"] * ls.BNBWD_SHAPE["k"] > 4 * cap * tpb * 32 and ragged
    assert (ls.BNBWD_SHAPE["M"] * ls.BNBWD_SHAPE["k"]) % 32 == 0


# ---- tests/test_train_bwd_ops_gpu.py: the training-path kernels of csrc/lpd_train.hip
def test_grid_for_mirror():
    assert [ls.grid_for(n, 256) for n in (1, 256, 257, 4096 * 256, 4096 * 256 + 1, 10 ** 9)] == [1, 1, 2, 4096, 4096, 4096]
    assert ls.chain_launch("group_max", 2 * 4096, 64)[:2] == (512, 512)         # the op tests' largest size (B = 2): one partial trip


@pytest.mark.parametrize("name", sorted(ls.CHAIN_SHAPES))
def test_edge_chain_shapes_pass_the_grid_cap(name):
    B, N, k, C = ls.CHAIN_SHAPES[name]
    assert N <= 32768 and C in (64, 128, 256)
    for kernel in ls.CHAIN_KERNELS:
        wanted, grid, items, per_trip = ls.chain_launch(kernel, B * N, C)
        assert grid == ls.GRID_CAP and wanted > ls.GRID_CAP, (kernel, wanted)
        assert items > 2 * grid * per_trip and items % (grid * per_trip) != 0, (kernel, items / (grid * per_trip))   # > 2 trips, the last part-filled
    if name == "c64":
        assert (B, N, k) == (44, 4096, 20)                                          # the lpdnetorigin training step
    assert ls.chain_launch("edge_bn_bwd_reduce", 5 * 4096, 256)[0] < ls.GRID_CAP   # why C = 256 needs B = 9


@pytest.mark.parametrize("B,F", sorted(ls.VLAD_BWD_CASES))
def test_vlad_finalize_bwd_cases_reach_their_regime(B, F):
    G = ls.vlad_bwd_slices(B, F)
    assert G == ls.VLAD_BWD_CASES[(B, F)]
    if G:
        assert G == 1 or ls.vlad_bwd_slices(B - 1, F) == G                          # inside the regime, not on its lower edge only
    else:
        assert B * 129 > F * 64 or F < 64                                            # the fallback: too many clouds, or F < 8 G
    assert sorted(set(ls.VLAD_BWD_CASES.values())) == [0, 1, 2, 4, 8]                # every regime has a case


@pytest.mark.parametrize("name", sorted(ls.GRAPH_CASES))
def test_graph_transpose_cases_take_their_path(name):
    B, N, k, path = ls.GRAPH_CASES[name]
    assert ls.graph_transpose_path(N) == path and B >= 2                             # B >= 2: a cloud's base offset is exercised
    assert B * N * k < 2 ** 31
    assert {p for _, _, _, p in ls.GRAPH_CASES.values()} == {"lds", "global"}


@pytest.mark.parametrize("Co", [64, 128, 256])
def test_dw_smallk_rows_reach_both_loops(Co):
    grid, step, whole = ls.dw_smallk_launch(ls.DW_SMALLK_ROWS["exact"], Co)
    assert whole and ls.DW_SMALLK_ROWS["exact"] // step >= 16                       # the unrolled loop only
    if Co == 64:
        assert (grid, step) == (704, 2816)
    grid, step, whole = ls.dw_smallk_launch(ls.DW_SMALLK_ROWS["tail"], Co)
    assert not whole and ls.DW_SMALLK_ROWS["tail"] // step >= 16                     # the unrolled loop and the tail


# ---- tests/test_fwd_ops_gpu.py: the forward head, BatchNorm apply, mining and loss kernels
@pytest.mark.parametrize("name", sorted(ls.FWD_AFFINE_SHAPES))
def test_affine_act_shapes_reach_their_regime(name):
    R, C, capped, fixed = ls.FWD_AFFINE_SHAPES[name]
    wanted, grid, fixed_q = ls.affine_act_launch(R, C)
    assert C % 4 == 0 and (wanted > ls.GRID_CAP) == capped and (grid == ls.GRID_CAP) == capped and fixed_q == fixed, (wanted, grid, fixed_q)
    if capped:
        assert (R * (C // 4)) % (grid * 256) != 0                                    # the last grid stride is part-filled
    if name == "c2048_odd_grid":
        assert C == 2048 and grid % 2 == 1
    if name == "reload":
        assert (C // 4) & (C // 4 - 1)                                               # C / 4 is not a power of two


def test_affine_act_launch_mirror():
    assert ls.affine_act_launch(32 * 4096, 256) == (8192, 4096, True)               # B = 32, N = 4096: C >= 256 walks the grid-stride loop
    assert ls.affine_act_launch(32 * 4096, 128)[:2] == (4096, 4096) and ls.affine_act_launch(32 * 4096, 64)[0] == 2048
    # every width of the form 4 * 2^n <= 1024 keeps its column quad; 2048 does with an even grid only
    assert all(ls.affine_act_launch(R, C)[2] for C in (4, 8, 64, 256, 1024) for R in (1, 77, 5000))
    assert ls.affine_act_launch(152, 2048)[1:] == (76, True)


@pytest.mark.parametrize("N", sorted(ls.FWD_VLAD_N))
def test_vlad_asum_cases_reach_their_regime(N):
    g, last, idle = ls.vlad_asum_split(N)
    assert ("chunk16" if g == 16 and N >= 1024 else "per64") == ls.FWD_VLAD_N[N]
    assert 0 < last and idle >= 0
    want = {63: (1, 63, 0), 64: (1, 64, 0), 65: (2, 32, 0), 1023: (16, 63, 0), 1024: (16, 64, 0), 1030: (16, 55, 0), 4096: (16, 256, 0)}
    assert (g, last, idle) == want[N]
    assert {N for N, _ in ls.FWD_VLAD_CASES} == set(ls.FWD_VLAD_N) and {F for _, F in ls.FWD_VLAD_CASES} == {96, 1000, 1024}
    assert any(F % 64 for _, F in ls.FWD_VLAD_CASES)                                  # a short last feature block of the residual pass


@pytest.mark.parametrize("case", sorted(ls.FWD_SOFTMAX_CASES, key=str))
def test_softmax_cases_pick_their_kernel(case):
    assert ls.softmax_kernel(*case) == ls.FWD_SOFTMAX_CASES[case]
    assert set(ls.FWD_SOFTMAX_CASES.values()) == {"rows", "colsum", "colsum64<1>"}
    assert all(r % 4096 == 0 for r in ls.FWD_SOFTMAX_ROWS)
    assert [ls.softmax_kernel(64, 320, True, parts=p) for p in (1, 2, 4, 8)] == ["colsum64<1>", "colsum64<2>", "colsum64<4>", "colsum64<8>"]
    with pytest.raises(ValueError):
        ls.softmax_kernel(64, 320, True, parts=3)


@pytest.mark.parametrize("D", sorted(ls.FWD_GATING_D))
def test_gating_sizes_reach_their_loops(D):
    assert ls.gating_loops(D) == ls.FWD_GATING_D[D]
    assert {d for _, d in ls.FWD_GATING_CASES} == set(ls.FWD_GATING_D) and {b for b, _ in ls.FWD_GATING_CASES} == {1, 44, 128}
    rows = list(ls.FWD_GATING_D.values())
    assert any(t > 1 for t, _, _, _ in rows) and any(tail for _, _, tail, _ in rows) and any(f > 1 for _, _, _, f in rows)
    assert any(D % 256 for D in ls.FWD_GATING_D)                                      # a part-filled last column tile
    assert ls.gating_loops(ls.GATING_DMAX)[3] == 8


def test_lds_guards():
    assert ls.hard_negatives_lds_bytes(4000) == 16000 and ls.hard_negatives_lds_bytes(ls.HARD_NEG_NC_MAX) == 144 * 1024
    assert ls.hard_negatives_lds_bytes(ls.HARD_NEG_NC_MAX + 1) is None
    assert ls.hard_negatives_lds_bytes(4000) < 64 * 1024 < ls.hard_negatives_lds_bytes(ls.HARD_NEG_NC_MAX) <= 160 * 1024 - 64   # past the default limit, inside the CU's LDS
    assert ls.metric_loss_lds_bytes(*ls.METRIC_LOSS_FITS) <= ls.METRIC_LOSS_LDS_MAX < ls.metric_loss_lds_bytes(*ls.METRIC_LOSS_REFUSED)
    assert ls.METRIC_LOSS_REFUSED[2] == ls.METRIC_LOSS_FITS[2] + 1
    assert ls.metric_loss_lds_bytes(2, 2, 18) == 4 * (2 * 38 + 4 + 6)


@pytest.mark.parametrize("case", sorted(ls.FWD_GROUP_MAX_BWD))
def test_group_max_bwd_cases_sit_on_both_sides_of_the_cap(case):
    M, C, k = case
    wanted, grid = ls.quad_launch("group_max_bwd", M, C)
    assert (wanted > ls.GRID_CAP) == ls.FWD_GROUP_MAX_BWD[case] and grid == min(wanted, ls.GRID_CAP)
    if wanted > ls.GRID_CAP:
        assert (M * (C // 4)) % (grid * 256) != 0
    assert sorted(ls.FWD_GROUP_MAX_BWD.values()) == [False, True]
    assert ls.quad_launch("scatter_add_rows", 20000, 64) == (5000, 4096)             # the size a scatter_add_rows case would need
