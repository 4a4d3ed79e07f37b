"""The two layers of GEMM dispatch, restated in Python, and the table of cases at which tests/test_gemm_routes_gpu.py runs every route.

Layer 1 (lpdnet_hip/ops.py): ops.gemm, ops._gemm_panels, ops.linear, ops.gemm_p8, ops.gemm_x3t_split, ops.linear_bn_stats, ops.gemm_act and
ops.gemm_bf16a choose an entry point and an ops.PROFILE label:
    gemm[..] lpd_gemm                 gemmx3[..] lpd_gemm_bf16x3       gemmx1[..] lpd_gemm_bf16x1
    gemmx3w[..] / gemmx1w[..] lpd_gemm_x3w (three / one product)       gemmx3w[..]xB lpd_gemm_x3w_batched
    gemmx3w+stats[..] lpd_gemm_x3w_stats    gemmx3w+act[..] lpd_gemm_x3w_act    gemmx2w[..] lpd_gemm_x3w_bf16a
    gemmx3t[..] lpd_gemm_x3t / lpd_gemm_x3ts / lpd_gemm_x3t_rows (batched: ..xB)
    gemm_p8[..] lpd_gemm_p8           gemm_p8+assign[..] lpd_gemm_p8_fused
Layer 2 (csrc/lpd_gemm.hip gemm_entry / gemm_x3w_impl, csrc/lpd_gemm_t.hip, csrc/lpd_gemm_p8.hip gemm_p8_impl) chooses a kernel and its
template arguments.  Instances are written as the sources order the arguments, booleans as 0 / 1:
    f32<AK,BK,TN,KTAIL,PANELS>   gemm_f32_kernel          x3<AK,BK,TN,KTAIL,PANELS>   gemm_bf16x3_kernel (one- and three-product: g.prods)
    fewrows<MT>  rows32  smallm<RG>                       linear_fewrows_kernel / linear_rows32_kernel / linear_smallm_kernel
    ..+red1 / ..+red2                                     split-K: gemm_splitk_reduce_kernel once / twice (groups of 16 slabs first)
    x3w<WN,KTAIL,PANELS,KC,TALL,MODE>                     gemm_x3w_wide_kernel
    x3t<KS,ROWS,RB>                                       gemm_x3t_kernel
    p8<D,CPANELS,FUSE>                                    gemm_p8_kernel<D, CPANELS, 0, FUSE>
route(case) resolves a case through both layers with every LPD_DEBUG switch at its default (all on) except those the case sets.
CASES is the table; BUILT lists every instance the sources build, each `reached by <case>` or `not reachable through a wrapper` with
the wrapper condition that excludes it.  tests/test_gemm_routes_cpu.py holds the two together and compares the constants below with the
constexpr values of the sources.
"""
import zlib

# ---- constants of the sources (tests/test_gemm_routes_cpu.py reads them from the .hip files)
GEMM_BK = 32          # k-tile of the generic kernels
SMALLM_KC = 128       # per-split depth of linear_smallm_kernel
FR_KPER = 256         # k-rows per block of linear_fewrows_kernel
R32_KPER = 256        # ... of linear_rows32_kernel
FR_MAXM = 4           # most rows of the weight-stream form
X3T_ROWS_PER_WG = 128  # XT_THREADS / 2: rows of a gemm_x3t workgroup (RB default)
X3T_RB_BF16 = 64      # RB of the bf16-C instance at K = 128
# ---- constants of the wrappers (lpdnet_hip/ops.py)
X3W_MIN_M = 1024
X3_MIN = 128          # split form: M >= 128 and N >= 128 (64 for the batched both-k-major product)
ROWS_MIN = 16384      # nb * M floor of lpd_gemm_x3t_rows and lpd_gemm_x3w_batched
NK_MAX = 1 << 22
STAT_CMAX = 1024

NONE, RELU, LEAKY, SIGMOID = 0, 1, 2, 3


def cdiv(a, b):
    return (a + b - 1) // b


# ================================================================== layer 2: entry points -> kernel instances
def reduce_stage(batch, splits):
    if splits <= 1:
        return ""
    return "+red2" if (batch == 1 and splits >= 64 and splits % 16 == 0) else "+red1"


def entry_generic(mode, M, N, K, ak, bk, batch=1, splits=1, panels=0):
    """gemm_entry: mode 0 = f32-input MFMA, 3 / 1 = split bf16 (three / one product)"""
    kern = "x3" if mode else "f32"
    if panels:
        assert not ak and batch == 1 and splits == 1 and K % 32 == 0
        return f"{kern}<0,{int(bk)},2,0,{panels}>"
    per = cdiv(cdiv(K, splits), GEMM_BK) * GEMM_BK
    stream = splits > 1 and not mode and not ak and bk and batch == 1
    if stream and M <= FR_MAXM and N % 256 == 0 and K >= 8192 and cdiv(K, FR_KPER) <= splits:
        return f"fewrows<{1 if M <= 1 else 2 if M <= 2 else 4}>" + reduce_stage(batch, cdiv(K, FR_KPER))
    if stream and FR_MAXM < M <= 32 and N % 256 == 0 and K >= 8192 and cdiv(K, R32_KPER) <= splits:
        return "rows32" + reduce_stage(batch, cdiv(K, R32_KPER))
    if stream and M <= 64 and per == SMALLM_KC:
        return f"smallm<{min(cdiv(M, 16), 4)}>" + reduce_stage(batch, splits)
    tn = 2 if N > 64 else 1
    ktail = K % GEMM_BK != 0 or per * splits != K
    return f"{kern}<{int(ak)},{int(bk)},{tn},{int(ktail)},0>" + reduce_stage(batch, splits)


def entry_x3w(N, K, panels=0, impl=0, a16=False, c16=False, a_affine=False):
    """gemm_x3w_impl: the prepared-fragment kernel.  None: the combination is refused (LPD_CHECK_ARG)"""
    if a_affine:
        if N > 128 or impl == 3 or panels & 1:
            return None
        impl = 2
    if impl == 0:
        impl = 3 if N >= 256 else 2
    nt = cdiv(N, 32)
    if a16 or c16:
        if K % 32 or panels:
            return None
        mode = (1 if a16 else 0) | (2 if c16 else 0) | (4 if (a16 and a_affine) else 0)
        if mode in (2, 3, 1) and impl == 3:
            return f"x3w<2,0,0,32,0,{mode}>"
        if mode in (1, 5) and impl == 2:
            return f"x3w<1,0,0,32,{int(nt <= 2)},{mode}>"
        return None
    wn = 1 if impl == 2 else 2
    tall = wn == 1 and nt <= 2
    return f"x3w<{wn},{int(K % 32 != 0)},{panels},32,{int(tall)},0>"


def x3w_prods(fast, a16, a_affine, map16):
    """products per term of the prepared-fragment kernel: 1 (single product), 2 (bf16 rows: no lo image of A), 3"""
    if fast:
        return 1
    return 2 if (a16 and (not a_affine or map16)) else 3


def entry_x3t(K, rows, c16=False):
    assert K in (64, 128)
    rb = X3T_RB_BF16 if (rows and K == 128 and c16) else X3T_ROWS_PER_WG
    return f"x3t<{K // 16},{int(rows)},{rb}>"


def x3t_applies(M, N, K, act, panel_n=None):
    ok = K in (64, 128) and N > 0 and N % 32 == 0 and M > 0 and M % 128 == 0 and 0 <= act <= 2
    return ok and (panel_n is None or (panel_n % 128 == 0 and M % panel_n == 0))


def entry_p8(impl, c_panels, fused):
    if fused:
        return f"p8<6,{int(c_panels)},1>"
    assert impl in (0, 5, 6)
    return f"p8<{5 if impl == 5 else 6},{int(c_panels)},0>"


def p8_applies(M, N, K, panel_n):
    return M > 0 and N > 0 and K >= 64 and N % 256 == 0 and K % 32 == 0 and panel_n % 256 == 0 and M % panel_n == 0


# ================================================================== layer 1: wrappers -> (PROFILE label, instance)
def _modes(c):
    exact, fast = c["mode"] == "f32", c["mode"] == "x1"
    return exact, fast


def route_gemm(c):
    """ops.gemm (row-major operands) and, through it, ops.linear"""
    M, N, K, nb, ak, bk = c["M"], c["N"], c["K"], c["nb"], c["ak"], c["bk"]
    exact, fast = _modes(c)
    splits, acc = c["splits"], c["accumulate"]
    batched = c["batched"]
    a16, c16, aff = c["a16"], c["c16"], c["a_affine"]
    act = NONE if aff else c["act"]          # with a_affine the case's activation is the operand transform's, the epilogue has none
    shp = f"[{M}x{N}x{K}]"
    epi = c["epi"]
    if (not exact and (not fast or c16) and not ak and splits == 1 and not a16 and not aff and not acc and nb * M >= ROWS_MIN
            and x3t_applies(M, N, K, act)):
        return "gemmx3t" + shp + (f"x{nb}" if batched else ""), entry_x3t(K, True, c16)
    if c16:
        return None
    if (batched and not exact and not ak and bk and splits == 1 and not acc and not epi and act == NONE and M % 128 == 0 and nb * M >= ROWS_MIN
            and 64 <= N <= 128 and K >= 256 and N * K <= NK_MAX and (not a16 or K % 32 == 0)):
        return f"gemmx3w{shp}x{nb}", entry_x3w(N, K, a16=a16, a_affine=aff)
    if aff or a16:
        return None
    if (not exact and not ak and not batched and splits == 1 and M >= X3W_MIN_M and N >= 64 and N * K <= NK_MAX
            and ((bk and K >= 128) or K >= 256)):
        return f"gemmx{'1' if fast else '3'}w{shp}", entry_x3w(N, K, impl=c["x3w_impl"])
    x3 = not exact and M >= X3_MIN and (not ak or bk) and N >= (64 if (batched and ak and bk) else X3_MIN)
    mode = (1 if fast else 3) if x3 else 0
    label = "gemm" + (("x1" if fast else "x3") if x3 else "") + shp
    return label, entry_generic(mode, M, N, K, ak, bk, nb, splits)


def route_linear(c):
    """ops.linear: torch weight layout, K > 8; splits None = K // 128 for M <= 128 and K >= 512"""
    assert c["K"] > 8 and not c["ak"] and not c["bk"]
    d = dict(c)
    if d["splits"] is None:
        d["splits"] = c["K"] // 128 if (c["M"] <= 128 and c["K"] >= 512) else 1
    return route_gemm(d)


def route_panels(c):
    """ops._gemm_panels: cloud-panel A and / or C"""
    M, N, K, bk = c["M"], c["N"], c["K"], c["bk"]
    exact, fast = _modes(c)
    pa, pc = c["panels"]["a"], c["panels"]["c"]
    Np = c["panels"]["Np"]
    assert K % 32 == 0 and Np % 128 == 0 and not c["ak"]
    pm = (1 if pa else 0) | (2 if pc else 0)
    shp = f"[{M}x{N}x{K}]"
    x3 = not exact and N >= 128 and M >= 128
    if x3 and c["x3t_panels"] and not c["accumulate"] and M >= 1024 and pa and pc and x3t_applies(M, N, K, c["act"], Np):
        return "gemmx3t" + shp, entry_x3t(K, False)
    if x3 and M >= X3W_MIN_M and K >= 256 and N * K <= NK_MAX:
        return "gemmx3w" + shp, entry_x3w(N, K, panels=pm, impl=c["x3w_impl"])
    return "gemm" + ("x3" if x3 else "") + shp, entry_generic(3 if x3 else 0, M, N, K, False, bk, panels=pm)


def route_p8(c):
    M, N, K = c["M"], c["N"], c["K"]
    if not p8_applies(M, N, K, c["panels"]["Np"]):
        return None
    fused = c["assign"]
    return ("gemm_p8+assign" if fused else "gemm_p8") + f"[{M}x{N}x{K}]", entry_p8(c["p8_impl"], c["panels"]["c"], fused)


def route_x3t_split(c):
    M, N, K = c["M"], c["N"], c["K"]
    if not x3t_applies(M, N, K, NONE, c["panels"]["Np"]):
        return None
    return f"gemmx3t[{M}x{N}x{K}]", entry_x3t(K, False)


def route_bn_stats(c):
    M, N, K = c["M"], c["N"], c["K"]
    a16, c16 = c["a16"], c["c16"]
    fused = (M >= X3W_MIN_M and 64 <= N <= STAT_CMAX and K >= 128 and N * K <= NK_MAX and (K >= 256 or N >= 128)
             and (not c16 or N % 32 == 0) and (not a16 or (N >= 256 and K % 32 == 0)))
    if not fused or (a16 and not c16):
        return None
    return f"gemmx3w+stats[{M}x{N}x{K}]", entry_x3w(N, K, impl=c["x3w_impl"], a16=a16, c16=c16)


def route_gemm_act(c):
    M, N, K = c["M"], c["N"], c["K"]
    if not (M >= X3W_MIN_M and 64 <= N <= 128 and K >= 256 and N * K <= NK_MAX) or (c["a16"] and K % 32):
        return None
    if c["map16"] and not c["a16"]:
        return None                      # a bf16 map is built for bf16 rows only
    return f"gemmx3w+act[{M}x{N}x{K}]", entry_x3w(N, K, a16=c["a16"], a_affine=True)


def route_bf16a(c):
    M, N, K = c["M"], c["N"], c["K"]
    if K % 32 or N * K > NK_MAX:
        return None
    return f"gemmx2w[{M}x{N}x{K}]", entry_x3w(N, K, impl=c["x3w_impl"], a16=True)


ROUTES = {"gemm": route_gemm, "linear": route_linear, "panels": route_panels, "p8": route_p8, "x3t_split": route_x3t_split,
          "bn_stats": route_bn_stats, "gemm_act": route_gemm_act, "bf16a": route_bf16a}


def route(c):
    return ROUTES[c["wrapper"]](c)


# ================================================================== the cases
CASES = []


def case(name, wrapper, M, N, K, label, inst, **kw):
    c = dict(name=name, wrapper=wrapper, M=M, N=N, K=K, label=label, inst=inst, nb=1, batched=False, ak=False, bk=True, mode="x3", splits=1,
             act=NONE, epi=True, accumulate=False, slice=False, a16=False, c16=False, a_affine=False, map16=False, store=True,
             x3w_impl=0, p8_impl=0, x3t_panels=True, assign=False, panels=None, split_in=False)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    if c["nb"] > 1:
        c["batched"] = True
    c["seed"] = zlib.crc32(name.encode())
    assert name not in {x["name"] for x in CASES}, name
    CASES.append(c)
    return c


def by_name(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


_L = {(False, False): "nn", (False, True): "nt", (True, False): "tn", (True, True): "tt"}      # (a_kmajor, b_kmajor)
_ACTS = (NONE, RELU, LEAKY, SIGMOID)

# ---- generic f32-input kernel (exact=True): every (AK, BK, TN, KTAIL), M = 130 (the second row tile holds two rows)
_i = 0
for (ak, bk), l in _L.items():
    for N in (40, 136):
        for K in (64, 52):
            case(f"f32/{l}_N{N}_K{K}", "gemm", 130, N, K, f"gemm[130x{N}x{K}]", f"f32<{int(ak)},{int(bk)},{1 if N == 40 else 2},{int(K == 52)},0>",
                 ak=ak, bk=bk, mode="f32", act=_ACTS[_i % 4])
            _i += 1
    # K = 37: the operand rows are padded to the next multiple of 4 (ld 40 / 132), the k tail ends inside a float4
    case(f"f32/{l}_N40_K37", "gemm", 130, 40, 37, "gemm[130x40x37]", f"f32<{int(ak)},{int(bk)},1,1,0>", ak=ak, bk=bk, mode="f32", act=LEAKY)
case("f32/nt_M1_N40_K64", "gemm", 1, 40, 64, "gemm[1x40x64]", "f32<0,1,1,0,0>", mode="f32", act=RELU)
case("f32/nn_M1_N136_K52", "gemm", 1, 136, 52, "gemm[1x136x52]", "f32<0,0,2,1,0>", bk=False, mode="f32", act=SIGMOID)
case("f32/nt_batch3", "gemm", 130, 40, 52, "gemm[130x40x52]", "f32<0,1,1,1,0>", nb=3, mode="f32", act=LEAKY, slice=True)
case("f32/tt_batch3", "gemm", 130, 136, 64, "gemm[130x136x64]", "f32<1,1,2,0,0>", nb=3, ak=True, mode="f32", act=RELU)
case("f32/nn_slice", "gemm", 130, 136, 64, "gemm[130x136x64]", "f32<0,0,2,0,0>", bk=False, mode="f32", act=LEAKY, slice=True)
case("f32/nt_accumulate", "gemm", 130, 40, 64, "gemm[130x40x64]", "f32<0,1,1,0,0>", mode="f32", act=LEAKY, accumulate=True, slice=True)
# what a fast-mode call gets below the wrapper's floor (M < 128 or N < 128): the f32 kernel, whatever the precision switch says
case("f32/fast_call_M6_splits4", "gemm", 6, 256, 1024, "gemm[6x256x1024]", "f32<0,1,2,0,0>+red1", splits=4, act=NONE)
case("f32/fast_call_N72", "gemm", 130, 72, 64, "gemm[130x72x64]", "f32<0,1,2,0,0>", act=LEAKY)
case("f32/fast_call_tn", "gemm", 130, 136, 64, "gemm[130x136x64]", "f32<1,0,2,0,0>", ak=True, bk=False, act=LEAKY)

# ---- generic split-bf16 kernel, three products and one (M < 1024 keeps the call off the prepared-fragment kernel)
for (ak, bk) in ((False, False), (False, True), (True, True)):
    for K in (64, 52):
        case(f"x3/{_L[(ak, bk)]}_K{K}", "gemm", 130, 136, K, f"gemmx3[130x136x{K}]", f"x3<{int(ak)},{int(bk)},2,{int(K == 52)},0>", ak=ak, bk=bk,
             act=_ACTS[_i % 4])
        _i += 1
case("x3/nt_K1024", "gemm", 130, 136, 1024, "gemmx3[130x136x1024]", "x3<0,1,2,0,0>", act=LEAKY)       # the deepest reduction of a split route here
case("x1/nt_K64", "gemm", 130, 136, 64, "gemmx1[130x136x64]", "x3<0,1,2,0,0>", mode="x1", act=LEAKY, slice=True)
case("x1/tt_K52", "gemm", 130, 136, 52, "gemmx1[130x136x52]", "x3<1,1,2,1,0>", ak=True, mode="x1", act=NONE)
case("x3/tt_batch2_N64_K64", "gemm", 130, 64, 64, "gemmx3[130x64x64]", "x3<1,1,1,0,0>", nb=2, ak=True, act=LEAKY)      # the only TN = 1 split route
case("x3/tt_batch2_N64_K52", "gemm", 130, 64, 52, "gemmx3[130x64x52]", "x3<1,1,1,1,0>", nb=2, ak=True, act=RELU)
case("x3/nt_slice_accumulate", "gemm", 130, 136, 52, "gemmx3[130x136x52]", "x3<0,1,2,1,0>", act=LEAKY, slice=True, accumulate=True)
# split-K on the split kernel
case("x3/nt_K192_splits3", "gemm", 130, 136, 192, "gemmx3[130x136x192]", "x3<0,1,2,0,0>+red1", splits=3, act=LEAKY)
case("x3/nt_K200_splits3", "gemm", 130, 136, 200, "gemmx3[130x136x200]", "x3<0,1,2,1,0>+red1", splits=3, act=SIGMOID, slice=True)
case("x3/nn_K200_splits3", "gemm", 130, 136, 200, "gemmx3[130x136x200]", "x3<0,0,2,1,0>+red1", bk=False, splits=3, act=RELU)
case("x3/nt_batch2_splits2", "gemm", 130, 136, 128, "gemmx3[130x136x128]", "x3<0,1,2,0,0>+red1", nb=2, splits=2, act=LEAKY, slice=True)
case("x1/nt_K200_splits3", "gemm", 130, 136, 200, "gemmx1[130x136x200]", "x3<0,1,2,1,0>+red1", mode="x1", splits=3, act=LEAKY)

# ---- split-K on the f32 kernels
case("splitk/two_stage", "gemm", 3, 40, 2048, "gemm[3x40x2048]", "f32<0,1,1,0,0>+red2", mode="f32", splits=64, act=LEAKY, slice=True)
case("splitk/one_stage", "gemm", 3, 40, 384, "gemm[3x40x384]", "f32<0,1,1,0,0>+red1", mode="f32", splits=12, act=RELU)
case("splitk/one_stage_tail", "gemm", 3, 40, 400, "gemm[3x40x400]", "f32<0,1,1,1,0>+red1", mode="f32", splits=12, act=SIGMOID, slice=True)
case("splitk/batch2_two_stage_form_refused", "gemm", 3, 40, 2048, "gemm[3x40x2048]", "f32<0,1,1,0,0>+red1", mode="f32", nb=2, splits=64, act=NONE)
for M, N, S, rg in ((1, 40, 4, 1), (16, 264, 2, 1), (17, 40, 3, 2), (33, 264, 2, 3), (49, 40, 4, 4), (64, 264, 3, 4)):
    case(f"smallm/M{M}_N{N}_splits{S}", "gemm", M, N, 128 * S, f"gemm[{M}x{N}x{128 * S}]", f"smallm<{rg}>+red1", mode="f32", splits=S,
         act=_ACTS[_i % 4], slice=(M in (17, 64)))
    _i += 1
case("smallm/M17_N264_K620_splits5", "gemm", 17, 264, 620, "gemm[17x264x620]", "smallm<2>+red1", mode="f32", splits=5, act=LEAKY)   # ragged last slice
case("smallm/M33_N40_two_stage", "gemm", 33, 40, 8192, "gemm[33x40x8192]", "smallm<3>+red2", mode="f32", splits=64, act=LEAKY, slice=True)
# (no sigmoid at K >= 8192: |pre| reaches the hundreds there, the float32 sigmoid underflows and the floor would measure that)
for M, N, K, mt in ((1, 256, 8192, 1), (2, 512, 8200, 2), (3, 256, 8200, 4), (4, 512, 8192, 4)):
    case(f"fewrows/M{M}_N{N}_K{K}", "gemm", M, N, K, f"gemm[{M}x{N}x{K}]", f"fewrows<{mt}>+red1", mode="f32", splits=cdiv(K, 256), act=_ACTS[_i % 3],
         slice=(M in (1, 3)))
    _i += 1
case("fewrows/M1_more_splits_than_slabs", "gemm", 1, 256, 8192, "gemm[1x256x8192]", "fewrows<1>+red1", mode="f32", splits=64, act=LEAKY)
for M, N, K in ((5, 256, 8192), (16, 512, 8200), (17, 256, 8200), (32, 512, 8192)):
    case(f"rows32/M{M}_N{N}_K{K}", "gemm", M, N, K, f"gemm[{M}x{N}x{K}]", "rows32+red1", mode="f32", splits=cdiv(K, 256), act=_ACTS[_i % 3],
         slice=(M in (5, 17)))
    _i += 1
# ops.linear: the torch weight layout keeps it off the weight-stream and column forms; its default split count is K // 128
case("linear/default_splits_K8192", "linear", 3, 256, 8192, "gemm[3x256x8192]", "f32<0,0,2,0,0>+red2", bk=False, splits=None, mode="f32", act=LEAKY, slice=True)
case("linear/default_splits_K520", "linear", 5, 40, 520, "gemm[5x40x520]", "f32<0,0,1,1,0>+red1", bk=False, splits=None, act=RELU)
case("linear/no_split_below_K512", "linear", 5, 40, 500, "gemm[5x40x500]", "f32<0,0,1,1,0>", bk=False, splits=None, mode="f32", act=SIGMOID)

# ---- generic kernels on cloud panels (X3T_PANELS off, K < 256): A only / C only / both, both weight layouts, f32 and split
_PAN = dict(Bc=2, Np=128)
for mode in ("f32", "x3"):
    for bk in (True, False):
        for pm, (pa, pc) in ((1, (True, False)), (2, (False, True)), (3, (True, True))):
            K = 32 if (pm + int(bk)) % 2 else 96
            kern = "f32" if mode == "f32" else "x3"
            case(f"panels/{kern}_{'kn' if bk else 'nk'}_P{pm}_K{K}", "panels", 256, 136, K, f"gemm{'x3' if mode == 'x3' else ''}[256x136x{K}]",
                 f"{kern}<0,{int(bk)},2,0,{pm}>", bk=bk, mode=mode, act=_ACTS[_i % 4], x3t_panels=False, panels=dict(_PAN, a=pa, c=pc),
                 accumulate=(pm == 2 and bk))
            _i += 1

# ---- the prepared-fragment kernel through ops.gemm: M = 1032 leaves a ragged last row tile
for N, K, bk, inst in ((64, 128, True, "x3w<1,0,0,32,1,0>"), (64, 264, False, "x3w<1,1,0,32,1,0>"), (72, 136, True, "x3w<1,1,0,32,0,0>"),
                       (200, 256, False, "x3w<1,0,0,32,0,0>"), (264, 128, True, "x3w<2,0,0,32,0,0>"), (264, 264, False, "x3w<2,1,0,32,0,0>")):
    case(f"x3w/N{N}_K{K}_{'kn' if bk else 'nk'}", "gemm", 1032, N, K, f"gemmx3w[1032x{N}x{K}]", inst, bk=bk, act=_ACTS[_i % 4], slice=(N == 72))
    _i += 1
case("x3w/impl2_N264", "gemm", 1032, 264, 128, "gemmx3w[1032x264x128]", "x3w<1,0,0,32,0,0>", x3w_impl=2, act=LEAKY)
case("x3w/impl3_N72", "gemm", 1032, 72, 136, "gemmx3w[1032x72x136]", "x3w<2,1,0,32,0,0>", x3w_impl=3, act=RELU)
case("x3w/impl3_N64", "gemm", 1032, 64, 128, "gemmx3w[1032x64x128]", "x3w<2,0,0,32,0,0>", x3w_impl=3, act=LEAKY)
case("x3w/impl2_N64_K136", "gemm", 1032, 64, 136, "gemmx3w[1032x64x136]", "x3w<1,1,0,32,1,0>", x3w_impl=2, act=NONE)
case("x3w/accumulate", "gemm", 1032, 200, 256, "gemmx3w[1032x200x256]", "x3w<1,0,0,32,0,0>", bk=False, act=LEAKY, accumulate=True, slice=True)
case("x3w/bare", "gemm", 1032, 200, 136, "gemmx3w[1032x200x136]", "x3w<1,1,0,32,0,0>", act=NONE, epi=False)     # the raw float2-store epilogue
case("x1w/N72_K128", "gemm", 1032, 72, 128, "gemmx1w[1032x72x128]", "x3w<1,0,0,32,0,0>", mode="x1", act=LEAKY)
case("x1w/N264_K264", "gemm", 1032, 264, 264, "gemmx1w[1032x264x264]", "x3w<2,1,0,32,0,0>", bk=False, mode="x1", act=NONE)
_PAN2 = dict(Bc=2, Np=512)
for N, wn in ((136, 1), (264, 2)):
    for pm, (pa, pc) in ((1, (True, False)), (2, (False, True)), (3, (True, True))):
        case(f"x3w/panels_N{N}_P{pm}", "panels", 1024, N, 256, f"gemmx3w[1024x{N}x256]", f"x3w<{wn},0,{pm},32,0,0>", bk=(pm != 2), act=_ACTS[_i % 4],
             panels=dict(_PAN2, a=pa, c=pc), accumulate=(pm == 2 and N == 136))
        _i += 1
# linear_bn_stats: the column sums and sums of squares out of the epilogue
case("stats/N72_K264", "bn_stats", 1032, 72, 264, "gemmx3w+stats[1032x72x264]", "x3w<1,1,0,32,0,0>", bk=False)
case("stats/N64_K256", "bn_stats", 1032, 64, 256, "gemmx3w+stats[1032x64x256]", "x3w<1,0,0,32,1,0>", bk=False, epi=False)
case("stats/N264_K128", "bn_stats", 1032, 264, 128, "gemmx3w+stats[1032x264x128]", "x3w<2,0,0,32,0,0>", bk=False)
case("stats/N256_K128_bf16c", "bn_stats", 1032, 256, 128, "gemmx3w+stats[1032x256x128]", "x3w<2,0,0,32,0,2>", bk=False, c16=True)
case("stats/N256_K128_bf16a_bf16c", "bn_stats", 1032, 256, 128, "gemmx3w+stats[1032x256x128]", "x3w<2,0,0,32,0,3>", bk=False, a16=True, c16=True)
# gemm_act: BatchNorm affine + activation in the operand loader
case("act/f32_N64_store", "gemm_act", 1032, 64, 256, "gemmx3w+act[1032x64x256]", "x3w<1,0,0,32,1,0>", act=LEAKY, epi=False)
case("act/f32_N128_nostore", "gemm_act", 1032, 128, 256, "gemmx3w+act[1032x128x256]", "x3w<1,0,0,32,0,0>", act=RELU, epi=False, store=False)
case("act/f32_N128_K264", "gemm_act", 1032, 128, 264, "gemmx3w+act[1032x128x264]", "x3w<1,1,0,32,0,0>", act=LEAKY, epi=False)
case("act/bf16_N64_map16_nostore", "gemm_act", 1032, 64, 256, "gemmx3w+act[1032x64x256]", "x3w<1,0,0,32,1,5>", act=LEAKY, epi=False, a16=True,
     map16=True, store=False)
case("act/bf16_N128_map16", "gemm_act", 1032, 128, 256, "gemmx3w+act[1032x128x256]", "x3w<1,0,0,32,0,5>", act=RELU, epi=False, a16=True, map16=True)
case("act/bf16_N64_map32", "gemm_act", 1032, 64, 256, "gemmx3w+act[1032x64x256]", "x3w<1,0,0,32,1,5>", act=NONE, epi=False, a16=True)
case("act/f32_N64_single_product", "gemm_act", 1032, 64, 256, "gemmx3w+act[1032x64x256]", "x3w<1,0,0,32,1,0>", act=LEAKY, epi=False, mode="x1")
# gemm_bf16a: bf16 rows against the split weight
case("bf16a/N64", "bf16a", 200, 64, 96, "gemmx2w[200x64x96]", "x3w<1,0,0,32,1,1>", epi=False, a16=True)
case("bf16a/N128_nk_accumulate", "bf16a", 200, 128, 96, "gemmx2w[200x128x96]", "x3w<1,0,0,32,0,1>", bk=False, epi=False, a16=True, accumulate=True, slice=True)
case("bf16a/N256", "bf16a", 200, 256, 64, "gemmx2w[200x256x64]", "x3w<2,0,0,32,0,1>", epi=False, a16=True)
# the batched per-problem form at the wrapper's floor: nb * M = 16384
for N, a16, aff, inst in ((64, False, False, "x3w<1,0,0,32,1,0>"), (128, False, True, "x3w<1,0,0,32,0,0>"), (64, True, True, "x3w<1,0,0,32,1,5>"),
                          (128, True, False, "x3w<1,0,0,32,0,1>")):
    case(f"x3wb/N{N}_{'bf16' if a16 else 'f32'}{'_affine' if aff else ''}", "gemm", 128, N, 256, f"gemmx3w[128x{N}x256]x128", inst, nb=128, epi=False,
         a16=a16, a_affine=aff, act=(LEAKY if aff else NONE))

# ---- the transposed short-reduction kernel
_PAN3 = dict(Bc=3, Np=384, a=True, c=True)      # 9 workgroups
for N, K, act, bk in ((160, 64, NONE, False), (160, 128, RELU, False), (128, 64, LEAKY, True), (160, 128, LEAKY, True)):
    case(f"x3t/panels_N{N}_K{K}_act{act}", "panels", 1152, N, K, f"gemmx3t[1152x{N}x{K}]", f"x3t<{K // 16},0,128>", bk=bk, act=act, panels=dict(_PAN3))
case("x3t/split_N32_K64", "x3t_split", 1152, 32, 64, "gemmx3t[1152x32x64]", "x3t<4,0,128>", bk=False, epi=False, split_in=True, panels=dict(_PAN3))
case("x3t/split_N96_K128", "x3t_split", 1152, 96, 128, "gemmx3t[1152x96x128]", "x3t<8,0,128>", bk=False, epi=False, split_in=True, panels=dict(_PAN3))
case("x3t/rows_N32_K64", "gemm", 16512, 32, 64, "gemmx3t[16512x32x64]", "x3t<4,1,128>", bk=False, act=LEAKY)       # 129 workgroups
case("x3t/rows_N96_K128", "gemm", 16512, 96, 128, "gemmx3t[16512x96x128]", "x3t<8,1,128>", act=RELU, slice=True)
case("x3t/rows_N32_K128_bf16", "gemm", 16512, 32, 128, "gemmx3t[16512x32x128]", "x3t<8,1,64>", act=LEAKY, c16=True, slice=True)
case("x3t/rows_N96_K64_bf16", "gemm", 16512, 96, 64, "gemmx3t[16512x96x64]", "x3t<4,1,128>", bk=False, act=NONE, c16=True)
case("x3t/rows_batch9", "gemm", 2048, 32, 64, "gemmx3t[2048x32x64]x9", "x3t<4,1,128>", nb=9, act=LEAKY, slice=True)

# ---- the panel kernel on split planes: K = 64 is two k-tiles, fewer than the units of lookahead
for Bc, K, pc, impl in ((1, 64, False, 0), (3, 96, True, 0), (3, 512, False, 5), (1, 96, True, 5)):
    case(f"p8/B{Bc}_K{K}_{'panels' if pc else 'rows'}_impl{impl}", "p8", 256 * Bc, 256, K, f"gemm_p8[{256 * Bc}x256x{K}]",
         f"p8<{5 if impl == 5 else 6},{int(pc)},0>", bk=False, act=_ACTS[_i % 3], p8_impl=impl, split_in=True, slice=True,
         panels=dict(Bc=Bc, Np=256, a=True, c=pc))
    _i += 1
case("p8/fused_B3_K64_rows", "p8", 768, 256, 64, "gemm_p8+assign[768x256x64]", "p8<6,0,1>", bk=False, act=LEAKY, assign=True, split_in=True,
     panels=dict(Bc=3, Np=256, a=True, c=False))
case("p8/fused_B1_K512_panels", "p8", 256, 256, 512, "gemm_p8+assign[256x256x512]", "p8<6,1,1>", bk=False, act=RELU, assign=True, split_in=True,
     panels=dict(Bc=1, Np=256, a=True, c=True))

N_CASES = 138      # a case leaves the table only on purpose: tests/test_gemm_routes_cpu.py holds this count


def _k(c):          # the kernel of a case without its reduction stage
    return c["inst"].split("+")[0]


# What the table must hold besides one case per instance: (what, predicate, least number of cases).  An instance reached twice hides a
# deleted case from BUILT; a property listed here does not.
REQUIRED = [
    ("f32 kernel at M = 1", lambda c: _k(c).startswith("f32<") and c["M"] == 1, 2),
    ("f32 kernel, K = 37 inside padded rows, every layout", lambda c: _k(c).startswith("f32<") and c["K"] == 37, 4),
    ("f32 kernel batched", lambda c: _k(c).startswith("f32<") and c["nb"] == 3, 2),
    ("f32 kernel into a slice", lambda c: _k(c).startswith("f32<") and c["slice"] and c["splits"] == 1, 3),
    ("f32 kernel accumulating", lambda c: _k(c).startswith("f32<") and c["accumulate"] and c["panels"] is None, 1),
    ("a fast-mode call below the wrapper's floor stays on the f32 kernel", lambda c: c["mode"] == "x3" and c["label"].startswith("gemm[")
     and c["wrapper"] == "gemm", 3),
    ("split kernel, K in {64, 52}, three layouts", lambda c: _k(c).startswith("x3<") and c["K"] in (64, 52) and c["nb"] == 1 and c["mode"] == "x3"
     and c["panels"] is None and not c["slice"], 6),
    ("single product on the generic kernel", lambda c: c["label"].startswith("gemmx1["), 3),
    ("single product on the prepared-fragment kernel", lambda c: c["label"].startswith("gemmx1w["), 2),
    ("split-K on the split kernel without a tail", lambda c: _k(c) == "x3<0,1,2,0,0>" and c["splits"] == 3 and c["K"] == 192, 1),
    ("split-K on the split kernel with a tail", lambda c: _k(c).startswith("x3<") and _k(c).endswith(",1,0>") and c["splits"] == 3 and c["K"] == 200, 3),
    ("split-K on the split kernel, batched", lambda c: _k(c).startswith("x3<") and c["nb"] == 2 and c["splits"] == 2, 1),
    ("split kernel into a slice, accumulating", lambda c: _k(c).startswith("x3<") and c["slice"] and c["accumulate"], 1),
    ("two-stage reduction behind the f32 kernel", lambda c: c["inst"].startswith("f32<") and c["inst"].endswith("+red2"), 2),
    ("two-stage reduction refused for a batch", lambda c: c["nb"] == 2 and c["splits"] == 64 and c["inst"].endswith("+red1"), 1),
    ("one-stage reduction with a k tail", lambda c: c["inst"] == "f32<0,1,1,1,0>+red1" and c["splits"] == 12, 1),
    ("column form at M = 1, 16, 17, 33, 49, 64", lambda c: _k(c).startswith("smallm<") and c["M"] in (1, 16, 17, 33, 49, 64)
     and c["K"] == 128 * c["splits"] and c["splits"] < 64, 6),
    ("column form, ragged last slice", lambda c: _k(c).startswith("smallm<") and c["K"] == 620 and c["splits"] == 5, 1),
    ("column form into the two-stage reduction", lambda c: c["inst"] == "smallm<3>+red2", 1),
    ("weight stream at M = 1, 2, 3, 4", lambda c: _k(c).startswith("fewrows<") and c["splits"] == cdiv(c["K"], 256), 4),
    ("weight stream with a ragged last slab", lambda c: _k(c).startswith("fewrows<") and c["K"] == 8200, 2),
    ("weight stream with more splits than slabs", lambda c: _k(c).startswith("fewrows<") and c["splits"] > cdiv(c["K"], 256), 1),
    ("rows32 at M = 5, 16, 17, 32", lambda c: _k(c) == "rows32" and c["M"] in (5, 16, 17, 32), 4),
    ("rows32 with a ragged last slab", lambda c: _k(c) == "rows32" and c["K"] == 8200, 2),
    ("a slice behind every split-K producer", lambda c: c["slice"] and "+red" in c["inst"] and _k(c)[:3] in ("f32", "sma", "few", "row", "x3<"), 12),
    ("ops.linear's default split count", lambda c: c["wrapper"] == "linear" and c["splits"] is None, 3),
    ("prepared-fragment kernel at a ragged last row tile", lambda c: c["label"].startswith("gemmx3w[") and c["M"] == 1032, 12),
    ("prepared-fragment kernel, forced block shapes", lambda c: c["x3w_impl"] in (2, 3) and c["wrapper"] == "gemm", 4),
    ("prepared-fragment kernel accumulating into a slice", lambda c: c["label"].startswith("gemmx3w[") and c["accumulate"] and c["slice"], 1),
    ("statistics with fp32 and bf16 C and bf16 A", lambda c: c["wrapper"] == "bn_stats", 5),
    ("gemm_act with and without the stored map, N = 64 and 128", lambda c: c["wrapper"] == "gemm_act", 7),
    ("gemm_act without the stored map", lambda c: c["wrapper"] == "gemm_act" and not c["store"], 2),
    ("gemm_bf16a at N = 64, 128, 256", lambda c: c["wrapper"] == "bf16a", 3),
    ("batched per-problem form at the wrapper's floor", lambda c: c["nb"] * c["M"] == ROWS_MIN and c["M"] == 128 and c["K"] == 256, 4),
    ("x3t panels with every activation, 9 workgroups", lambda c: c["label"].startswith("gemmx3t[1152x") and c["wrapper"] == "panels", 4),
    ("x3t on split planes", lambda c: c["wrapper"] == "x3t_split", 2),
    ("x3t rows at 129 workgroups, fp32 and bf16", lambda c: c["label"].startswith("gemmx3t[16512x"), 4),
    ("x3t rows batched into a slice", lambda c: c["label"].endswith("x9") and c["slice"], 1),
    ("panel kernel at two k-tiles", lambda c: c["wrapper"] == "p8" and c["K"] == 64, 2),
    ("panel kernel, fused assignment, rows and panels", lambda c: c["wrapper"] == "p8" and c["assign"], 2),
]


# ================================================================== every instance the sources build
def _built():
    """{instance: 'reached by <case>' | 'not reachable through a wrapper: <condition>'}"""
    b = {}
    first = {}
    for c in CASES:
        first.setdefault(c["inst"].split("+")[0], c["name"])
    for c in CASES:
        if "+red" in c["inst"]:
            first.setdefault("splitk_reduce" + c["inst"][c["inst"].index("+"):], c["name"])

    def put(inst, why=None):
        b[inst] = ("reached by " + first[inst]) if inst in first else why

    for kern in ("f32", "x3"):
        for ak in (0, 1):
            for bk in (0, 1):
                for tn in (1, 2):
                    for kt in (0, 1):
                        why = None
                        if kern == "x3" and ak and not bk:
                            why = "not reachable through a wrapper: ops.gemm takes the split form only for `not a_kmajor or b_kmajor`"
                        elif kern == "x3" and tn == 1 and not (ak and bk):
                            why = ("not reachable through a wrapper: ops.gemm takes the split form only for N >= 128 (TN = 2); N = 64 only for the "
                                   "batched both-k-major product")
                        put(f"{kern}<{ak},{bk},{tn},{kt},0>", why)
        for bk in (0, 1):
            for pm in (1, 2, 3):
                put(f"{kern}<0,{bk},2,0,{pm}>")
    for i in ("fewrows<1>", "fewrows<2>", "fewrows<4>", "rows32", "smallm<1>", "smallm<2>", "smallm<3>", "smallm<4>", "splitk_reduce+red1",
              "splitk_reduce+red2"):
        put(i)
    for wn in (1, 2):
        for kt in (0, 1):
            for pm in (0, 1, 2, 3):
                put(f"x3w<{wn},{kt},{pm},32,0,0>",
                    "not reachable through a wrapper: ops._gemm_panels requires K % 32 == 0 of cloud-panel operands" if (kt and pm) else None)
                put(f"x3w<{wn},{kt},{pm},64,0,0>", "not reachable through a wrapper: 64-deep chunks need LPD_DEBUG=x3w-kc=64 (an experiment)")
    for kt in (0, 1):
        for pm in (0, 1, 2, 3):
            put(f"x3w<1,{kt},{pm},32,1,0>", "not reachable through a wrapper: ops._gemm_panels takes the split form only for N >= 128, "
                "the tall form is N <= 64" if pm else None)
    for inst in ("x3w<2,0,0,32,0,2>", "x3w<2,0,0,32,0,3>", "x3w<2,0,0,32,0,1>", "x3w<1,0,0,32,1,1>", "x3w<1,0,0,32,0,1>", "x3w<1,0,0,32,1,5>",
                 "x3w<1,0,0,32,0,5>"):
        put(inst)
        put(inst.replace("<2,0,", "<2,1,").replace("<1,0,", "<1,1,"),
            "not reachable through a wrapper: every wrapper (and gemm_x3w_impl itself) requires K % 32 == 0 of bf16 rows or a bf16 result")
    for inst in ("x3t<4,0,128>", "x3t<8,0,128>", "x3t<4,1,128>", "x3t<8,1,128>", "x3t<8,1,64>"):
        put(inst)
    for inst in ("p8<6,0,0>", "p8<6,1,0>", "p8<5,0,0>", "p8<5,1,0>", "p8<6,0,1>", "p8<6,1,1>"):
        put(inst)
    return b


BUILT = _built()
UNREACHABLE = sorted(k for k, v in BUILT.items() if v is None or v.startswith("not reachable"))
