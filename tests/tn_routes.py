"""The dispatch of the A^T B and bf16-storage products of csrc/lpd_train2.hip and csrc/lpd_train3.hip, restated in Python, and the table of
cases at which tests/test_tn_routes_gpu.py runs every route (the companion of tests/gemm_routes.py for the forward GEMM family).

Layer 1 (lpdnet_hip/ops.py) chooses an entry point and an ops.PROFILE label:
    gemm_tn[KAxKBxM](xB)        lpd_gemm_tn        ops.gemm_tn, ops.pool_tn
    gemm_tn+act[KAxKBxM](xB)    lpd_gemm_tn_act    ops.gemm_tn(a_affine=..), where ops.gemm_tn_act_applies
    gemm_tn_bf16[KAxKBxM]       lpd_gemm_tn_bf16   ops.gemm_tn_bf16
    gemm_bf16s[MxNxK]           lpd_gemm_bf16s     ops.gemm_bf16s
    edge_dw_sel_bf16[E] / edge_dw_sel_f32[E]       ops.edge_dw_sel_bf16 / ops.edge_dw_sel_f32
The label names neither the tile width nor the split count nor the number of products per term; layer 2 (gemm_tn_impl and the entry
points themselves) decides those.  Instances are written as the sources order the template arguments, booleans as 0 / 1:
    tn_x3<KBT,AB>          gemm_tn_x3_kernel          register-transposing, 128 x KBT tiles, 64-row chunks
    tn_x3_256<AB>          gemm_tn_x3_256_kernel      register-transposing, 256 x 256 tiles
    tn_tr<A16,TB,ATR,B16>  gemm_tn_tr_kernel          transposed LDS reads, 256 x TB tiles, 32-row chunks
    tn_bf16<K>             gemm_tn_bf16_kernel<K, K>
    bf16s<K,N>             gemm_bf16s_kernel
    dw_sel_bf16 / dw_sel_f32 / dw_sel_tr<BF16>        edge_dw_sel_bf16_kernel / edge_dw_sel_f32_kernel / edge_dw_sel_tr_kernel
followed by the reduction over the slabs: `+reduce16[nslabs]` (gemm_tn_reduce16_kernel) or `+slab_reduce[nslabs]` (slab_reduce_kernel
and dw2_finish_kernel of the edge entries).
route(case) -> (label, instance, splits, products per term) under the LPD_DEBUG switches the case names (`sw`; the library reads them
once per process, so tests/test_tn_routes_gpu.py runs such a case in a child interpreter).  CASES is the table; BUILT lists every
instance the sources build, each `reached by <case>`, `reached by <case> under LPD_DEBUG=<switches>` or `not reachable ..`.
tests/test_tn_routes_cpu.py holds the table to the restatement and the restatement to the sources and to the library's own host functions.
"""
import zlib

# ---- constants of the sources (tests/test_tn_routes_cpu.py finds them in the .hip text)
TR_MIN_M = 2048           # tn_tr_tb: M >= 2048
TR_CHUNK = 32             # ... M % 32 == 0; rows_per_split of the transposed-read route is rounded to 32
TR_SPLIT_ROWS = 256       # gemm_tn_splits: a split of the transposed-read route keeps M / splits >= 256
TR_CAP_ONE, TR_CAP_TWO = 256, 512     # blocks in flight: one per CU, two with bf16 rows as A and narrow B tiles
T256_MIN_M = 8192         # gemm_tn_256
X3_SPLIT_ROWS = 1024      # the register-transposing routes keep M / splits >= 1024
X3_CHUNK = 64             # rows_per_split elsewhere is rounded to 64
TN_BLOCKS = 512           # LPD_DEBUG=tn-blocks default
TNBF16_ROWS, TNBF16_MAX = 2048, 1024      # lpd_gemm_tn_bf16_ws_floats: blocks = clamp(M / 2048, 1, 1024)
DWSEL_ROWS, DWSEL_MAX = 4096, 256         # edge_dw_sel_blocks: clamp(E / 4096, 1, 256)
DWSEL_SLAB = 256 * 128 + 128              # floats of a slab: S | G | column sums
BF16S_WAVE_ROWS, BF16S_PER_BLOCK, BF16S_CAP = 32, 32, 2048     # lpd_gemm_bf16s: grid_for((M + 31) / 32, 4 * 8, 2048)
# ---- constants of the wrappers (lpdnet_hip/ops.py)
TN_APPLIES_ROWS = 4096    # ops.gemm_tn_applies: rows >= 4096
POOL_MIN_N = 256          # ops.pool_tn: N >= 256

SWITCHES = {"tn-tr": 1, "tn256": 1, "tn-blocks": TN_BLOCKS, "dw-sel-tr": 1}      # the defaults


def switches(sw=""):
    """'tn-tr=0,tn256=0' -> the switch values the library would read from LPD_DEBUG"""
    out = dict(SWITCHES)
    for t in sw.split(","):
        if t:
            k, v = t.split("=")
            assert k in out, k
            out[k] = int(v)
    return out


def cdiv(a, b):
    return (a + b - 1) // b


def rup(a, b):
    return cdiv(a, b) * b


# ================================================================== layer 2: lpd_gemm_tn / lpd_gemm_tn_act
def tn_tr_tb(M, KA, KB, batch, a_bf16, act=False, sw=SWITCHES):
    """b-channels per block of the transposed-read kernel, 0 where it is not taken; with the operand transform (act) the switch is ignored"""
    if KA % 256 != 0 or KB % 64 != 0 or M % TR_CHUNK != 0 or M < TR_MIN_M:
        return 0
    tb = 256 if KB % 256 == 0 else (128 if KB % 128 == 0 else 64)
    if act:
        return tb
    if not sw["tn-tr"]:
        return 0
    if not a_bf16 and batch > 1:
        return 0
    return tb


def gemm_tn_256(M, KA, KB, batch, sw=SWITCHES):
    return bool(sw["tn256"]) and batch == 1 and KA % 256 == 0 and KB % 256 == 0 and M % 32 == 0 and M >= T256_MIN_M


def gemm_tn_splits(M, KA, KB, batch, a_bf16=True, act=False, sw=SWITCHES):
    tb = tn_tr_tb(M, KA, KB, batch, a_bf16, act, sw)
    if tb:
        tiles, cap, rows = (KA // 256) * (KB // tb) * batch, (TR_CAP_ONE if (tb == 256 or not a_bf16) else TR_CAP_TWO), TR_SPLIT_ROWS
    elif gemm_tn_256(M, KA, KB, batch, sw):
        tiles, cap, rows = (KA // 256) * (KB // 256), 256, X3_SPLIT_ROWS
    else:
        tiles, cap, rows = (KA // 128) * cdiv(KB, 128) * batch, sw["tn-blocks"], X3_SPLIT_ROWS
    splits = 1
    while tiles * splits * 2 <= cap and M // (splits * 2) >= rows:
        splits *= 2
    return splits


def rows_per_split(M, splits, tr):
    return rup(cdiv(M, splits), TR_CHUNK if tr else X3_CHUNK)


def tn_ws_floats(M, KA, KB, batch, sw=SWITCHES):
    """lpd_gemm_tn_ws_floats: room for either operand type"""
    batch = max(batch, 1)
    return max(gemm_tn_splits(M, KA, KB, batch, True, False, sw), gemm_tn_splits(M, KA, KB, batch, False, False, sw)) * batch * KA * KB


def tn_act_ws_floats(M, KA, KB, batch, a_bf16, sw=SWITCHES):
    batch = max(batch, 1)
    return gemm_tn_splits(M, KA, KB, batch, bool(a_bf16), True, sw) * batch * KA * KB


def entry_tn(M, KA, KB, batch, a16, b16, affine, sw=SWITCHES):
    """gemm_tn_impl -> (instance, splits, products per term); None: LPD_CHECK_ARG refuses the call"""
    if not (M > 0 and batch >= 1 and KA > 0 and KA % 128 == 0 and KB > 0 and KB % 64 == 0):
        return None
    if b16 and not (a16 and not affine and batch == 1 and tn_tr_tb(M, KA, KB, batch, True, True, sw) == 256):
        return None
    act = affine or b16                       # both forms exist on the transposed-read kernel only
    if act and not tn_tr_tb(M, KA, KB, batch, a16, True, sw):
        return None
    splits = gemm_tn_splits(M, KA, KB, batch, a16, act, sw)
    prods = 1 if b16 else (2 if a16 else 3)
    red = f"+reduce16[{splits}]"              # n = KA * KB is a multiple of 128 * 64: `n % 64 == 0` always holds
    tb = tn_tr_tb(M, KA, KB, batch, a16, act, sw)
    if tb:
        if b16:
            return "tn_tr<1,256,0,1>" + red, splits, prods
        if act:
            if tb != 64:
                return None                   # the transform is built for the 64-wide tile only
            return f"tn_tr<{int(a16)},64,1,0>" + red, splits, prods
        return f"tn_tr<{int(a16)},{tb},0,0>" + red, splits, prods
    if gemm_tn_256(M, KA, KB, batch, sw):
        return f"tn_x3_256<{int(a16)}>" + red, splits, prods
    kbt = 128 if KB % 128 == 0 else 64
    return f"tn_x3<{kbt},{int(a16)}>" + red, splits, prods


# ================================================================== layer 2: the other entries
def tn_bf16_blocks(M):
    return min(max(M // TNBF16_ROWS, 1), TNBF16_MAX)


def tn_bf16_ws_floats(M, KA, KB):
    return tn_bf16_blocks(M) * KA * KB


def tn_bf16_rows_per_block(M):
    return rup(cdiv(M, tn_bf16_blocks(M)), 64)


def entry_tn_bf16(M, KA, KB):
    if not ((KA == 128 and KB == 128) or (KA == 64 and KB == 64)) or M <= 0:
        return None
    b = tn_bf16_blocks(M)
    return f"tn_bf16<{KA}>+reduce16[{b}]", b, 1


def bf16s_grid(M):
    """blocks of lpd_gemm_bf16s: four waves a block, a wave a 32-row tile at a time, eight tiles per wave before the grid grows"""
    return min(max(cdiv(cdiv(M, BF16S_WAVE_ROWS), BF16S_PER_BLOCK), 1), BF16S_CAP)


def entry_bf16s(M, N, K):
    if not ((N == 128 and K == 128) or (N == 64 and K == 64)) or M <= 0:
        return None
    return f"bf16s<{K},{N}>", 1, 2


def edge_dw_sel_blocks(E):
    return min(max(E // DWSEL_ROWS, 1), DWSEL_MAX)


def edge_dw_sel_rows_per_block(E, bf16):
    return rup(cdiv(E, edge_dw_sel_blocks(E)), 128 if bf16 else 64)


def edge_dw_sel_ws_bytes(E):
    return edge_dw_sel_blocks(E) * DWSEL_SLAB * 4 + DWSEL_SLAB * 8


def entry_dw_sel(Mp, k, bf16, sw=SWITCHES):
    E = Mp * k
    if not (8 <= k <= 255 and Mp > 0 and E % (128 if bf16 else 64) == 0):
        return None
    b = edge_dw_sel_blocks(E)
    if bf16:
        kern = "dw_sel_tr<1>" if sw["dw-sel-tr"] == 2 else "dw_sel_bf16"       # measured slower on bf16 tensors: on request only
    else:
        kern = "dw_sel_tr<0>" if sw["dw-sel-tr"] != 0 else "dw_sel_f32"
    return f"{kern}+slab_reduce[{b}]", b, (1 if bf16 else 3)


# ================================================================== layer 1: the wrappers
def gemm_tn_act_applies(M, KA, KB):
    """ops.gemm_tn_act_applies on aligned unit-stride operands with every ops switch on"""
    return KA % 256 == 0 and KB % 64 == 0 and KB % 128 != 0 and M % 32 == 0 and M >= 2048


def gemm_tn_applies(KA, KB, rows):
    """ops.gemm_tn_applies on aligned 2-D unit-stride operands: where the training path takes lpd_gemm_tn for a weight gradient"""
    return KA % 128 == 0 and KB % 64 == 0 and rows >= TN_APPLIES_ROWS


def pool_tn_applies(N, E, K):
    """ops.pool_tn on contiguous operands"""
    return E % 128 == 0 and K % 64 == 0 and N >= POOL_MIN_N


def route_gemm_tn(c):
    M, KA, KB, nb, a16, b16, aff = c["M"], c["KA"], c["KB"], c["nb"], c["a16"], c["b16"], c["affine"]
    if b16 and (not a16 or nb > 1 or aff):
        return None                          # ValueError of ops.gemm_tn
    if aff and (c["extra"] or not gemm_tn_act_applies(M, KA, KB)):
        return None
    if c["wrapper"] == "pool_tn" and not (pool_tn_applies(M, KA, KB) and not a16 and not aff and not c["sliced"]):
        return None
    e = entry_tn(M, KA, KB, nb, a16, b16, aff, switches(c["sw"]))
    if e is None:
        return None
    label = ("gemm_tn+act" if aff else "gemm_tn") + f"[{KA}x{KB}x{M}]" + (f"x{nb}" if nb > 1 else "")
    return (label,) + e


def route_tn_bf16(c):
    e = entry_tn_bf16(c["M"], c["KA"], c["KB"])
    return None if e is None else (f"gemm_tn_bf16[{c['KA']}x{c['KB']}x{c['M']}]",) + e


def route_bf16s(c):
    e = entry_bf16s(c["M"], c["KB"], c["KA"])
    return None if e is None else (f"gemm_bf16s[{c['M']}x{c['KB']}x{c['KA']}]",) + e


def route_dw_sel(c):
    e = entry_dw_sel(c["M"], c["k"], c["a16"], switches(c["sw"]))
    return None if e is None else (f"edge_dw_sel_{'bf16' if c['a16'] else 'f32'}[{c['M'] * c['k']}]",) + e


ROUTES = {"gemm_tn": route_gemm_tn, "pool_tn": route_gemm_tn, "gemm_tn_bf16": route_tn_bf16, "gemm_bf16s": route_bf16s, "dw_sel": route_dw_sel}


def route(c):
    """(label, instance, splits, products)"""
    return ROUTES[c["wrapper"]](c)


# ================================================================== the cases
CASES = []


def case(name, wrapper, M, KA, KB, label, inst, splits, prods, **kw):
    """gemm_tn / pool_tn: A [nb, M, KA], B [nb, M, KB]; extra: rows of the buffer past the `rows` the call names.  gemm_tn_bf16 the same,
    contiguous.  gemm_bf16s: A [M, K = KA], W N = KB columns.  dw_sel: M points of k edges, 128 channels; a16: bf16 storage."""
    c = dict(name=name, wrapper=wrapper, M=M, KA=KA, KB=KB, label=label, inst=inst, splits=splits, prods=prods, nb=1, extra=0, a16=False,
             b16=False, affine=False, sliced=wrapper == "gemm_tn", sw="", k=0, b_kmajor=False)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    c["seed"] = zlib.crc32(name.encode())
    assert name not in {x["name"] for x in CASES}, name
    CASES.append(c)
    return c


def by_name(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


_T = {False: "f32", True: "bf16"}

# ---- the transposed-read kernel at the default switches.  M = 2048, KA = 256: one a-tile, 8 splits of 8 chunks of 32 rows
for a16 in (False, True):
    for KB in (256, 128, 64):
        case(f"tr/{_T[a16]}_KB{KB}_M2048", "gemm_tn", 2048, 256, KB, f"gemm_tn[256x{KB}x2048]", f"tn_tr<{int(a16)},{KB},0,0>+reduce16[8]", 8,
             2 if a16 else 3, a16=a16)
# M = 2080: 8 splits of 288 rows = 9 chunks (the double buffer ends on the other half), the last split 64 rows = 2 chunks
case("tr/f32_KB256_M2080", "gemm_tn", 2080, 256, 256, "gemm_tn[256x256x2080]", "tn_tr<0,256,0,0>+reduce16[8]", 8, 3)
case("tr/bf16_KB64_M2080", "gemm_tn", 2080, 256, 64, "gemm_tn[256x64x2080]", "tn_tr<1,64,0,0>+reduce16[8]", 8, 2, a16=True)
# the operand transform (negative scales on every fifth channel, LeakyReLU 0.2), plain and batched
for a16 in (False, True):
    case(f"tr/act_{_T[a16]}", "gemm_tn", 2048, 256, 64, "gemm_tn+act[256x64x2048]", f"tn_tr<{int(a16)},64,1,0>+reduce16[8]", 8, 2 if a16 else 3,
         a16=a16, affine=True)
    case(f"tr/act_{_T[a16]}_batch2", "gemm_tn", 2048, 256, 64, "gemm_tn+act[256x64x2048]x2", f"tn_tr<{int(a16)},64,1,0>+reduce16[8]", 8,
         2 if a16 else 3, a16=a16, affine=True, nb=2)
case("tr/bf16_bf16_M2048", "gemm_tn", 2048, 256, 256, "gemm_tn[256x256x2048]", "tn_tr<1,256,0,1>+reduce16[8]", 8, 1, a16=True, b16=True)
case("tr/bf16_KB128_batch2", "gemm_tn", 2048, 256, 128, "gemm_tn[256x128x2048]x2", "tn_tr<1,128,0,0>+reduce16[8]", 8, 2, a16=True, nb=2)
# 128 slabs: gemm_tn_reduce16_kernel walks 64 slabs a trip
case("tr/f32_KB64_M32768_128slabs", "gemm_tn", 32768, 256, 64, "gemm_tn[256x64x32768]", "tn_tr<0,64,0,0>+reduce16[128]", 128, 3)

# ---- the register-transposing kernel at the default switches
for a16 in (False, True):
    for KB in (128, 64):
        # one slab, the second 64-row chunk holds 36 rows
        case(f"x3/{_T[a16]}_KB{KB}_M100", "gemm_tn", 100, 128, KB, f"gemm_tn[128x{KB}x100]", f"tn_x3<{KB},{int(a16)}>+reduce16[1]", 1,
             2 if a16 else 3, a16=a16)
        # two splits of 1088 rows, the second 997 = 15 chunks and 37 rows
        case(f"x3/{_T[a16]}_KB{KB}_M2085", "gemm_tn", 2085, 128, KB, f"gemm_tn[128x{KB}x2085]", f"tn_x3<{KB},{int(a16)}>+reduce16[2]", 2,
             2 if a16 else 3, a16=a16)
case("x3/f32_KB128_rows1100_of_1200", "gemm_tn", 1100, 128, 128, "gemm_tn[128x128x1100]", "tn_x3<128,0>+reduce16[1]", 1, 3, extra=100)
case("x3/bf16_KB64_rows1100_of_1200", "gemm_tn", 1100, 128, 64, "gemm_tn[128x64x1100]", "tn_x3<64,1>+reduce16[1]", 1, 2, a16=True, extra=100)
# fp32 rows, batched, at a shape the transposed-read route would take for one problem
case("x3/f32_KA256_KB64_batch3", "gemm_tn", 2048, 256, 64, "gemm_tn[256x64x2048]x3", "tn_x3<64,0>+reduce16[2]", 2, 3, nb=3)
case("x3/f32_KA256_KB128_batch3", "gemm_tn", 2048, 256, 128, "gemm_tn[256x128x2048]x3", "tn_x3<128,0>+reduce16[2]", 2, 3, nb=3)
# ops.pool_tn at its floor (contiguous operands: the wrapper's condition)
case("x3/pool_tn_N256_batch2", "pool_tn", 256, 128, 64, "gemm_tn[128x64x256]x2", "tn_x3<64,0>+reduce16[1]", 1, 3, nb=2)

# ---- routes only a switch reaches
for a16 in (False, True):
    case(f"sw/no_tr/x3_256_{_T[a16]}_M8192", "gemm_tn", 8192, 256, 256, "gemm_tn[256x256x8192]", f"tn_x3_256<{int(a16)}>+reduce16[8]", 8,
         2 if a16 else 3, a16=a16, sw="tn-tr=0")
case("sw/no_tr/x3_f32_KA256_KB128_M2048", "gemm_tn", 2048, 256, 128, "gemm_tn[256x128x2048]", "tn_x3<128,0>+reduce16[2]", 2, 3, sw="tn-tr=0")
case("sw/no_tr/x3_bf16_KA256_KB64_M2048", "gemm_tn", 2048, 256, 64, "gemm_tn[256x64x2048]", "tn_x3<64,1>+reduce16[2]", 2, 2, a16=True, sw="tn-tr=0")
case("sw/no_tr_no_256/x3_f32_M8192", "gemm_tn", 8192, 256, 256, "gemm_tn[256x256x8192]", "tn_x3<128,0>+reduce16[8]", 8, 3, sw="tn-tr=0,tn256=0")
# 512 tiles: one split at the default cap of 512 blocks, two at 1024 (M / 2 >= 1024; M % 32 != 0 keeps the call off the other routes)
case("sw/tn_blocks1024/x3_f32_512tiles_M2064", "gemm_tn", 2064, 8192, 1024, "gemm_tn[8192x1024x2064]", "tn_x3<128,0>+reduce16[2]", 2, 3,
     sw="tn-blocks=1024")

# ---- lpd_gemm_tn_bf16
for K in (128, 64):
    case(f"tn_bf16/K{K}_M100", "gemm_tn_bf16", 100, K, K, f"gemm_tn_bf16[{K}x{K}x100]", f"tn_bf16<{K}>+reduce16[1]", 1, 1, a16=True, b16=True)
    # 17 slabs: group 0 of the reduction takes slabs 0 and 16, the others one -- the `b + 16 u < nslabs` masks
    case(f"tn_bf16/K{K}_M34916", "gemm_tn_bf16", 17 * 2048 + 100, K, K, f"gemm_tn_bf16[{K}x{K}x34916]", f"tn_bf16<{K}>+reduce16[17]", 17, 1,
         a16=True, b16=True)
case("tn_bf16/K64_M133120_65slabs", "gemm_tn_bf16", 65 * 2048, 64, 64, "gemm_tn_bf16[64x64x133120]", "tn_bf16<64>+reduce16[65]", 65, 1,
     a16=True, b16=True)

# ---- lpd_gemm_bf16s: M = 1061 is 34 tiles on 2 blocks = 8 waves (five trips for the first two), the last tile 5 rows
for K in (128, 64):
    for bk in (False, True):
        for M in (100, 32 * 33 + 5):
            case(f"bf16s/K{K}_{'kn' if bk else 'nk'}_M{M}", "gemm_bf16s", M, K, K, f"gemm_bf16s[{M}x{K}x{K}]", f"bf16s<{K},{K}>", 1, 2, a16=True,
                 b_kmajor=bk)

# ---- lpd_edge_dw_sel_bf16 / lpd_edge_dw_sel_f32 (M points, k edges each)
for a16 in (True, False):
    kern = "dw_sel_bf16" if a16 else "dw_sel_tr<0>"
    lab = "edge_dw_sel_" + _T[a16]
    p = 1 if a16 else 3
    case(f"dw_sel/{_T[a16]}_k8_E128", "dw_sel", 16, 128, 128, f"{lab}[128]", f"{kern}+slab_reduce[1]", 1, p, a16=a16, k=8)
    case(f"dw_sel/{_T[a16]}_k20_E640", "dw_sel", 32, 128, 128, f"{lab}[640]", f"{kern}+slab_reduce[1]", 1, p, a16=a16, k=20)
    # two blocks; bf16: 4224 rows a block = 211.2 points: the edges of point 211 straddle the boundary.  fp32: 4160 rows = 208 points
    case(f"dw_sel/{_T[a16]}_k20_M416", "dw_sel", 416, 128, 128, f"{lab}[8320]", f"{kern}+slab_reduce[2]", 2, p, a16=a16, k=20)
    case(f"dw_sel/{_T[a16]}_k64_E512", "dw_sel", 8, 128, 128, f"{lab}[512]", f"{kern}+slab_reduce[1]", 1, p, a16=a16, k=64)
# fp32 storage rounds the rows of a block to 64: M = 416 puts the boundary between two points; M = 432 gives 4352 rows = 217.6 points
case("dw_sel/f32_k20_M432", "dw_sel", 432, 128, 128, "edge_dw_sel_f32[8640]", "dw_sel_tr<0>+slab_reduce[2]", 2, 3, k=20)
case("sw/dw_sel_tr0/f32_k20_M432", "dw_sel", 432, 128, 128, "edge_dw_sel_f32[8640]", "dw_sel_f32+slab_reduce[2]", 2, 3, k=20, sw="dw-sel-tr=0")
case("sw/dw_sel_tr0/f32_k8_E128", "dw_sel", 16, 128, 128, "edge_dw_sel_f32[128]", "dw_sel_f32+slab_reduce[1]", 1, 3, k=8, sw="dw-sel-tr=0")
case("sw/dw_sel_tr2/bf16_k20_M416", "dw_sel", 416, 128, 128, "edge_dw_sel_bf16[8320]", "dw_sel_tr<1>+slab_reduce[2]", 2, 1, a16=True, k=20,
     sw="dw-sel-tr=2")
case("sw/dw_sel_tr2/bf16_k8_E128", "dw_sel", 16, 128, 128, "edge_dw_sel_bf16[128]", "dw_sel_tr<1>+slab_reduce[1]", 1, 1, a16=True, k=8,
     sw="dw-sel-tr=2")

N_CASES = 60      # a case leaves the table only on purpose: tests/test_tn_routes_cpu.py holds this count
SWITCH_SETS = sorted({c["sw"] for c in CASES if c["sw"]})


def _k(c):
    return c["inst"].split("+")[0]


def _nslabs(c):
    return int(c["inst"].split("[")[1][:-1]) if "[" in c["inst"] else 1


# What the table must hold besides one case per instance: (what, predicate, least number of cases)
REQUIRED = [
    ("transposed-read kernel at M = 2048, KA = 256: 8 splits of 8 chunks, every tile width, both A types",
     lambda c: _k(c).startswith("tn_tr<") and _k(c).endswith(",0,0>") and c["M"] == 2048 and c["KA"] == 256 and c["splits"] == 8 and c["nb"] == 1, 6),
    ("transposed-read kernel with an odd chunk count and a short last split", lambda c: _k(c).startswith("tn_tr<") and c["M"] == 2080, 1),
    ("operand transform, plain and batched, both A types", lambda c: c["affine"] and c["KB"] == 64, 4),
    ("operand transform batched over 2 problems of 2048 rows", lambda c: c["affine"] and c["nb"] == 2 and c["M"] == 2048, 2),
    ("bf16 rows on both sides", lambda c: _k(c) == "tn_tr<1,256,0,1>", 1),
    ("transposed-read kernel batched with bf16 A", lambda c: _k(c).startswith("tn_tr<1,") and c["nb"] > 1 and not c["affine"], 1),
    ("128 slabs behind the transposed-read kernel", lambda c: _k(c).startswith("tn_tr<") and _nslabs(c) == 128, 1),
    ("register-transposing kernel at M = 100", lambda c: _k(c).startswith("tn_x3<") and c["M"] == 100, 4),
    ("register-transposing kernel, two splits, ragged last chunk", lambda c: _k(c).startswith("tn_x3<") and c["M"] == 2085 and c["KA"] == 128, 4),
    ("rows = M - 100 on a longer buffer", lambda c: c["extra"] == 100, 2),
    ("fp32 rows batched at KA = 256", lambda c: _k(c) in ("tn_x3<64,0>", "tn_x3<128,0>") and c["nb"] == 3 and c["KA"] == 256 and not c["sw"], 1),
    ("ops.pool_tn", lambda c: c["wrapper"] == "pool_tn", 1),
    ("operands are column slices of a wider buffer", lambda c: c["wrapper"] == "gemm_tn" and c["sliced"], 30),
    ("256 x 256 tiles behind tn-tr=0", lambda c: _k(c).startswith("tn_x3_256<") and c["sw"] == "tn-tr=0" and c["M"] == 8192 and c["splits"] == 8, 2),
    ("register-transposing kernel at KA % 256 == 0, M >= 2048 behind tn-tr=0",
     lambda c: _k(c).startswith("tn_x3<") and c["sw"] == "tn-tr=0" and c["KA"] % 256 == 0 and c["M"] >= 2048, 2),
    ("128-wide kernel at the 256-tile shape behind tn-tr=0,tn256=0", lambda c: c["sw"] == "tn-tr=0,tn256=0" and _k(c) == "tn_x3<128,0>" and c["M"] == 8192, 1),
    ("a split count that tn-blocks=1024 doubles", lambda c: c["sw"] == "tn-blocks=1024", 1),
    ("dw_sel_f32 behind dw-sel-tr=0", lambda c: _k(c) == "dw_sel_f32" and c["sw"] == "dw-sel-tr=0", 1),
    ("dw_sel_tr<1> behind dw-sel-tr=2", lambda c: _k(c) == "dw_sel_tr<1>" and c["sw"] == "dw-sel-tr=2", 1),
    ("gemm_tn_bf16 at M = 100", lambda c: c["wrapper"] == "gemm_tn_bf16" and c["M"] == 100, 2),
    ("gemm_tn_bf16 with 17 slabs", lambda c: c["wrapper"] == "gemm_tn_bf16" and _nslabs(c) == 17, 2),
    ("gemm_tn_bf16 with more than 64 slabs", lambda c: c["wrapper"] == "gemm_tn_bf16" and _nslabs(c) > 64, 1),
    ("gemm_bf16s, both sizes, both layouts, M = 100 and 1061", lambda c: c["wrapper"] == "gemm_bf16s" and c["M"] in (100, 1061), 8),
    ("edge_dw_sel at k = 8, E = 128", lambda c: c["wrapper"] == "dw_sel" and c["k"] == 8 and c["M"] * c["k"] == 128 and not c["sw"], 2),
    ("edge_dw_sel at k = 20, E = 640", lambda c: c["wrapper"] == "dw_sel" and c["k"] == 20 and c["M"] == 32, 2),
    ("edge_dw_sel at k = 20, M = 416", lambda c: c["wrapper"] == "dw_sel" and c["k"] == 20 and c["M"] == 416 and not c["sw"], 2),
    ("edge_dw_sel with a point straddling the block boundary, both storage types",
     lambda c: c["wrapper"] == "dw_sel" and not c["sw"] and c["splits"] == 2 and edge_dw_sel_rows_per_block(c["M"] * c["k"], c["a16"]) % c["k"] != 0, 2),
    ("edge_dw_sel at k = 64", lambda c: c["wrapper"] == "dw_sel" and c["k"] == 64, 2),
]


# ================================================================== every instance the sources build
def _built():
    first = {}
    for c in sorted(CASES, key=lambda c: bool(c["sw"])):       # (stable) the default-switch cases first: a switch is named only where it is needed
        where = c["name"] + (" under LPD_DEBUG=" + c["sw"] if c["sw"] else "")
        first.setdefault(_k(c), where)
        if "+" in c["inst"]:
            first.setdefault(c["inst"].split("+")[1].split("[")[0], where)
    b = {}

    def put(inst, why=None):
        b[inst] = ("reached by " + first[inst]) if inst in first else why

    for kbt in (128, 64):
        for ab in (0, 1):
            put(f"tn_x3<{kbt},{ab}>")
    for ab in (0, 1):
        put(f"tn_x3_256<{ab}>")
    for a16 in (0, 1):
        for tb in (256, 128, 64):
            put(f"tn_tr<{a16},{tb},0,0>")
        put(f"tn_tr<{a16},64,1,0>")
    put("tn_tr<1,256,0,1>")
    for k in (128, 64):
        put(f"tn_bf16<{k}>")
        put(f"bf16s<{k},{k}>")
    for i in ("dw_sel_bf16", "dw_sel_f32", "dw_sel_tr<0>", "dw_sel_tr<1>", "reduce16", "slab_reduce"):
        put(i)
    put("tn_reduce", "not reachable: gemm_tn_reduce_kernel is launched for n % 64 != 0 only, and n = KA * KB with KA % 128 == 0 and KB % 64 == 0 "
        "(lpd_gemm_tn) or KA = KB in {64, 128} (lpd_gemm_tn_bf16); no LPD_DEBUG switch changes that")
    return b


BUILT = _built()
UNREACHABLE = sorted(k for k, v in BUILT.items() if v is None or v.startswith("not reachable"))
SWITCH_ONLY = sorted(k for k, v in BUILT.items() if v and " under LPD_DEBUG=" in v)
