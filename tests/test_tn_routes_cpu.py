"""tests/tn_routes.py against itself, against the sources and against the library's own host functions; what the per-element measure of
tests/test_tn_routes_gpu.py sees that the norm-relative gates of tests/test_ops_gpu.py do not; and that a correct kernel can meet the
bounds (the float32 emulation of each number format does).  Runs without a GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

import tn_checks as tc
import tn_routes as tr
from fp64_checks import SUM_X, U23, X2_TERM, X3_TERM, _scaled, check_bound, half_ulp_bf16, seq_matmul, seq_matmul_x3, split_bf16

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _resolved(c):
    return c["label"], c["inst"], c["splits"], c["prods"]


@pytest.mark.parametrize("name", [c["name"] for c in tr.CASES])
def test_case_resolves_to_its_label_instance_splits_and_products(name):
    c = tr.by_name(name)
    assert tr.route(c) == _resolved(c)


def test_table_is_whole():
    assert len(tr.CASES) == tr.N_CASES
    assert len({c["name"] for c in tr.CASES}) == len(tr.CASES)
    assert tr.SWITCH_SETS == ["dw-sel-tr=0", "dw-sel-tr=2", "tn-blocks=1024", "tn-tr=0", "tn-tr=0,tn256=0"]


@pytest.mark.parametrize("what", [r[0] for r in tr.REQUIRED])
def test_table_holds_what_it_must(what):
    _, pred, least = next(r for r in tr.REQUIRED if r[0] == what)
    have = [c["name"] for c in tr.CASES if pred(c)]
    assert len(have) >= least, (what, have)


def test_stated_shapes_are_what_the_restatement_makes_of_them():
    """the chunk and split arithmetic the case comments state"""
    assert tr.rows_per_split(2048, 8, True) == 256                                    # 8 splits of 8 chunks
    assert tr.rows_per_split(2080, 8, True) == 288 and 2080 - 7 * 288 == 64           # 9 chunks, the last split 2
    assert tr.rows_per_split(2085, 2, False) == 1088 and (2085 - 1088) % 64 == 37
    assert tr.rows_per_split(32768, 128, True) == 256
    assert tr.tn_bf16_rows_per_block(17 * 2048 + 100) == 2112 and tr.tn_bf16_blocks(65 * 2048) == 65
    assert tr.bf16s_grid(100) == 1 and tr.bf16s_grid(32 * 33 + 5) == 2 and tr.cdiv(32 * 33 + 5, 32) == 34
    assert tr.edge_dw_sel_rows_per_block(8320, True) == 4224 and 4224 % 20 != 0
    assert tr.edge_dw_sel_rows_per_block(8320, False) == 4160 and 4160 % 20 == 0      # fp32 storage: the boundary falls between two points
    assert tr.edge_dw_sel_rows_per_block(8640, False) == 4352 and 4352 % 20 != 0
    # the doubled split count, and that the default switches reach neither the 256 kernel nor the 128-wide one at its shape
    c = tr.by_name("sw/tn_blocks1024/x3_f32_512tiles_M2064")
    assert tr.entry_tn(c["M"], c["KA"], c["KB"], 1, False, False, False)[1] * 2 == c["splits"]
    for a16 in (False, True):
        assert tr.entry_tn(8192, 256, 256, 1, a16, False, False)[0].startswith(f"tn_tr<{int(a16)},256,0,0>")
    # every shape gemm_tn_256() accepts, tn_tr_tb() accepts first
    for M in (8192, 8192 + 32, 16384, 1 << 20):
        for KA in (256, 1024):
            for KB in (256, 512):
                assert tr.gemm_tn_256(M, KA, KB, 1) and tr.tn_tr_tb(M, KA, KB, 1, False) == 256 and tr.tn_tr_tb(M, KA, KB, 1, True) == 256


def test_every_built_instance_is_reached_or_explained():
    for inst, why in tr.BUILT.items():
        assert why, f"{inst}: neither reached by a case nor marked unreachable"
        if why.startswith("reached by "):
            name, _, sw = why[len("reached by "):].partition(" under LPD_DEBUG=")
            c = tr.by_name(name)
            assert c["sw"] == sw
            got = tr.route(c)[1]
            assert inst in (got.split("+")[0], got.split("+")[1].split("[")[0] if "+" in got else None), (inst, got)
            if sw:      # a switch is named only where no default-switch case reaches the instance
                assert not any(not x["sw"] and inst in (tr._k(x), x["inst"].split("+")[-1].split("[")[0]) for x in tr.CASES), inst
        else:
            assert why.startswith("not reachable") and len(why) > 60, (inst, why)
            assert not any(inst in (tr._k(c), c["inst"].split("+")[-1].split("[")[0]) for c in tr.CASES), f"{inst} is marked unreachable but a case claims it"
    for c in tr.CASES:
        assert tr._k(c) in tr.BUILT, c["name"]
    assert tr.UNREACHABLE == ["tn_reduce"]
    assert tr.SWITCH_ONLY == ["dw_sel_f32", "dw_sel_tr<1>", "tn_x3_256<0>", "tn_x3_256<1>"]
    assert len(tr.BUILT) == 26


def _b(s):
    return int(s.strip() == "true")


def test_built_list_matches_the_instantiations_in_the_sources():
    t2, t3 = _src("lpd_train2.hip"), _src("lpd_train3.hip")
    impl = t2[t2.index("static int gemm_tn_impl(const void* A_, long long lda, const float* B, long long ldb, float* dW, float* ws, long long M, int KA, int KB,\n"
                       "                        int batch, long long sA, long long sB, int ab_flags"):]
    got = set()
    for m in re.finditer(r"LPD_TN_TR_LAUNCH\((true|false), (\d+), (true|false)\);", impl):
        got.add(f"tn_tr<{_b(m.group(1))},{m.group(2)},{_b(m.group(3))},0>")
    for m in re.finditer(r"hipLaunchKernelGGL\(\(gemm_tn_tr_kernel<(true|false), (\d+), (true|false), (true|false)>\)", impl):
        got.add(f"tn_tr<{_b(m.group(1))},{m.group(2)},{_b(m.group(3))},{_b(m.group(4))}>")
    assert got == {k for k in tr.BUILT if k.startswith("tn_tr<")} and len(got) == 9
    got = {f"tn_x3<{m.group(1)},{_b(m.group(2))}>" for m in re.finditer(r"LPD_TN_LAUNCH\((\d+), (true|false)\);", impl)}
    assert got == {k for k in tr.BUILT if k.startswith("tn_x3<")} and len(got) == 4
    got = {f"tn_x3_256<{_b(m.group(1))}>" for m in re.finditer(r"hipLaunchKernelGGL\(gemm_tn_x3_256_kernel<(true|false)>", impl)}
    assert got == {k for k in tr.BUILT if k.startswith("tn_x3_256<")} and len(got) == 2
    got = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\(gemm_tn_bf16_kernel<(\d+), (\d+)>\)", t2):
        assert m.group(1) == m.group(2)
        got.add(f"tn_bf16<{m.group(1)}>")
    assert got == {k for k in tr.BUILT if k.startswith("tn_bf16<")} and len(got) == 2
    got = {f"bf16s<{m.group(1)},{m.group(2)}>" for m in re.finditer(r"auto kern = gemm_bf16s_kernel<(\d+), (\d+)>;", t2)}
    assert got == {k for k in tr.BUILT if k.startswith("bf16s<")} and len(got) == 2
    got = {f"dw_sel_tr<{_b(m.group(1))}>" for m in re.finditer(r"hipLaunchKernelGGL\(edge_dw_sel_tr_kernel<(true|false)>", t3)}
    assert got == {k for k in tr.BUILT if k.startswith("dw_sel_tr<")} and len(got) == 2
    assert "hipLaunchKernelGGL(edge_dw_sel_bf16_kernel," in t3 and "hipLaunchKernelGGL(edge_dw_sel_f32_kernel," in t3
    # the reductions: reduce16 wherever n % 64 == 0, the plain kernel otherwise; the transposed-read route does not even ask
    assert len(re.findall(r"if \(n % 64 == 0\) hipLaunchKernelGGL\(gemm_tn_reduce16_kernel,", t2)) == 3
    assert len(re.findall(r"else hipLaunchKernelGGL\(gemm_tn_reduce_kernel,", t2)) == 3
    assert len(re.findall(r"hipLaunchKernelGGL\(gemm_tn_reduce(16)?_kernel,", t2)) == 7
    assert len(re.findall(r"hipLaunchKernelGGL\(slab_reduce_kernel,", t3)) == 2


def test_restated_constants_and_conditions_are_those_of_the_sources():
    t2, t3 = _src("lpd_train2.hip"), _src("lpd_train3.hip")
    for text in (
            'static const bool on = lpd_debug("tn256", 1) != 0;',
            f"return on && batch == 1 && KA % 256 == 0 && KB % 256 == 0 && M % 32 == 0 && M >= {tr.T256_MIN_M};",
            'static const bool on = lpd_debug("tn-tr", 1) != 0;',
            f"if (KA % 256 != 0 || KB % 64 != 0 || M % {tr.TR_CHUNK} != 0 || M < {tr.TR_MIN_M}) return 0;",
            "if (act) return KB % 256 == 0 ? 256 : (KB % 128 == 0 ? 128 : 64);\n    if (!on) return 0;",
            "if (!a_bf16 && batch > 1) return 0;",
            f"const long long tiles = (long long)(KA / 256) * (KB / tb) * batch, cap = (tb == 256 || !a_bf16) ? {tr.TR_CAP_ONE} : {tr.TR_CAP_TWO};",
            f"while (tiles * splits * 2 <= cap && M / (splits * 2) >= {tr.TR_SPLIT_ROWS}) splits *= 2;",
            "const long long tiles = (long long)(KA / 256) * (KB / 256);",
            f"while (tiles * splits * 2 <= 256 && M / (splits * 2) >= {tr.X3_SPLIT_ROWS}) splits *= 2;",
            "long long tiles = (long long)(KA / 128) * ((KB + 127) / 128) * batch;",
            f'static const int cap = lpd_debug("tn-blocks", {tr.TN_BLOCKS});',
            f"while (tiles * splits * 2 <= cap && M / (splits * 2) >= {tr.X3_SPLIT_ROWS}) splits *= 2;",
            f"rps = (rps + {tr.X3_CHUNK - 1}) / {tr.X3_CHUNK} * {tr.X3_CHUNK};",
            f"rps = (rps + {tr.TR_CHUNK - 1}) / {tr.TR_CHUNK} * {tr.TR_CHUNK};",
            "LPD_CHECK_ARG(KA > 0 && KA % 128 == 0 && KB > 0 && KB % 64 == 0,",
            "LPD_CHECK_ARG(!b_bf16 || (a_bf16 && !a_scale && batch == 1 && tn_tr_tb(M, KA, KB, batch, true, true) == 256),",
            "const bool act = a_scale != nullptr || b_bf16;",
            "LPD_CHECK_ARG(!act || tn_tr_tb(M, KA, KB, batch, a_bf16 != 0, true),",
            'LPD_CHECK_ARG(tb == 64, "lpd_gemm_tn_act: built for KB %% 128 != 0 (64-wide b tiles), KB=%d", KB);',
            "const int kbt = KB % 128 == 0 ? 128 : 64;",
            "const long long a = gemm_tn_splits(M, KA, KB, batch, true), b = gemm_tn_splits(M, KA, KB, batch, false);",
            "return gemm_tn_splits(M, KA, KB, batch, a_bf16 != 0, true) * batch * KA * KB;",
            f"const long long blocks = M / {tr.TNBF16_ROWS} > {tr.TNBF16_MAX} ? {tr.TNBF16_MAX} : (M / {tr.TNBF16_ROWS} < 1 ? 1 : M / {tr.TNBF16_ROWS});",
            "rpb = (rpb + 63) / 64 * 64;",
            'LPD_CHECK_ARG((KA == 128 && KB == 128) || (KA == 64 && KB == 64), "lpd_gemm_tn_bf16: built for 128 x 128 and 64 x 64");',
            "LPD_CHECK_ARG((N == 128 && K == 128) || (N == 64 && K == 64),",
            f"const int grid = grid_for((M + {tr.BF16S_WAVE_ROWS - 1}) / {tr.BF16S_WAVE_ROWS}, 4 * 8, {tr.BF16S_CAP});",
            "const long long ntile = (M + 31) / 32;"):
        assert text in t2, text
    assert tr.BF16S_PER_BLOCK == 4 * 8
    for text in (
            'static const bool on = lpd_debug("dw-sel-tr", 1) != 0;',
            'static const bool tr16 = lpd_debug("dw-sel-tr", 1) == 2;',
            f"long long b = E / {tr.DWSEL_ROWS};\n    return b > {tr.DWSEL_MAX} ? {tr.DWSEL_MAX} : (b < 1 ? 1 : b);",
            "rpb = (rpb + 127) / 128 * 128;",
            "rpb = (rpb + 63) / 64 * 64;",
            "return edge_dw_sel_blocks(E) * (256 * 128 + 128) * (long long)sizeof(float) + (256 * 128 + 128) * (long long)sizeof(double);",
            "if (tr16 && E < (1ll << 32)) {",
            "if (edge_dw_sel_tr() && E < (1ll << 32)) {",
            'LPD_CHECK_ARG(k >= 8 && k <= 255 && ldw >= 128, "lpd_edge_dw_sel_bf16:',
            "LPD_CHECK_ARG((M * k) % 128 == 0,",
            "LPD_CHECK_ARG((M * k) % 64 == 0,"):
        assert text in t3, text
    assert tr.DWSEL_SLAB == 256 * 128 + 128
    with open(os.path.join(ROOT, "lpd-net-pytorch_amd", "lpdnet_hip", "ops.py")) as f:
        o = f.read()
    for text in (
            "return (GEMM_TN and GEMM_BF16X3 and _EXACT.depth == 0 and KA % 256 == 0 and KB % 64 == 0 and KB % 128 != 0 and M % 32 == 0 and M >= 2048",
            "if rows is not None or not gemm_tn_act_applies(A, B):",
            "if not a16 or B.dim() != 2 or B.stride(1) != 1 or B.stride(0) % 8 != 0 or a_affine is not None:",
            "return (GEMM_TN and GEMM_BF16X3 and _EXACT.depth == 0 and A.dim() == 2 and B.dim() == 2 and A.shape[1] % 128 == 0\n"
            f"            and B.shape[1] % 64 == 0 and rows >= {tr.TN_APPLIES_ROWS} and",
            f"if (GEMM_TN and GEMM_BF16X3 and _EXACT.depth == 0 and E % 128 == 0 and K % 64 == 0 and N >= {tr.POOL_MIN_N} and feat3.is_contiguous()",
            '_call(f"gemm_tn+act[{KA}x{KB}x{M}]" + (f"x{nb}" if nb > 1 else ""), lib.lpd_gemm_tn_act,',
            '_call(f"gemm_tn[{KA}x{KB}x{M}]" + (f"x{nb}" if nb > 1 else ""), lib.lpd_gemm_tn,',
            '_call(f"gemm_tn_bf16[{KA}x{KB}x{M}]", lib.lpd_gemm_tn_bf16,',
            '_call(f"gemm_bf16s[{M}x{N}x{K}]", lib.lpd_gemm_bf16s,',
            '_call(f"edge_dw_sel_bf16[{M * k}]", lib.lpd_edge_dw_sel_bf16,',
            '_call(f"edge_dw_sel_f32[{M * k}]", lib.lpd_edge_dw_sel_f32,'):
        assert text in o, text


def test_wrapper_conditions():
    assert tr.gemm_tn_act_applies(2048, 256, 64) and not tr.gemm_tn_act_applies(2048, 256, 128) and not tr.gemm_tn_act_applies(2016, 256, 64)
    assert not tr.gemm_tn_act_applies(2048, 128, 64) and not tr.gemm_tn_act_applies(2080 + 16, 256, 64)
    assert tr.gemm_tn_applies(128, 64, 4096) and not tr.gemm_tn_applies(128, 64, 4095) and not tr.gemm_tn_applies(64, 64, 8192)
    assert tr.pool_tn_applies(256, 128, 64) and not tr.pool_tn_applies(255, 128, 64) and not tr.pool_tn_applies(256, 128, 32)
    c = dict(tr.by_name("tr/act_f32"))
    assert tr.route(dict(c, KB=128)) is None and tr.route(dict(c, extra=100)) is None and tr.route(dict(c, M=2000)) is None
    c = dict(tr.by_name("tr/bf16_bf16_M2048"))
    assert tr.route(dict(c, a16=False)) is None and tr.route(dict(c, nb=2)) is None and tr.route(dict(c, KB=128)) is None
    assert tr.route(dict(c, sw="tn-tr=0")) == _resolved(c)        # bf16 rows on both sides ignore the switch, like the transform
    assert tr.route(dict(tr.by_name("tr/act_bf16"), sw="tn-tr=0"))[1] == "tn_tr<1,64,1,0>+reduce16[8]"


def test_a_changed_threshold_names_the_cases_that_lose_their_route(monkeypatch):
    monkeypatch.setattr(tr, "TR_MIN_M", 4096)
    lost = [c["name"] for c in tr.CASES if tr.route(c) != _resolved(c)]
    assert "tr/f32_KB256_M2048" in lost and "tr/act_bf16" in lost and "x3/f32_KB128_M100" not in lost
    monkeypatch.setattr(tr, "TR_MIN_M", 2048)
    monkeypatch.setattr(tr, "DWSEL_ROWS", 8192)
    lost = [c["name"] for c in tr.CASES if tr.route(c) != _resolved(c)]
    assert "dw_sel/bf16_k20_M416" in lost


# ------------------------------------------------------------------ the library's own host functions
def _grid():
    Ms = sorted({m + d for m in (32, 100, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 1 << 20) for d in (-32, -1, 0, 1, 32, 37)} - {0, -1})
    shapes = [(KA, KB) for KA in (128, 256, 384, 512, 1024, 8192) for KB in (64, 128, 192, 256, 512, 1024)]
    return [(M, KA, KB, nb) for M in Ms if M > 0 for KA, KB in shapes for nb in (1, 2, 3, 44, 64)]


def host_mismatches(lib, sw=""):
    """grid points at which the restatement and the library disagree (host arithmetic only: no GPU call)"""
    s = tr.switches(sw)
    bad = []
    for M, KA, KB, nb in _grid():
        if lib.lpd_gemm_tn_ws_floats(M, KA, KB, nb) != tr.tn_ws_floats(M, KA, KB, nb, s):
            bad.append(("tn", M, KA, KB, nb))
        for a16 in (0, 1):
            if lib.lpd_gemm_tn_act_ws_floats(M, KA, KB, nb, a16) != tr.tn_act_ws_floats(M, KA, KB, nb, a16, s):
                bad.append(("tn_act", M, KA, KB, nb, a16))
    for M in [1, 100, 2047, 2048, 4095, 4096, 17 * 2048 + 100, 65 * 2048, 1024 * 2048 - 1, 1024 * 2048, 1025 * 2048, 1 << 33]:
        for K in (64, 128):
            if lib.lpd_gemm_tn_bf16_ws_floats(M, K, K) != tr.tn_bf16_ws_floats(M, K, K):
                bad.append(("tn_bf16", M, K))
    for E in [128, 640, 4095, 4096, 8191, 8192, 8320, 8640, 256 * 4096 - 128, 256 * 4096, 257 * 4096, 1 << 33]:
        if lib.lpd_edge_dw_sel_bf16_ws_bytes(E) != tr.edge_dw_sel_ws_bytes(E):
            bad.append(("dw_sel", E))
    return bad


def test_split_and_block_counts_equal_what_the_library_reports():
    from lpdnet_hip import _lib
    assert not any(t in os.environ.get("LPD_DEBUG", "") for t in ("tn-tr", "tn256", "tn-blocks")), "the default switches are the ones restated"
    assert host_mismatches(_lib.load()) == []
    # the grid moves every threshold: each route and each cap is the binding one somewhere
    routes = set()
    for M, KA, KB, nb in _grid():
        for a16 in (False, True):
            e = tr.entry_tn(M, KA, KB, nb, a16, False, False)
            routes.add((e[0].split("<")[0], e[1]))
    assert {k for k, _ in routes} == {"tn_tr", "tn_x3"} and {s for _, s in routes} >= {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}


@pytest.mark.parametrize("sw", ["tn-tr=0", "tn-tr=0,tn256=0", "tn-blocks=1024"])
def test_split_counts_under_the_switches_equal_what_the_library_reports(sw):
    """the library reads LPD_DEBUG once, so a fresh interpreter asks (host arithmetic only)"""
    code = ("import test_tn_routes_cpu as t; from lpdnet_hip import _lib; bad = t.host_mismatches(_lib.load(), %r); print('mismatches', bad[:8]); "
            "raise SystemExit(1 if bad else 0)" % sw)
    env = dict(os.environ, LPD_DEBUG=sw, PYTHONPATH=os.pathsep.join([HERE, os.path.join(ROOT, "lpd-net-pytorch_amd")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches []" in r.stdout, r.stdout + r.stderr
    s = tr.switches(sw)
    assert any(tr.tn_ws_floats(*g, s) != tr.tn_ws_floats(*g) for g in _grid()), "the switch changes no workspace of the grid"


# ------------------------------------------------------------------ the measure has teeth
def _rel(got, ref):
    """the gate of tests/test_ops_gpu.py"""
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def _worst(got, ref, f32, scale, term, round16=False):
    """(largest |got - ref| / bound over the elements, as check_bound forms the bound)"""
    ref, s = ref.double(), scale.double().clamp_min(1e-300)
    floor = max(_scaled(f32, ref, scale, exact_zero=False), U23)
    bound = torch.full_like(ref, term + SUM_X * floor)
    if round16:
        bound = bound + half_ulp_bf16(ref.abs() + bound * s) / s
    return ((got.double() - ref).abs() / s / bound).max().item()


def test_the_measure_sees_what_the_norm_relative_gates_let_through():
    """float32 emulations of dW = A^T B and of gemm_bf16s on the graded inputs, one seeded defect at a time.  Each leaves the per-element
    bound of tests/test_tn_routes_gpu.py and stays inside the gate tests/test_ops_gpu.py holds the kernel by today (_rel < 2e-5 for the
    fp32 results, _rel < 6e-3 for the bf16 result of gemm_bf16s); the undamaged emulation stays inside the bound."""
    g = torch.Generator().manual_seed(7)
    M, KA, KB = 2048, 128, 64
    A = torch.randn(M, KA, generator=g) * tc.grade(KA, 13)
    B = torch.randn(M, KB, generator=g) * tc.grade(KB, 7)
    small = (torch.arange(KA) % 13) == 12                   # the A columns of the smallest grade
    # 1: fp32 x fp32, three products; the a_lo b_hi product dropped for the small columns
    ref, scale, f32 = A.double().t() @ B.double(), A.double().abs().t() @ B.double().abs(), seq_matmul(A.t(), B)
    good = seq_matmul_x3(A.t(), B, 3)
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(B)
    bad = good.clone()
    bad[small] = (seq_matmul(ah.t(), bh) + seq_matmul(ah.t(), bl))[small]
    w0, w1 = _worst(good, ref, f32, scale, X3_TERM), _worst(bad, ref, f32, scale, X3_TERM)
    print(f"MEASURE teeth/a_lo_b_hi_dropped correct={w0:.3f} seeded={w1:.1f} of the bound, rel={_rel(bad, ref):.2e}")
    assert w0 <= 1.0 and w1 > 10.0 and _rel(bad, ref) < 2e-5
    # 2: bf16 A, two products; a stale lo image (that of the fp32 tensor the rows were rounded from) multiplied in for the small columns
    A16 = A.bfloat16().float()
    ref, scale, f32 = A16.double().t() @ B.double(), A16.double().abs().t() @ B.double().abs(), seq_matmul(A16.t(), B)
    good = seq_matmul_x3(A16.t(), B, 3)
    bad = good.clone()
    bad[small] = (good + seq_matmul(al.t(), bh))[small]
    w0, w1 = _worst(good, ref, f32, scale, X2_TERM), _worst(bad, ref, f32, scale, X2_TERM)
    print(f"MEASURE teeth/stale_a_lo correct={w0:.3f} seeded={w1:.1f} of the bound, rel={_rel(bad, ref):.2e}")
    assert w0 <= 1.0 and w1 > 10.0 and _rel(bad, ref) < 2e-5
    # 3: gemm_bf16s; the lo image of W dropped in one 32-column tile
    c = tr.by_name("bf16s/K128_nk_M1061")
    d = tc.make_inputs(c)
    ref, scale, f32 = tc.reference(c, d)
    good = tc.emulate(c, d)
    wh, _ = split_bf16(d["W"])
    bad = good.clone()
    bad[:, 32:64] = seq_matmul(d["A"], wh).bfloat16().float()[:, 32:64]
    w0, w1 = _worst(good, ref, f32, scale, X2_TERM, True), _worst(bad, ref, f32, scale, X2_TERM, True)
    print(f"MEASURE teeth/w_lo_dropped_in_a_tile correct={w0:.3f} seeded={w1:.1f} of the bound, rel={_rel(bad, ref):.2e}")
    assert w0 <= 1.0 and w1 > 2.0 and _rel(bad, ref) < 6e-3


@pytest.mark.parametrize("name", [c["name"] for c in tr.CASES if not c["sw"] and c["M"] <= 4096])
def test_the_emulation_of_the_number_format_meets_the_bound(name):
    """three, two or one product per term accumulated in sequence in float32 (with the transform's re-rounding, the bf16 store) stays
    inside the bound the GPU test asserts for the case: a correct kernel can meet it"""
    c = tr.by_name(name)
    d = tc.make_inputs(c)
    ref, scale, f32 = tc.reference(c, d)
    check_bound(name, tc.emulate(c, d), ref, f32, scale, tc.term_of(c), round16=c["wrapper"] == "gemm_bf16s", what="tn-emu")
