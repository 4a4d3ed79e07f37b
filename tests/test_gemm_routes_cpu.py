"""tests/gemm_routes.py against itself and against the sources, and what the per-element measure of tests/test_gemm_routes_gpu.py sees that
the norm-relative measure of tests/test_ops_gpu.py does not.  Runs without a GPU."""
import os
import re

import pytest
import torch

import gemm_routes as gr
from fp64_checks import LEAKY, SLOPE, SUM_X, U23, X3_TERM, _act, _act_scale, _scaled, half_ulp_bf16, seq_matmul, seq_matmul_x3

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lpd-net-pytorch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constexpr(src, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, name
    return int(m.group(1))


@pytest.mark.parametrize("name", [c["name"] for c in gr.CASES])
def test_case_resolves_to_its_label_and_instance(name):
    c = gr.by_name(name)
    assert gr.route(c) == (c["label"], c["inst"])


def test_table_is_whole():
    assert len(gr.CASES) == gr.N_CASES
    assert len({c["name"] for c in gr.CASES}) == len(gr.CASES)


@pytest.mark.parametrize("what", [r[0] for r in gr.REQUIRED])
def test_table_holds_what_it_must(what):
    _, pred, least = next(r for r in gr.REQUIRED if r[0] == what)
    have = [c["name"] for c in gr.CASES if pred(c)]
    assert len(have) >= least, (what, have)


def test_every_built_instance_is_reached_or_explained():
    names = {c["name"] for c in gr.CASES}
    for inst, why in gr.BUILT.items():
        assert why, f"{inst}: neither reached by a case nor marked unreachable"
        if why.startswith("reached by "):
            c = gr.by_name(why[len("reached by "):])
            assert c["name"] in names
            got = gr.route(c)[1]
            assert inst in (got.split("+")[0], "splitk_reduce" + got[got.index("+"):] if "+" in got else None), (inst, got)
        else:
            assert why.startswith("not reachable through a wrapper: ") and len(why) > 60, (inst, why)
            assert not any(c["inst"].split("+")[0] == inst for c in gr.CASES), f"{inst} is marked unreachable but a case claims it"
    # every instance a case claims is one the sources build
    for c in gr.CASES:
        assert c["inst"].split("+")[0] in gr.BUILT, c["name"]


def test_built_list_matches_the_instantiations_in_the_sources():
    """the explicit template arguments the launch code names: x3t_launch<..>, gemm_p8_kernel<..> outside the timing-only block, the bf16
    modes of x3w_wide_launch_kc<..> and the panel / layout switches of the generic kernels"""
    t = _src("lpd_gemm_t.hip")
    x3t = set()
    for m in re.finditer(r"x3t_launch<([^>]*)>\(g", t):
        a = [s.strip() for s in m.group(1).split(",")]
        x3t.add(f"x3t<{a[0]},{int(len(a) > 1 and a[1] == 'true')},{a[2] if len(a) > 2 else gr.X3T_ROWS_PER_WG}>")
    assert x3t == {k for k in gr.BUILT if k.startswith("x3t<")}
    p = _src("lpd_gemm_p8.hip")
    p = p[:p.index("#ifdef LPD_P8_BENCH")] + p[p.index("#else", p.index("#ifdef LPD_P8_BENCH")):]
    p8 = set()
    for m in re.finditer(r"launch\(gemm_p8_kernel<([^>]*)>\)", p):
        a = [s.strip() for s in m.group(1).split(",")]
        assert len(a) < 3 or a[2] == "0"
        p8.add(f"p8<{a[0]},{int(a[1] == 'true')},{int(len(a) > 3 and a[3] == 'true')}>")
    assert p8 == {k for k in gr.BUILT if k.startswith("p8<")}
    g = _src("lpd_gemm.hip")
    modes = set()
    for m in re.finditer(r"x3w_wide_launch_kc<(\d), 0, 32, (true|false), (\d)>\(g", g):
        modes.add(f"x3w<{m.group(1)},0,0,32,{int(m.group(2) == 'true')},{m.group(3)}>")
    assert modes == {k for k in gr.BUILT if k.startswith("x3w<") and not k.endswith(",0>") and ",0,0,32," in k and k[6] == "0"}
    assert set(re.findall(r"x3w_wide_launch<(\d), (\d)>\(g", g)) == {(str(w), str(q)) for w in (1, 2) for q in range(4)}
    assert set(re.findall(r"gemm_panel_launch<(true|false), (\d)>\(g", g)) == {(b, str(q)) for b in ("true", "false") for q in (1, 2, 3)}
    assert re.search(r"LPD_FEWROWS\(1\);.*LPD_FEWROWS\(2\);.*LPD_FEWROWS\(4\);", g, re.S)
    assert [int(x) for x in re.findall(r"LPD_SMALLM\((\d)\);", g)] == [1, 2, 3, 4]


def test_restated_constants_are_those_of_the_sources():
    g, t = _src("lpd_gemm.hip"), _src("lpd_gemm_t.hip")
    assert gr.GEMM_BK == _constexpr(g, "GEMM_BK")
    assert gr.SMALLM_KC == _constexpr(g, "SMALLM_KC")
    assert gr.FR_KPER == _constexpr(g, "FR_KPER")
    assert gr.R32_KPER == _constexpr(g, "R32_KPER")
    assert gr.FR_MAXM == _constexpr(g, "FR_MAXM")
    assert gr.X3T_ROWS_PER_WG * 2 == _constexpr(t, "XT_THREADS")
    m = re.search(r"template <int KS, bool ROWS = false, int RB = (\d+)>", t)
    assert m and int(m.group(1)) == gr.X3T_ROWS_PER_WG
    m = re.search(r'lpd_debug\("x3t-rb", (\d+)\)', t)
    assert m and int(m.group(1)) == gr.X3T_RB_BF16 and f"x3t_launch<8, true, {gr.X3T_RB_BF16}>" in t
    # the conditions the restatement carries, as the sources spell them
    assert "const int tn = N > 64 ? 2 : 1;" in g
    assert "batch == 1 && splits >= 64 && splits % 16 == 0" in g
    assert "M <= 64 && g.K == SMALLM_KC" in g
    assert "if (impl == 0) impl = N >= 256 ? 3 : 2;" in g
    assert "if (NT <= 2) { x3w_wide_launch_kc<1, PANELS, 32, true>" in g


def test_a_changed_threshold_names_the_cases_that_lose_their_route(monkeypatch):
    """the table is held to the restatement: moving a threshold makes cases resolve elsewhere"""
    monkeypatch.setattr(gr, "FR_MAXM", 2)
    lost = [c["name"] for c in gr.CASES if gr.route(c) != (c["label"], c["inst"])]
    assert "fewrows/M3_N256_K8200" in lost and "fewrows/M4_N512_K8192" in lost
    monkeypatch.setattr(gr, "FR_MAXM", 4)
    monkeypatch.setattr(gr, "X3_MIN", 64)
    lost = [c["name"] for c in gr.CASES if gr.route(c) != (c["label"], c["inst"])]
    assert "f32/fast_call_N72" in lost


# ------------------------------------------------------------------ the measure has teeth
def _graded(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * (2.0 ** -(torch.arange(M) % 13).float()).view(M, 1)
    W = torch.randn(K, N, generator=g) * (2.0 ** -(torch.arange(N) % 7).float()).view(1, N)
    return A, W


def _rel(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def _measure(got, ref, f32, scale):
    floor = max(_scaled(f32, ref, scale, exact_zero=False), U23)
    return _scaled(got, ref, scale, exact_zero=False), X3_TERM + SUM_X * floor


TEETH = ["x3/nt_K64", "x3w/N264_K264_nk", "x3/nt_K1024"]


@pytest.mark.parametrize("name", TEETH)
def test_the_measure_sees_what_the_norm_relative_one_lets_through(name):
    """A float32 emulation of the three-product form stays inside the GPU test's bound; a small row computed as a plain bf16 product, a
    negative LeakyReLU branch fed from the single product and one k element dropped from a small column all leave it -- the first two by
    more than 10 x while max|a - b| / max|b| stays under the 3e-5 that tests/test_ops_gpu.py asserts for these kernels.  The shapes are
    those of three cases of the table."""
    c = gr.by_name(name)
    M, N, K = c["M"], c["N"], c["K"]
    A, W = _graded(M, N, K, M + N + K)
    pre, terms = A.double() @ W.double(), A.double().abs() @ W.double().abs()
    f32, x3, x1 = seq_matmul(A, W), seq_matmul_x3(A, W, 3), seq_matmul_x3(A, W, 1)
    err, bound = _measure(x3, pre, f32, terms)
    print(f"MEASURE teeth/{M}x{N}x{K} correct err={err:.3e} bound={bound:.3e} rel={_rel(x3, pre):.3e}")
    assert err <= bound
    # 1: one row of scale 2^-12 keeps ah bh only
    mut = x3.clone()
    mut[12] = x1[12]
    e1, _ = _measure(mut, pre, f32, terms)
    print(f"MEASURE teeth/{M}x{N}x{K} small-row-x1 err={e1:.3e} bound={bound:.3e} rel={_rel(mut, pre):.3e}")
    assert e1 >= 10 * bound and _rel(mut, pre) < 3e-5
    # 2: the negative LeakyReLU branch from the single product
    ref, scale = _act(pre, LEAKY), _act_scale(pre, terms, LEAKY)
    good = _act(x3, LEAKY)
    mut = torch.where(x3 > 0, x3, x1 * SLOPE)
    f32a = _act(f32, LEAKY)
    e0, b2 = _measure(good, ref, f32a, scale)
    e2, _ = _measure(mut, ref, f32a, scale)
    print(f"MEASURE teeth/{M}x{N}x{K} leaky-x1 err={e2:.3e} bound={b2:.3e} rel={_rel(mut, ref):.3e}")
    assert e0 <= b2 and e2 >= 10 * b2 and _rel(mut, ref) < 3e-5
    # 3: one k element dropped from one small-scale column (n % 7 == 6)
    mut = x3.clone()
    mut[:, 6] = seq_matmul_x3(A[:, :K - 1], W[:K - 1, 6:7], 3)[:, 0]
    e3, _ = _measure(mut, pre, f32, terms)
    print(f"MEASURE teeth/{M}x{N}x{K} dropped-k err={e3:.3e} bound={bound:.3e} rel={_rel(mut, pre):.3e}")
    assert e3 > bound


def test_half_an_ulp_of_bf16_is_not_two_to_the_minus_nine():
    """the allowance of a bf16 result: torch's round-to-nearest of float32 values stays within 2^(floor(log2 |v|) - 8), reaches it, and
    passes 2^-9 |v| (at the bottom of a binade half an ulp is 2^-8 |v|)"""
    v = torch.randn(1 << 16, generator=torch.Generator().manual_seed(1)) * 3
    v = torch.cat([v, torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -8 - 2.0 ** -20, 1.9999, 3.0])])
    d = (v.bfloat16().double() - v.double()).abs()
    assert bool((d <= half_ulp_bf16(v)).all())
    assert bool((d > 2.0 ** -9 * v.double().abs()).any())
    assert (d / half_ulp_bf16(v)).max().item() > 0.99
