"""Every GEMM route (csrc/lpd_gemm.hip, csrc/lpd_gemm_t.hip, csrc/lpd_gemm_p8.hip) per element against float64 on the CPU, at the smallest
shape at which the route can still go wrong.  tests/gemm_routes.py holds the table of cases and says which kernel instance each one runs;
tests/test_gemm_routes_cpu.py checks that statement against a restatement of the dispatch and shows what the measure sees.

Each case
  - calls the lpdnet_hip.ops wrapper with ops.PROFILE set and asserts the label of the case -- `gemmx3[..]`, not `gemm[..]` -- so that a
    case cannot run another route than its name says;
  - draws A and W from a seeded CPU generator with GRADED scales: row i of A times 2^-(i % 13), column n of W times 2^-(n % 7) (a
    norm-relative measure cannot see an error on a small row or column; randn inputs have none); row 5 of A is zero; the epilogue has a
    bias and a shift on about half of the columns and a scale on all, about 30 % of them negative; operand rows are padded to a multiple
    of 4 floats and the padding holds 1e4, so a k tail that reads it shows;
  - compares with float64: pre = A W, terms = |A| |W|, the epilogue written out; the scale of an element is (terms + |bias|) |scale| + |shift|
    taken through the activation (fp64_checks._act_scale; its kink rule with the width derived below), plus |C| where the call accumulates;
  - takes the float32 FLOOR from a float32 accumulation in sequence over k (K rank-1 updates, fp64_checks.seq_matmul) with the same
    epilogue in float32, scaled like the error, never below 2^-23;
  - asserts |got - ref| <= (TERM + 2 floors) * scale per element, that an element whose scale is 0 is exactly 0, and that everything
    outside the output kept its fill value bit for bit: an output slice has 8 guard columns on either side and 4 guard rows above and
    below EVERY problem (so a store past a ragged last row tile, or into the next problem of a batch, shows), a panel output has guard
    panels and its own pad rows; every kernel family has at least one sliced case;
  - prints `MEASURE gemm/<case> err=.. floor=.. bound=..` (units of the scale, at the element closest to its bound).

TERM comes from the number format, never from what the kernels give.  The bf16 figures below take |a - bf16(a)| <= 2^-9 |a|, which is how
X3_TERM = 3 * 2^-18 of tests/test_fwd_ops_gpu.py was set and what this module was asked to assert.  That is NOT the worst case: round to
nearest on an 8-bit significand errs by up to half an ulp, 2^-8 |a| at the bottom of a binade (see `bf16 result`), so the worst case of
the three-product form is 3 * 2^-16, of the single product 2 * 2^-8 + 2^-16, of the two-product form 2^-16.  Over a sum of K terms with
operands spread over their binades the errors do not line up, and the kernels measure at half of the asserted figures or less; a product
of few terms whose operands all sit just above a power of two could pass 3 * 2^-18 with a correct kernel.  A later failure between the
asserted figure and the worst case on such inputs is to be read as that, not as a wrong kernel.
  f32    f32-input MFMA and fp32 FMA routes, split-K slabs included: 0 -- only the summation order differs from the in-sequence sum
         (SUM_X = 2 floors, as the sums of tests/test_fwd_ops_gpu.py).
  x3     split bf16, three products: a = ah + al + ra with |al| <= 2^-9 |a|, |ra| <= 2^-18 |a| (bf16 keeps 8 significant bits, round to
         nearest); a b - (ah bh + ah bl + al bh) = al bl + ra b + a rb - .. <= 3 * 2^-18 |a b| = X3_TERM.
  x1     one product ah bh: |a - ah| <= 2^-9 |a| for both operands: 2 * 2^-9 + 2^-18.
  x2     bf16 rows are the EXACT inputs (the test makes the bf16 values first), two products against the split weight: only the weight's
         residual rb is lost: 2^-18.
  split planes (lpd_gemm_x3ts, lpd_gemm_p8): the planes hi, lo are the exact inputs, a = hi + lo; three products lose lo * bl and the
         weight's residual: 2 * 2^-18 <= X3_TERM, which is what is asserted.
  bf16 result: the fp32 accumulator v, within e of ref (e the bound of the accumulator), is rounded to bf16: half an ulp.  Half an ulp of
         an 8-bit significand at v is 2^(floor(log2 |v|) - 8): 2^-9 |v| only at the top of a binade, 2^-8 |v| at its bottom (1 + 2^-8 rounds
         to 1: tests/test_gemm_routes_cpu.py shows torch's own rounding passing 2^-9 |v| and never half an ulp), so the bound is
         e + 2^(floor(log2(|ref| + e)) - 8), not e + 2^-9 |ref|.
  kink of an activation: fp64_checks._act_scale gives an element within 2^-20 terms of the kink the full scale, because either side is a
         correct rounding there.  A pre-activation of a route is only good to TERM terms, so the distance is 2^-20 + TERM for every
         route: 2^-20 for f32 routes, 1.2e-5 for three products (a ReLU element with |pre| = 5e-6 terms may come out 0 or not), 3.9e-3
         for a single product (a LeakyReLU element with |pre| = 1e-3 terms may come out on either branch).
Terms the list above does not have, derived the same way:
  operand transform (gemm_act, gemm(a_affine=)): x' = act(s x + t) is evaluated in fp32 in the loader: three roundings of 2^-24 (product,
         sum, slope) relative to its own terms |s x| + |t|.  Where the map is stored (gemm_act(store=True)) the STORED values are the
         product's exact inputs and the map itself is checked against float64 as an f32 route (a bf16 map with the bf16-result rule);
         gemm_act(store=False) must give bit for bit the product of the storing call.  Where nothing is stored (a_affine) the product is
         scaled by terms(x') |W| and TERM grows by 2^-22; bf16 rows there are rounded to bf16 again after the transform, unobservably, so
         the unrounded map is the exact input and TERM is 2^-9 + 2^-18 + 2^-22 (2^-9 with the convention above); the float32 floor of
         that case takes the UNROUNDED float32 map, so the rounding is counted once, in TERM.
  lpd_gemm_p8 folds `scale` into the weight with one fp32 multiplication in torch; the same multiplication on the CPU gives the same
         bits, and the folded weight is the reference's input (no term).
  column sums of linear_bn_stats: sum_m y[m][n] against the float64 column sums of the float64 product, scaled by the column sum of the
         elements' scales, TERM of the product plus 2 floors of an in-sequence float32 column sum of the float32 product; sums of squares
         scaled by sum_m scale^2 with (1 + TERM)^2 - 1 (y^2 moves by 2 y e + e^2).
  fused assignment product of lpd_gemm_p8_fused: parts[j] = C[:, 256 j : 256 j + 256] W2[256 j : 256 j + 256] takes the kernel's own fp32 C
         (read back) as its exact input: a three-product route, X3_TERM.
"""
import pytest
import torch

import gemm_routes as gr
from fp64_checks import AFFINE_TERM, NONE, SLOPE, X1_TERM, X2_TERM, X3_TERM, _act, _act_scale, _seqsum, check_bound, seq_matmul

pytestmark = pytest.mark.gpu

PAD = 1e4          # what operand padding and unused panels hold
FILL = -7.0        # what the surroundings of an output hold


def _ops():
    from lpdnet_hip import ops
    return ops


def _r4(n):
    return (n + 3) // 4 * 4


def term_of(c):
    """TERM of the product of a case (module docstring)"""
    lab = c["label"]
    if lab.startswith("gemm["):
        return 0.0
    if c["a16"] and c["a_affine"] and c["wrapper"] == "gemm":
        return 2.0 ** -9 + X2_TERM + AFFINE_TERM
    if c["mode"] == "x1" and not c["a16"]:
        return X1_TERM
    if c["a16"] and gr.x3w_prods(False, True, c["a_affine"], c["map16"]) == 2:
        return X2_TERM
    if c["a_affine"] and c["wrapper"] == "gemm":
        return X3_TERM + AFFINE_TERM
    return X3_TERM


# ------------------------------------------------------------------ inputs (CPU, seeded)
def make_inputs(c):
    g = torch.Generator().manual_seed(c["seed"])
    nb, M, N, K = c["nb"], c["M"], c["N"], c["K"]
    A = torch.randn(nb, M, K, generator=g) * (2.0 ** -(torch.arange(M) % 13).float()).view(1, M, 1)
    W = torch.randn(nb, K, N, generator=g) * (2.0 ** -(torch.arange(N) % 7).float()).view(1, 1, N) * K ** -0.5      # |pre| stays O(1): no sigmoid saturates
    if M > 5:
        A[:, 5] = 0.0
    d = dict(A=A, W=W, bias=None, scale=None, shift=None, base=None, a_sc=None, a_sh=None, hi=None, lo=None)
    if c["a16"]:
        d["A"] = A.bfloat16().float()                       # the bf16 values are made first: they are the exact inputs
    if c["split_in"]:
        hi = A.bfloat16()
        lo = (A - hi.float()).bfloat16()
        d["hi"], d["lo"] = hi, lo
        d["A"] = (hi.double() + lo.double())                # the planes are the exact inputs
    if c["epi"]:
        half = (torch.rand(N, generator=g) < 0.5).float()
        d["bias"] = torch.randn(N, generator=g) * 0.5 * half
        if c["wrapper"] != "bn_stats":
            sign = torch.where(torch.rand(N, generator=g) < 0.3, -1.0, 1.0)
            d["scale"] = (0.5 + torch.rand(N, generator=g)) * sign
            d["shift"] = torch.randn(N, generator=g) * 0.25 * (torch.rand(N, generator=g) < 0.5).float()
        if c["wrapper"] == "p8":
            d["bias"] = None                                 # the panel kernel has scale and shift only
    if c["a_affine"] or c["wrapper"] == "gemm_act":
        sign = torch.where(torch.rand(K, generator=g) < 0.3, -1.0, 1.0)
        d["a_sc"] = (0.5 + torch.rand(K, generator=g)) * sign
        d["a_sh"] = torch.randn(K, generator=g) * 0.05 * (torch.rand(K, generator=g) < 0.5).float()
    if c["accumulate"]:
        d["base"] = torch.randn(nb, M, N, generator=g) * 0.1
    if c["assign"]:
        d["aw"] = torch.randn(N, 64, generator=g) * (2.0 ** -(torch.arange(64) % 7).float()).view(1, 64)
    return d


def reference(c, d, A=None, terms_A=None, A32=None):
    """(ref, scale, f32) [nb, M, N] of the whole call; A / terms_A / A32 override the left operand (operand transforms)"""
    A64 = (d["A"] if A is None else A).double()
    tA = A64.abs() if terms_A is None else terms_A.double()
    A32 = A64.float() if A32 is None else A32
    W = d["W"]
    if c["wrapper"] == "p8" and d["scale"] is not None:
        W = (W.transpose(1, 2).contiguous() * d["scale"].view(1, -1, 1)).transpose(1, 2)      # W [N, K] * scale[:, None] in fp32, as ops.gemm_p8 does
    W64 = W.double()
    pre, terms, p32 = A64 @ W64, tA @ W64.abs(), seq_matmul(A32, W)
    if d["bias"] is not None:
        b = d["bias"]
        pre, terms, p32 = pre + b.double(), terms + b.double().abs(), p32 + b
    if d["scale"] is not None and c["wrapper"] != "p8":
        s, t = d["scale"], d["shift"]
        pre, terms, p32 = pre * s.double() + t.double(), terms * s.double().abs() + t.double().abs(), p32 * s + t
    elif d["shift"] is not None:
        t = d["shift"]
        pre, terms, p32 = pre + t.double(), terms + t.double().abs(), p32 + t
    act = NONE if (c["a_affine"] or c["wrapper"] in ("gemm_act", "bn_stats", "bf16a", "x3t_split")) else c["act"]
    kink = 2.0 ** -20 + term_of(c)        # how far from 0 a correct pre-activation of this route may still change sign (module docstring)
    ref, scale, f32 = _act(pre, act), _act_scale(pre, terms, act, kink), _act(p32, act)
    if d["base"] is not None:
        ref, scale, f32 = ref + d["base"].double(), scale + d["base"].double().abs(), f32 + d["base"]
    return ref, scale, f32


def transform(c, d):
    """operand transform x' = act(s x + t): (fp64 map, its terms, the fp32 evaluation)"""
    x, s, t = d["A"], d["a_sc"], d["a_sh"]
    aff = s.double() * x.double() + t.double()
    tt = (s.double() * x.double()).abs() + t.double().abs()
    return _act(aff, c["act"]), _act_scale(aff, tt, c["act"]), _act(s * x + t, c["act"])


# ------------------------------------------------------------------ device placement
def rows_dev(x, dev, dtype=torch.float32):
    """[nb, R, C] -> device view with rows padded to a multiple of 4 elements, the padding holding PAD; 2-D when nb == 1"""
    nb, R, C = x.shape
    buf = torch.full((nb, R, _r4(C)), PAD, dtype=dtype, device=dev)
    buf[:, :, :C] = x.to(dev).to(dtype)
    v = buf[:, :, :C]
    return v


def to_panels(x, Bc):
    """rows [Bc * Np, C] -> [Bc, C / 8, Np, 8]"""
    M, C = x.shape
    return x.reshape(Bc, M // Bc, C // 8, 8).permute(0, 2, 1, 3)


def panels_in(ops, x, Bc, dev):
    """cloud panels of x as a panel sub-range of a wider buffer whose other panels hold PAD"""
    M, C = x.shape
    big = ops.panels_empty(Bc, M // Bc, C + 64, dev)
    big.fill_(PAD)
    big[:, 4:4 + C // 8] = to_panels(x.to(dev), Bc)
    return big[:, 4:4 + C // 8]


def split_in(ops, hi, lo, Bc, dev):
    M, C = hi.shape
    big = ops.split_panels_empty(Bc, M // Bc, C + 64, dev)
    big.fill_(3.0)
    big[0, :, 4:4 + C // 8] = to_panels(hi.to(dev), Bc)
    big[1, :, 4:4 + C // 8] = to_panels(lo.to(dev), Bc)
    return big[:, :, 4:4 + C // 8]


class Out:
    """the output of a case: a slice of a wider buffer filled with FILL (or the wrapper's own allocation), pre-filled where the call
    accumulates; untouched() asserts that the surroundings kept their bits"""

    def __init__(self, ops, c, d, dev):
        nb, M, N = c["nb"], c["M"], c["N"]
        self.c, self.wide, self.out = c, None, None
        dt = torch.bfloat16 if c["c16"] else torch.float32
        self.panels = c["panels"] is not None and c["panels"]["c"]
        if self.panels:
            Bc, Np = c["panels"]["Bc"], c["panels"]["Np"]
            self.wide = ops.panels_empty(Bc, Np, N + 64, dev)
            self.storage().fill_(FILL)
            self.out = self.wide[:, 4:4 + N // 8]
            if d["base"] is not None:
                self.out.copy_(to_panels(d["base"][0].to(dev), Bc))
        elif c["slice"] or d["base"] is not None:
            # 4 guard rows above and below every problem and 8 guard columns on either side (16-byte alignment of the slice is kept)
            self.wide = torch.full((nb, M + 8, N + 16), FILL, dtype=dt, device=dev)
            self.out = self.wide[:, 4:4 + M, 8:8 + N]
            if d["base"] is not None:
                self.out.copy_(d["base"].to(dev))
            if not c["batched"]:
                self.out = self.out[0]

    def storage(self):
        """the panels with the pad rows between them: they belong to the buffer, not to the [:, :, :Np] view"""
        Bc, P, Np, _ = self.wide.shape
        return torch.as_strided(self.wide, (Bc, P, self.wide.stride(1) // 8, 8), self.wide.stride())

    def rows(self, ops, got):
        c = self.c
        if self.panels:
            assert got.data_ptr() == self.out.data_ptr()
            return ops.panels_to_rows(got).view(1, c["M"], c["N"])
        return got.reshape(c["nb"], c["M"], c["N"])

    def untouched(self):
        if self.wide is None:
            return
        if self.panels:
            N = self.c["N"]
            full, Np = self.storage(), self.wide.shape[2]
            assert bool((full[:, :4] == FILL).all()) and bool((full[:, 4 + N // 8:] == FILL).all()), "a neighbour panel was written"
            assert bool((full[:, 4:4 + N // 8, Np:] == FILL).all()), "a pad row of an output panel was written"
        else:
            M, N = self.c["M"], self.c["N"]
            assert bool((self.wide[:, :, :8] == FILL).all()) and bool((self.wide[:, :, 8 + N:] == FILL).all()), "a neighbour column was written"
            assert bool((self.wide[:, :4] == FILL).all()) and bool((self.wide[:, 4 + M:] == FILL).all()), \
                "a row above the first or below the last row of a problem was written"


def vec(x, dev):
    return None if x is None else x.to(dev)


class switches:
    """the ops switches of a case, restored on exit; PROFILE collects the labels"""

    def __init__(self, ops, c):
        self.ops, self.c = ops, c

    def __enter__(self):
        ops, c = self.ops, self.c
        self.saved = (ops.X3T_PANELS, ops.X3W_IMPL, ops.P8_IMPL)
        ops.X3T_PANELS, ops.X3W_IMPL, ops.P8_IMPL = c["x3t_panels"], c["x3w_impl"], c["p8_impl"]
        if c["mode"] == "x1":
            ops._FAST.depth += 1
        self.prof = ops.PROFILE = {}
        return self.prof

    def __exit__(self, *exc):
        ops, c = self.ops, self.c
        ops.PROFILE = None
        if c["mode"] == "x1":
            ops._FAST.depth -= 1
        ops.X3T_PANELS, ops.X3W_IMPL, ops.P8_IMPL = self.saved
        return False


def assert_label(c, prof):
    gemms = sorted(k for k in prof if k.startswith("gemm") and k != "gemm_prep_b")
    assert gemms == [c["label"]], (c["name"], gemms, c["label"])
    assert len(prof[c["label"]]) == 1


# ------------------------------------------------------------------ the wrappers
def run_gemm(ops, c, d, dev):
    nb, ak, bk = c["nb"], c["ak"], c["bk"]
    dtA = torch.bfloat16 if c["a16"] else torch.float32
    A = rows_dev(d["A"].transpose(1, 2) if ak else d["A"], dev, dtA)
    B = rows_dev(d["W"] if bk else d["W"].transpose(1, 2), dev)
    if not c["batched"]:
        A, B = A[0], B[0]
    o = Out(ops, c, d, dev)
    kw = dict(bias=vec(d["bias"], dev), scale=vec(d["scale"], dev), shift=vec(d["shift"], dev), slope=SLOPE, exact=c["mode"] == "f32")
    with switches(ops, c) as prof:
        if c["wrapper"] == "linear":
            got = ops.linear(A, B, act=c["act"], out=o.out, splits=c["splits"], **kw)
        else:
            aff = (d["a_sc"].to(dev), d["a_sh"].to(dev), c["act"], SLOPE) if c["a_affine"] else None
            got = ops.gemm(A, B, a_kmajor=ak, b_kmajor=bk, act=NONE if c["a_affine"] else c["act"], out=o.out, splits=c["splits"],
                           accumulate=c["accumulate"], out_bf16=c["c16"], a_affine=aff, **kw)
    assert_label(c, prof)
    assert got.dtype == (torch.bfloat16 if c["c16"] else torch.float32)
    if c["a_affine"]:
        m64, mt, m32 = transform(c, d)
        ref, scale, f32 = reference(c, d, A=m64, terms_A=mt, A32=m32)
    else:
        ref, scale, f32 = reference(c, d)
    check_bound(c["name"], o.rows(ops, got), ref, f32, scale, term_of(c), round16=c["c16"])
    o.untouched()


def run_panels(ops, c, d, dev):
    p = c["panels"]
    Bc, bk = p["Bc"], c["bk"]
    A = panels_in(ops, d["A"][0], Bc, dev) if p["a"] else rows_dev(d["A"], dev)[0]
    B = rows_dev(d["W"] if bk else d["W"].transpose(1, 2), dev)[0]
    o = Out(ops, c, d, dev)
    with switches(ops, c) as prof:
        got = ops.gemm(A, B, b_kmajor=bk, bias=vec(d["bias"], dev), scale=vec(d["scale"], dev), shift=vec(d["shift"], dev), act=c["act"],
                       slope=SLOPE, out=o.out, accumulate=c["accumulate"], exact=c["mode"] == "f32", a_panels=p["a"], out_panels=p["c"])
    assert_label(c, prof)
    ref, scale, f32 = reference(c, d)
    check_bound(c["name"], o.rows(ops, got), ref, f32, scale, term_of(c))
    o.untouched()


def run_x3t_split(ops, c, d, dev):
    p = c["panels"]
    S = split_in(ops, d["hi"][0], d["lo"][0], p["Bc"], dev)
    W = d["W"][0].t().contiguous().to(dev)
    o = Out(ops, c, d, dev)
    with switches(ops, c) as prof:
        got = ops.gemm_x3t_split(S, W, out=o.out)
    assert_label(c, prof)
    ref, scale, f32 = reference(c, d)
    check_bound(c["name"], o.rows(ops, got), ref, f32, scale, term_of(c))
    o.untouched()


def run_p8(ops, c, d, dev):
    p = c["panels"]
    M, N = c["M"], c["N"]
    S = split_in(ops, d["hi"][0], d["lo"][0], p["Bc"], dev)
    W = d["W"][0].t().contiguous().to(dev)
    o = Out(ops, c, d, dev)
    aw = d["aw"].to(dev) if c["assign"] else None
    with switches(ops, c) as prof:
        got = ops.gemm_p8(S, W, scale=vec(d["scale"], dev), shift=vec(d["shift"], dev), act=c["act"], slope=SLOPE, out=o.out,
                          out_panels=p["c"], assign_w=aw)
    assert_label(c, prof)
    parts = None
    if c["assign"]:
        got, parts = got
    ref, scale, f32 = reference(c, d)
    rows = o.rows(ops, got)
    check_bound(c["name"], rows, ref, f32, scale, term_of(c))
    o.untouched()
    if parts is not None:
        assert parts.shape == (N // 256, M, 64)
        C = rows[0].cpu()
        for j in range(N // 256):
            Cj, Wj = C[:, 256 * j:256 * j + 256], d["aw"][256 * j:256 * j + 256]
            check_bound(f"{c['name']}:parts{j}", parts[j], Cj.double() @ Wj.double(), seq_matmul(Cj, Wj), Cj.double().abs() @ Wj.double().abs(), X3_TERM)


def run_bn_stats(ops, c, d, dev):
    M = c["M"]
    x = rows_dev(d["A"], dev, torch.bfloat16 if c["a16"] else torch.float32)[0]
    w = d["W"][0].t().contiguous().to(dev)
    keep = ops._bn_finalize
    ops._bn_finalize = lambda sums, R, C, bn: sums.clone()        # the fp64 column sums as the epilogue left them
    try:
        with switches(ops, c) as prof:
            y, sums = ops.linear_bn_stats(x, w, None, bias=vec(d["bias"], dev), out_bf16=c["c16"])
    finally:
        ops._bn_finalize = keep
    assert_label(c, prof)
    assert y.dtype == (torch.bfloat16 if c["c16"] else torch.float32) and sums.dtype == torch.float64 and sums.shape == (2, c["N"])
    ref, scale, f32 = reference(c, d)
    t = term_of(c)
    check_bound(c["name"], y.view(1, M, -1), ref, f32, scale, t, round16=c["c16"])
    ref, scale, f32 = ref[0], scale[0], f32[0]
    check_bound(c["name"] + ":sum", sums[0], ref.sum(0), _seqsum(f32, 0), scale.sum(0), t)
    check_bound(c["name"] + ":sumsq", sums[1], (ref * ref).sum(0), _seqsum(f32 * f32, 0), (scale * scale).sum(0), (1 + t) ** 2 - 1)


def run_gemm_act(ops, c, d, dev):
    M, K = c["M"], c["K"]
    x = rows_dev(d["A"], dev, torch.bfloat16 if c["a16"] else torch.float32)[0]
    w = rows_dev(d["W"], dev)[0]
    args = (d["a_sc"].to(dev), d["a_sh"].to(dev), c["act"], SLOPE)
    with switches(ops, c) as prof:
        xa, got = ops.gemm_act(x, w, *args, out_bf16=c["map16"], store=c["store"])
    assert_label(c, prof)
    if not c["store"]:
        assert xa is None
        with switches(ops, c):
            xa, stored = ops.gemm_act(x, w, *args, out_bf16=c["map16"], store=True)
        assert torch.equal(got, stored), "store=False changes the product"
    assert xa.dtype == (torch.bfloat16 if c["map16"] else torch.float32) and xa.shape == (M, K)
    m64, mt, m32 = transform(c, d)
    check_bound(c["name"] + ":map", xa.view(1, M, K), m64, m32, mt, 0.0, round16=c["map16"])
    ref, scale, f32 = reference(c, d, A=xa.float().cpu().view(1, M, K))          # the stored map is the product's exact input
    check_bound(c["name"], got.view(1, M, -1), ref, f32, scale, X1_TERM if c["mode"] == "x1" else (X2_TERM if c["map16"] else X3_TERM))


def run_bf16a(ops, c, d, dev):
    bk = c["bk"]
    A = rows_dev(d["A"], dev, torch.bfloat16)[0]
    W = rows_dev(d["W"] if bk else d["W"].transpose(1, 2), dev)[0]
    o = Out(ops, c, d, dev)
    with switches(ops, c) as prof:
        got = ops.gemm_bf16a(A, W, b_kmajor=bk, out=o.out, accumulate=c["accumulate"])
    assert_label(c, prof)
    ref, scale, f32 = reference(c, d)
    check_bound(c["name"], o.rows(ops, got), ref, f32, scale, term_of(c))
    o.untouched()


RUN = {"gemm": run_gemm, "linear": run_gemm, "panels": run_panels, "x3t_split": run_x3t_split, "p8": run_p8, "bn_stats": run_bn_stats,
       "gemm_act": run_gemm_act, "bf16a": run_bf16a}


@pytest.mark.parametrize("name", [c["name"] for c in gr.CASES])
def test_gemm_route(cuda, name):
    c = gr.by_name(name)
    ops = _ops()
    RUN[c["wrapper"]](ops, c, make_inputs(c), cuda)
