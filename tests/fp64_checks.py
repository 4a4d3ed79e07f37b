"""The per-element measure of the fp64 comparisons, shared by tests/test_fwd_ops_gpu.py and tests/test_gemm_routes_*.py.

An output element is compared with a float64 evaluation of the same formula and its error is scaled by the float64 sum |term| of that
element (`scale`); a float32 evaluation of the formula from the same inputs gives the fp32 FLOOR of the element (never taken below 2^-23).
Nothing here needs a GPU: `got` may be any tensor.
"""
import torch

U23 = 2.0 ** -23
ELEM_X = 4.0
SUM_X = 2.0
X3_TERM = 3 * 2.0 ** -18       # split-bf16 three-product form: |a b - (ah bh + ah bl + al bh)| <= (2^-18 + 2 * 2^-18) |a b|
X1_TERM = 2 * 2.0 ** -9 + 2.0 ** -18      # one product ah bh: both operands rounded to bf16
X2_TERM = 2.0 ** -18                      # bf16 rows (exact) against a split operand: only that operand's residual is lost
AFFINE_TERM = 2.0 ** -22                  # operand transform evaluated in fp32 in a loader (tests/test_gemm_routes_gpu.py derives the three)
NONE, RELU, LEAKY, SIGMOID = 0, 1, 2, 3
SLOPE = 0.01


def _scaled(got, ref, scale, exact_zero=True):
    """max |got - ref| / scale; an element whose scale is 0 (no non-zero term) must be exact"""
    d = (got.detach().double().cpu() - ref).abs()
    s = scale.double()
    if exact_zero:
        assert bool((d[s == 0] == 0).all()), "an element without any non-zero term is not exactly 0"
    return (d / s.clamp_min(1e-300))[s > 0].max().item() if bool((s > 0).any()) else 0.0


def _check(tag, got, ref, f32, scale, factor):
    """GPU error and fp32 floor of one output, both scaled by `scale`; asserts err <= factor * max(floor, 2^-23)"""
    floor = max(_scaled(f32, ref, scale, exact_zero=False), U23)
    err = _scaled(got, ref, scale)
    print(f"MEASURE {tag} err={err:.3e} floor={floor:.3e} bound={factor * floor:.3e}")
    assert err <= factor * floor, (tag, err, floor)
    return err, floor


def _act(pre, act):
    if act == SIGMOID:
        return torch.sigmoid(pre)
    ns = {NONE: 1.0, RELU: 0.0, LEAKY: SLOPE}[act]
    return torch.where(pre > 0, pre, pre * ns)


def _act_scale(pre, terms, act, kink=2.0 ** -20):
    """sum |term| of act(pre) where pre carries `terms` = sum |term|: the slope of the activation times the terms of its argument, plus
    the value itself for the sigmoid; within 2^-20 `terms` of the kink the full scale (either side is a correct rounding).  `kink`: a
    route whose pre-activation is only good to kink * terms (a bf16 product) may come out on either side within that distance"""
    if act == SIGMOID:
        y = torch.sigmoid(pre)
        return y + y * (1 - y) * terms
    ns = {NONE: 1.0, RELU: 0.0, LEAKY: SLOPE}[act]
    fac = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, ns))
    return torch.where(pre.abs() <= kink * terms, terms, terms * fac)


def _seqsum(t, dim):
    """float32 sum along `dim` in sequence, term after term (a loop: torch.cumsum on the CPU accumulates float32 in double)"""
    t = t.float().movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def half_ulp_bf16(v):
    """half an ulp of bfloat16 (8 significant bits) at |v|: 2^(floor(log2 |v|) - 8); between 2^-9 |v| and 2^-8 |v|"""
    v = v.double().abs()
    return torch.where(v > 0, 2.0 ** (torch.floor(torch.log2(v.clamp_min(1e-300))) - 8), torch.zeros_like(v))


def seq_matmul(A, W):
    """float32 A [.., M, K] @ W [.., K, N] accumulated IN SEQUENCE over k: K rank-1 updates, each a float32 multiply and a float32 add"""
    A, W = A.float(), W.float()
    acc = torch.zeros(A.shape[:-1] + (W.shape[-1],), dtype=torch.float32)
    for k in range(A.shape[-1]):
        acc = acc + A[..., :, k:k + 1] * W[..., k:k + 1, :]
    return acc


def check_bound(tag, got, ref, f32, scale, term, round16=False, what="gemm"):
    """The GEMM form of _check: per element |got - ref| <= e = (term + 2 floors) * scale; round16 (the fp32 value v, within e of ref, is
    stored as bf16): e + half an ulp of bf16 at |ref| + e, i.e. 2^(floor(log2(|ref| + e)) - 8).  floor = max over the elements of |f32 - ref| / scale, never below 2^-23.  An element whose scale is 0
    must be exactly 0.  Prints err / floor / bound (in units of `scale`) of the element closest to its bound."""
    ref, s = ref.double(), scale.double()
    d = (got.detach().double().cpu() - ref).abs()
    assert bool(torch.isfinite(d).all()), (tag, "non-finite result")
    assert bool((d[s == 0] == 0).all()), (tag, "an element without any non-zero term is not exactly 0")
    floor = max(_scaled(f32, ref, s, exact_zero=False), U23)
    pos = s > 0
    if not bool(pos.any()):
        print(f"MEASURE {what}/{tag} err=0.000e+00 floor={floor:.3e} bound={term + SUM_X * floor:.3e}")
        return 0.0, floor, term + SUM_X * floor
    sp = s.clamp_min(1e-300)
    bound = torch.full_like(d, term + SUM_X * floor)
    if round16:
        bound = bound + half_ulp_bf16(ref.abs() + bound * sp) / sp
    ratio = torch.where(pos, d / sp / bound, torch.zeros_like(d))
    i = int(ratio.argmax())
    err, b = (d / sp).flatten()[i].item(), bound.flatten()[i].item()
    print(f"MEASURE {what}/{tag} err={err:.3e} floor={floor:.3e} bound={b:.3e}")
    assert ratio.flatten()[i].item() <= 1.0, (tag, err, floor, b)
    return err, floor, b


def split_bf16(x):
    """hi = bf16(x), lo = bf16(x - hi), both as float32 (round to nearest even)"""
    hi = x.float().bfloat16().float()
    return hi, (x.float() - hi).bfloat16().float()


def seq_matmul_x3(A, W, prods=3):
    """float32 emulation of the split-bf16 product accumulated in sequence over k: per term ah bh + ah bl + al bh (prods = 3) or ah bh
    alone (prods = 1), every product and every add rounded to float32"""
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(W)
    acc = torch.zeros(A.shape[:-1] + (W.shape[-1],), dtype=torch.float32)
    for k in range(A.shape[-1]):
        a_h, a_l, b_h, b_l = ah[..., :, k:k + 1], al[..., :, k:k + 1], bh[..., k:k + 1, :], bl[..., k:k + 1, :]
        acc = acc + a_h * b_h
        if prods == 3:
            acc = acc + a_h * b_l
            acc = acc + a_l * b_h
    return acc
