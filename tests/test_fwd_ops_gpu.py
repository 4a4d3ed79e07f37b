"""The forward head, the BatchNorm apply, the mining and the loss kernels (csrc/lpd_misc.hip, lpd_affine_act / lpd_bn_finalize of
csrc/lpd_train.hip, csrc/lpd_loss.hip) against float64 on the CPU, at the sizes at which eval (B = 32) and training (B = 44) run them.
tests/launch_sizes.py states each launch regime; tests/test_launch_sizes_cpu.py checks that the shapes used here reach it.

Every case calls the op through its lpdnet_hip.ops wrapper and compares with a float64 torch-CPU evaluation of the same formula, written
out here.  No oracle model code and no other kernel is the expected side.

How the bounds are set (none is taken from what the kernels give):
  - moves and selections (transpose, colmax, mul, f64_to_f32, group_max_bwd, the bf16 copy of affine_act) are compared bit for bit;
  - an op with rounding is evaluated a third time in float32 on the CPU from the same inputs; its error against the float64 reference,
    element by element and scaled by the float64 sum |term| of that element (affine and bias terms included), is the fp32 FLOOR of the
    formula for those inputs (never taken below 2^-23).  The GPU result must stay within ELEM_X = 4 floors: the factor covers another
    summation order, fused multiply-adds and another expf;
  - sums over points (softmax column sums, VLAD a_sum and column norms, the gating and small-K dot products, the distances of the loss)
    take the floor from a float32 accumulation IN SEQUENCE, term after term (a loop of float32 adds): the kernels add runs of rows one
    after the other and then atomics in any order, and the in-sequence sum bounds every such order.  The GPU must stay within SUM_X = 2;
  - the split-bf16 product (apply_transform at K = 64 over many rows) is a different number format: each operand is hi + lo in bfloat16
    (8 significant bits each) and the lo * lo products are dropped, 3 * 2^-18 of sum |term| at most (see X3_TERM);
  - retrieval_topk / hard_negatives: index lists equal a float64 stable argsort on exactly representable inputs; on real-valued
    descriptors every returned rank stays within 4 float32 floors of the same distance formulation.
Each case prints `MEASURE <op>/<shape> ...` with the GPU error next to its floor.
"""
import copy

import numpy as np
import pytest
import torch

import launch_sizes as ls
from fp64_checks import (ELEM_X, LEAKY, NONE, RELU, SIGMOID, SLOPE, SUM_X, U23, X3_TERM,      # noqa: F401  (the shared measure)
                         _act, _act_scale, _check, _scaled, _seqsum)

pytestmark = pytest.mark.gpu

FLT_MIN = 1.1754943508222875e-38


def _ops():
    from lpdnet_hip import ops
    return ops


def _err():
    from lpdnet_hip import LpdHipError
    return LpdHipError


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================== bit-exact ops
@pytest.mark.parametrize("shape", [(44, 4096, 64), (2, 1024, 4096), (3, 33, 31), (1, 1, 5), (5, 4097, 3), (2, 32, 32), (2, 31, 33)])
def test_transpose_bit_exact(cuda, shape):
    x = torch.randn(shape, generator=_gen(sum(shape)))
    got = _ops().transpose(x.to(cuda))
    assert got.shape == (shape[0], shape[2], shape[1]) and got.is_contiguous()
    assert torch.equal(got.cpu(), x.transpose(1, 2).contiguous())
    _free()


@pytest.mark.parametrize("B,N,C", [(44, 4096, 1024), (2, 4096, 70), (3, 3, 64), (1, 1, 4)])
@pytest.mark.parametrize("values", ["randn", "negative", "neginf"])
def test_colmax_bit_exact(cuda, B, N, C, values):
    if (B, N, C) == (44, 4096, 1024) and values != "randn":
        values = values + "-small"
        B = 3                                               # the large cloud count once: the other value sets at B = 3 of the same N and C
    x = torch.randn(B * N, C, generator=_gen(B + N + C))
    if values.startswith("negative"):
        x = -x.abs() - 0.5
    elif values.startswith("neginf"):
        x[torch.rand(B * N, C, generator=_gen(1)) < 0.3] = float("-inf")
        x[:N, 0] = float("-inf")                            # a whole column of one cloud
    got = _ops().colmax(x.to(cuda), B, N)
    assert torch.equal(got.cpu(), x.view(B, N, C).max(dim=1).values)
    _free()


def test_colmax_on_a_column_slice(cuda):
    """ldi != C: the columns 4 .. 4 + 70 of a 96-wide tensor, and 64 columns from column 3 on"""
    B, N = 3, 1000
    wide = torch.randn(B * N, 96, generator=_gen(4))
    dw = wide.to(cuda)
    for c0, C in ((4, 70), (3, 64), (0, 96), (95, 1)):
        got = _ops().colmax(dw[:, c0:c0 + C], B, N)
        assert torch.equal(got.cpu(), wide[:, c0:c0 + C].reshape(B, N, C).max(dim=1).values), (c0, C)


@pytest.mark.parametrize("n", [255, 256, 257, 44 * 256])
def test_mul_bit_exact(cuda, n):
    g = _gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e3
    assert torch.equal(_ops().mul(a.to(cuda), b.to(cuda)).cpu(), a * b)
    if n == 44 * 256:
        a2, b2 = a.view(44, 256), b.view(44, 256)
        assert torch.equal(_ops().mul(a2.to(cuda), b2.to(cuda)).cpu(), a2 * b2)


@pytest.mark.parametrize("n", [1, 2, 3, 44 * 4096 * 3 + 1])
def test_f64_to_f32_rounds_like_numpy(cuda, n):
    """What tests/test_model_gpu.py's ingest test leaves out (it has one 7-element vector: two ties, +overflow, one underflow to -0, the
    largest float's upper neighbourhood): n = 1, 2, 3 and a submap batch plus one (the scalar tail behind the paired loads), +-0,
    subnormal results (exact, rounded and tied), results that round up to the smallest normal, -overflow, +-inf, NaN and ties at
    several exponents, to even in both directions."""
    f = np.float64
    tiny = f(2.0) ** -149
    special = np.array([0.0, -0.0, tiny, -tiny, 0.5 * tiny, 1.5 * tiny, 2.5 * tiny, 0.75 * tiny, -0.25 * tiny, 3.0 * tiny, f(2.0) ** -127 * 1.3,
                        f(2.0) ** -126 * (1 - f(2.0) ** -25), f(2.0) ** -126, 1e-39, -1e-42, 1e-46, np.inf, -np.inf, np.nan, -1e300, 3.5e38, -3.5e38,
                        3.4028235677973366e38, np.nextafter(f(3.4028235677973366e38), 0), 1 + f(2.0) ** -24, 1 + 3 * f(2.0) ** -24,
                        -(1 + f(2.0) ** -24), 1 + f(2.0) ** -24 + f(2.0) ** -50, 1 + f(2.0) ** -24 - f(2.0) ** -52, 1024 + f(2.0) ** -14,
                        1024 + 3 * f(2.0) ** -14, f(2.0) ** 100 * (1 + 5 * f(2.0) ** -24), 1.0, -7.25, 0.1], dtype=np.float64)
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    if n > 3:
        x[:special.size] = special
        x[-special.size:] = special[::-1]
        x[special.size:2 * special.size] = x[special.size:2 * special.size].astype(np.float32).astype(np.float64) + rng.choice([-1, 1], special.size) * \
            np.spacing(x[special.size:2 * special.size].astype(np.float32)).astype(np.float64) / 2          # exact ties of random floats
        want = x.astype(np.float32)
        got = _ops().f64_to_f32(torch.from_numpy(x).to(cuda)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32) & 0x7fffffff > 0x7f800000, np.isnan(want))
        ok = np.isnan(want) | (got.view(np.uint32) == want.view(np.uint32))                                # the sign of zero included
        assert ok.all(), (x[~ok][:5], got[~ok][:5], want[~ok][:5])
        return
    for start in range(0, special.size - n + 1):
        v = special[start:start + n].copy()
        want = v.astype(np.float32)
        got = _ops().f64_to_f32(torch.from_numpy(v).to(cuda)).cpu().numpy()
        ok = np.isnan(want) & np.isnan(got) | (got.view(np.uint32) == want.view(np.uint32))
        assert ok.all(), (v, got, want)


@pytest.mark.parametrize("M,C,k", sorted(ls.FWD_GROUP_MAX_BWD))
def test_group_max_bwd_is_an_index_scatter(cuda, M, C, k):
    """dX[(i, t)][c] = dOut[i][c] where arg[i][c] == t, else 0 (accumulate = False writes every element; accumulate = True adds into dX)"""
    ops = _ops()
    g = _gen(M + C)
    buf = torch.randn(M, C + 8, generator=g).to(cuda)
    dOut = buf[:, 4:4 + C]                                               # ldo != C
    arg = torch.randint(0, k, (M, C), generator=g).to(torch.uint8).to(cuda)
    want = torch.zeros(M, k, C)
    want.scatter_(1, arg.cpu().long().view(M, 1, C), dOut.cpu().reshape(M, 1, C))          # one source element per (i, c)
    got = torch.full((M * k, C), 7.0, device=cuda)
    ops.group_max_bwd(dOut, arg, k, got, accumulate=False)
    assert torch.equal(got.cpu(), want.view(M * k, C))
    got2 = ops.group_max_bwd(dOut, arg, k)                               # the wrapper's own buffer
    assert torch.equal(got2, got)
    del got2
    base = torch.randn(M * k, C, generator=_gen(5))
    got.copy_(base)
    ops.group_max_bwd(dOut, arg, k, got, accumulate=True)
    want = base.view(M, k, C)
    want.scatter_add_(1, arg.cpu().long().view(M, 1, C), dOut.cpu().reshape(M, 1, C))      # one addend per element: base + g in fp32, no order involved
    assert torch.equal(got.cpu(), want.view(M * k, C))
    del got, base, want
    _free()


# ================================================================== affine_act / affine_act2
def _affine_ref(x, sc, sh, act):
    pre = sc.double() * x.double() + sh.double()
    terms = (sc.double() * x.double()).abs() + sh.double().abs()
    f32 = _act(sc * x + sh, act)
    return _act(pre, act), _act_scale(pre, terms, act), f32


# all four activations in the three small regimes; the two capped ones (20 M and 17 M elements) with the two branches of the kernel, the
# piecewise-linear one and the sigmoid
AFFINE_CASES = [(n, a) for n in sorted(ls.FWD_AFFINE_SHAPES) for a in (NONE, RELU, LEAKY, SIGMOID)
                if not ls.FWD_AFFINE_SHAPES[n][2] or a in (LEAKY, SIGMOID)]


@pytest.mark.parametrize("name,act", AFFINE_CASES)
def test_affine_act_against_fp64(cuda, name, act):
    """act(scale * X + shift) in every launch regime of lpd_affine_act (tests/launch_sizes.py FWD_AFFINE_SHAPES), X a column slice"""
    ops = _ops()
    R, C, _, _ = ls.FWD_AFFINE_SHAPES[name]
    g = _gen(R + C + act)
    wide = torch.randn(R, C + 4, generator=g) * 2
    x = wide[:, :C]
    sc, sh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref, scale, f32 = _affine_ref(x, sc, sh, act)
    got = ops.affine_act(wide.to(cuda)[:, :C], sc.to(cuda), sh.to(cuda), act, SLOPE)
    assert got.shape == (R, C)
    _check(f"affine_act/{name}/act{act}", got, ref, f32, scale, ELEM_X)
    if act == LEAKY:                                                       # no scale / shift, no activation: a copy
        plain = ops.affine_act(wide.to(cuda)[:, :C], None, None, NONE)
        assert torch.equal(plain.cpu(), x)
    _free()


@pytest.mark.parametrize("name", ["capped_pow2", "capped_reload", "reload", "c2048_odd_grid"])
def test_affine_act_forms(cuda, name):
    """in place, rows=, strided out, the bf16 copy (affine_act2: out16 a column slice) and only16 -- each equal, bit for bit, to the plain
    call that test_affine_act_against_fp64 measures, so every form is held to the same float64 comparison"""
    ops = _ops()
    R, C, _, _ = ls.FWD_AFFINE_SHAPES[name]
    g = _gen(R + C)
    x = (torch.randn(R, C, generator=g) * 2).to(cuda)
    sc, sh = torch.randn(C, generator=g).to(cuda), torch.randn(C, generator=g).to(cuda)
    plain = ops.affine_act(x, sc, sh, LEAKY, SLOPE)
    ref, scale, f32 = _affine_ref(x.cpu(), sc.cpu(), sh.cpu(), LEAKY)
    _check(f"affine_act_forms/{name}", plain, ref, f32, scale, ELEM_X)
    del ref, scale, f32
    # strided out
    buf = torch.full((R, C + 8), -3.0, device=cuda)
    out = ops.affine_act(x, sc, sh, LEAKY, SLOPE, out=buf[:, 4:4 + C])
    assert out.data_ptr() == buf[:, 4:4 + C].data_ptr() and torch.equal(out, plain)
    assert bool((buf[:, :4] == -3.0).all()) and bool((buf[:, 4 + C:] == -3.0).all())
    del buf, out
    # rows=: the rows beyond are left alone
    rows = R - R // 3
    part = torch.full((R, C), -3.0, device=cuda)
    ops.affine_act(x, sc, sh, LEAKY, SLOPE, out=part, rows=rows)
    assert torch.equal(part[:rows], plain[:rows]) and bool((part[rows:] == -3.0).all())
    del part
    # the bf16 copy beside the fp32 rows, and alone
    wide16 = torch.zeros((R, C + 8), dtype=torch.bfloat16, device=cuda)
    o16 = wide16[:, 4:4 + C]
    out = ops.affine_act(x, sc, sh, LEAKY, SLOPE, out16=o16)
    assert torch.equal(out, plain)
    assert torch.equal(o16.view(torch.int16), plain.to(torch.bfloat16).view(torch.int16))                  # bit for bit
    assert bool((wide16[:, :4] == 0).all()) and bool((wide16[:, 4 + C:] == 0).all())
    only = torch.zeros((R, C + 8), dtype=torch.bfloat16, device=cuda)
    r16 = ops.affine_act(x, sc, sh, LEAKY, SLOPE, out16=only[:, 4:4 + C], only16=True)
    assert r16.dtype == torch.bfloat16 and torch.equal(r16.view(torch.int16), o16.view(torch.int16))
    part16 = torch.zeros((R, C), dtype=torch.bfloat16, device=cuda)
    ops.affine_act(x, sc, sh, SIGMOID, out16=part16, rows=rows, only16=True)
    sig = ops.affine_act(x, sc, sh, SIGMOID)
    assert torch.equal(part16[:rows].view(torch.int16), sig[:rows].to(torch.bfloat16).view(torch.int16)) and bool((part16[rows:] == 0).all())
    del wide16, only, part16, sig, out
    # in place
    xin = x.clone()
    res = ops.affine_act(xin, sc, sh, LEAKY, SLOPE, out=xin)
    assert res.data_ptr() == xin.data_ptr() and torch.equal(xin, plain)
    _free()


# ================================================================== bn_train_stats -> _bn_finalize
def _bn_module(C, momentum, track, seed):
    g = _gen(seed)
    bn = torch.nn.BatchNorm1d(C, momentum=momentum, track_running_stats=track)
    with torch.no_grad():
        w = 0.3 + torch.rand(C, generator=g)
        bn.weight.copy_(torch.where(torch.rand(C, generator=g) < 0.35, -w, w))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        if track:
            bn.running_mean.copy_(torch.randn(C, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.train()


@pytest.mark.parametrize("momentum,track", [(0.1, True), (None, True), (0.1, False)], ids=["m0.1", "cumulative", "untracked"])
@pytest.mark.parametrize("R,C", [(2, 64), (3001, 64), (44 * 4096, 64), (20001, 1024), (5000, 12)])
def test_bn_train_stats_and_finalize(cuda, R, C, momentum, track):
    """scale / shift / mean / invstd of one train-mode BatchNorm application and its running-statistics update, twice in a row, against
    torch's own BatchNorm1d in float64 on the CPU.  The float32 floor is the same module in float32.  Column 0 is the constant 1e4:
    its variance must come out 0 (the clamp) and its invstd 1 / sqrt(eps) to the last bit."""
    ops = _ops()
    g = _gen(R + C)
    bn = _bn_module(C, momentum, track, R + C)
    bn64, bn32 = copy.deepcopy(bn).double(), copy.deepcopy(bn)
    dbn = bn.to(cuda)
    for call in (1, 2):
        x = torch.randn(R, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 3 * torch.randn(C, generator=g)
        x[:, 0] = 1e4
        if C > 2:
            x[:, 1] += 300.0                                                # a large mean against a unit spread
        st = ops.bn_train_stats(x.to(cuda), dbn)
        x64 = x.double()
        rm0 = bn64.running_mean.clone() if track else None
        rv0 = bn64.running_var.clone() if track else None
        bn64(x64), bn32(x)                                                  # torch.nn.functional.batch_norm(training=True) underneath
        mean = x64.mean(0)
        var = x64.var(0, unbiased=False)
        invstd = 1.0 / torch.sqrt(var + bn.eps)
        w, b = bn64.weight.detach(), bn64.bias.detach()
        mabs = x64.abs().mean(0)
        # the float32 evaluation of the same statistics
        m32, v32 = x.mean(0), x.var(0, unbiased=False)
        i32 = 1.0 / torch.sqrt(v32 + bn.eps)
        w32, b32 = bn32.weight.detach(), bn32.bias.detach()
        tag = f"bn_finalize/{R}x{C}/{'cum' if momentum is None else momentum}/{'track' if track else 'notrack'}/call{call}"
        _check(tag + "/mean", st.mean, mean, m32, mabs, ELEM_X)
        _check(tag + "/invstd", st.invstd, invstd, i32, invstd, ELEM_X)
        _check(tag + "/scale", st.scale, w * invstd, w32 * i32, (w * invstd).abs(), ELEM_X)
        _check(tag + "/shift", st.shift, b - mean * w * invstd, b32 - m32 * w32 * i32, b.abs() + (mabs * w * invstd).abs(), ELEM_X)
        assert st.count == R
        eps32 = float(np.float32(bn.eps))
        assert st.invstd[0].item() == float(np.float32(1.0 / np.sqrt(np.float64(eps32)))), "constant column: var = 0 exactly, invstd = 1 / sqrt(eps)"
        assert st.mean[0].item() == 1e4
        if track:
            f = 1.0 / call if momentum is None else momentum
            unb = var * R / (R - 1)
            assert torch.allclose(bn64.running_mean, (1 - f) * rm0 + f * mean, rtol=1e-12, atol=1e-12)      # the reference does what the formula says
            assert torch.allclose(bn64.running_var, (1 - f) * rv0 + f * unb, rtol=1e-12, atol=1e-12)
            _check(tag + "/running_mean", dbn.running_mean, bn64.running_mean, bn32.running_mean, (1 - f) * rm0.abs() + f * mabs, ELEM_X)
            _check(tag + "/running_var", dbn.running_var, bn64.running_var, bn32.running_var, (1 - f) * rv0 + f * unb, ELEM_X)
            got0, want0 = dbn.running_var[0].item(), float(np.float32((1 - f) * rv0[0].item()))
            assert abs(got0 - want0) <= 2.0 ** -23 * abs(want0), "constant column adds no variance"
            assert int(dbn.num_batches_tracked) == int(bn64.num_batches_tracked) == call
        else:
            assert dbn.running_mean is None and dbn.running_var is None and dbn.num_batches_tracked is None
    _free()


def test_bn_train_stats_one_row_raises(cuda):
    bn = _bn_module(64, 0.1, True, 1).to(cuda)
    rm = bn.running_mean.clone()
    with pytest.raises(ValueError):
        _ops().bn_train_stats(torch.randn(1, 64, device=cuda), bn)
    with pytest.raises(ValueError):
        _ops().bn_train_stats(torch.randn(5, 64, device=cuda), bn, rows=1)
    assert torch.equal(bn.running_mean, rm) and int(bn.num_batches_tracked) == 0


# ================================================================== softmax_affine
def _softmax_logits(rows, ncols, seed):
    """3 * randn, with the second cloud multiplied by 30 (most of a row underflows), 64 rows of equal logits and one row with a +80 outlier"""
    a = torch.randn(rows, ncols, generator=_gen(seed)) * 3
    a[4096:8192] *= 30
    a[100:164] = 1.25
    a[300, ncols // 2] += 80
    return a


def _softmax_checks(tag, got, ref, f32):
    """element-wise: relative to the fp64 value where that is a normal float, absolute (at most the smallest normal: a result below it may be
    flushed or rounded to a subnormal) below; every row sums to 1"""
    normal = ref >= FLT_MIN
    floor = max(((f32.double() - ref).abs() / ref)[normal].max().item(), U23)
    g = got.double().cpu()
    err = ((g - ref).abs() / ref)[normal].max().item()
    print(f"MEASURE {tag}/elements err={err:.3e} floor={floor:.3e} bound={ELEM_X * floor:.3e}")
    assert err <= ELEM_X * floor, (tag, err, floor)
    assert bool(((g - ref).abs()[~normal] <= FLT_MIN).all())
    rowerr = (g.sum(1) - 1).abs().max().item()
    print(f"MEASURE {tag}/rowsum err={rowerr:.3e} bound={ELEM_X * floor:.3e}")
    assert rowerr <= ELEM_X * floor
    return floor


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("ncols", [64, 40, 1])
@pytest.mark.parametrize("rows", ls.FWD_SOFTMAX_ROWS)
def test_softmax_affine_against_fp64(cuda, rows, ncols, affine):
    """the row kernel, the generic column-sum kernel and the 64-column one (tests/launch_sizes.py FWD_SOFTMAX_CASES) at 32 x 4096 and
    44 x 4096 rows; at 64 columns also from an input 4 bytes off the 16-byte alignment (the generic kernel takes the 64-column job)"""
    ops = _ops()
    N = 4096
    B = rows // N
    g = _gen(rows + ncols)
    a = _softmax_logits(rows, ncols, rows + ncols)
    sc = (0.5 + torch.rand(ncols, generator=g)) if affine else None
    sh = torch.randn(ncols, generator=g) if affine else None
    v64 = a.double() * sc.double() + sh.double() if affine else a.double()
    ref = torch.softmax(v64, dim=1)
    f32 = torch.softmax(a * sc + sh if affine else a, dim=1)
    colref = ref.view(B, N, ncols).sum(1)
    colfloor = max(((_seqsum(f32.view(B, N, ncols), 1).double() - colref).abs() / colref).max().item(), U23)
    del v64
    da = a.to(cuda)
    dsc, dsh = (sc.to(cuda), sh.to(cuda)) if affine else (None, None)
    tag = f"softmax/{rows}x{ncols}/{'affine' if affine else 'plain'}"
    _softmax_checks(tag + "/rows", ops.softmax_affine(da, dsc, dsh), ref, f32)
    forms = [("colsum", da)]
    if ncols == 64:
        flat = torch.empty(rows * ncols + 1, device=cuda)
        off = flat[1:].view(rows, ncols)
        off.copy_(da)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert ls.softmax_kernel(ncols, N, False) == "colsum" and ls.softmax_kernel(ncols, N, True) == "colsum64<1>"
        forms.append(("colsum-unaligned", off))
    for name, x in forms:
        out, ws = ops.softmax_affine(x, dsc, dsh, colsum_rows=N)
        _softmax_checks(f"{tag}/{name}", out, ref, f32)
        assert ws.shape == (B, 2 * ncols) and bool((ws[:, ncols:] == 0).all())
        cerr = ((ws[:, :ncols].double().cpu() - colref).abs() / colref).max().item()
        print(f"MEASURE {tag}/{name}/colsums err={cerr:.3e} floor={colfloor:.3e} bound={SUM_X * colfloor:.3e}")
        assert cerr <= SUM_X * colfloor
        del out, ws
    _free()


@pytest.mark.parametrize("P", [1, 2, 4, 8])
def test_softmax_affine_parts_every_plane_count(cuda, P):
    """test_ops_gpu.py::test_gemm_p8_fused_assignment_product runs P = 4 and P = 1 on planes that lie back to back; here every P of the
    template, with part_stride > rows * 64 (the planes are the first rows of taller ones) and the measures of this module"""
    ops = _ops()
    Bc, Np = 3, 320
    rows = Bc * Np
    g = _gen(P)
    tall = torch.randn(P, rows + 64, 64, generator=g) * 2
    parts = tall[:, :rows]
    sc, sh = 0.5 + torch.rand(64, generator=g), torch.randn(64, generator=g)
    dparts = tall.to(cuda)[:, :rows]
    assert dparts.stride(0) == (rows + 64) * 64 > rows * 64
    out, ws = ops.softmax_affine_parts(dparts, sc.to(cuda), sh.to(cuda), colsum_rows=Np)
    ref = torch.softmax(parts.double().sum(0) * sc.double() + sh.double(), dim=1)
    s32 = parts[0].clone()
    for j in range(1, P):
        s32 = s32 + parts[j]
    f32 = torch.softmax(s32 * sc + sh, dim=1)
    _softmax_checks(f"softmax_parts/P{P}", out, ref, f32)
    colref = ref.view(Bc, Np, 64).sum(1)
    colfloor = max(((_seqsum(f32.view(Bc, Np, 64), 1).double() - colref).abs() / colref).max().item(), U23)
    cerr = ((ws[:, :64].double().cpu() - colref).abs() / colref).max().item()
    print(f"MEASURE softmax_parts/P{P}/colsums err={cerr:.3e} floor={colfloor:.3e} bound={SUM_X * colfloor:.3e}")
    assert cerr <= SUM_X * colfloor and bool((ws[:, 64:] == 0).all())
    with pytest.raises(_err()):
        ops.softmax_affine_parts(torch.zeros(3, rows, 64, device=cuda), sc.to(cuda), sh.to(cuda), colsum_rows=Np)      # P = 3 is not built


# ================================================================== vlad_finalize
def _vlad_ref(vraw, asum, cw2, dt):
    """the descriptor and its normalisers from a_sum in `dt`; float32: every sum over features in sequence"""
    add = (lambda t, dim: t.sum(dim)) if dt == torch.float64 else _seqsum
    r = vraw.to(dt) - asum.to(dt).unsqueeze(1) * cw2.to(dt)
    ss = add(r * r, 1)                                                        # [B, KC]
    inv_c = 1.0 / ss.sqrt().clamp_min(1e-12)
    tot = add(ss * inv_c * inv_c, 1)
    inv_g = 1.0 / tot.sqrt().clamp_min(1e-12)
    return (r * inv_c.unsqueeze(1) * inv_g.view(-1, 1, 1)).reshape(r.shape[0], -1), inv_c, inv_g


def _vlad_refs(vraw, act, cw2):
    B, F, KC = vraw.shape
    asum64, asum32 = act.double().sum(1), _seqsum(act, 1)
    ref, inv_c, inv_g = _vlad_ref(vraw, asum64, cw2, torch.float64)
    f32, c32, g32 = _vlad_ref(vraw, asum32, cw2, torch.float32)
    terms = (vraw.double().abs() + (asum64.unsqueeze(1) * cw2.double()).abs()) * inv_c.unsqueeze(1) * inv_g.view(-1, 1, 1)
    return dict(asum=(asum64, asum32), inv_c=(inv_c, c32), inv_g=(inv_g, g32), out=(ref, f32), scale=ref.abs() + terms.reshape(B, -1))


def _vlad_compare(tag, out, aux, refs):
    for key in ("asum", "inv_c", "inv_g"):
        _check(f"{tag}/{key}", aux[key], refs[key][0], refs[key][1], refs[key][0], SUM_X)
    _check(tag + "/descriptor", out, refs["out"][0], refs["out"][1], refs["scale"], ELEM_X)
    nrm = out.double().pow(2).sum(1).sqrt().cpu()
    assert bool(((nrm - 1).abs() < 1e-5).all())


@pytest.mark.parametrize("N,F", ls.FWD_VLAD_CASES)
def test_vlad_finalize_against_fp64(cuda, N, F):
    """both a_sum regimes (ceil(N / 64) blocks, 16 chunks from N = 1024 on) at B = 44; with the a_sum of the softmax (ws=) where N % 16 == 0;
    out= a taller buffer; the aux outputs the backward consumes"""
    ops = _ops()
    B, KC = 44, 64
    g = _gen(N + F)
    vraw = torch.randn(B, F, KC, generator=g) * 3
    cw2 = torch.randn(F, KC, generator=g)
    logits = (torch.randn(B * N, KC, generator=g) * 3).to(cuda)
    if N % 16 == 0:
        dact, ws = ops.softmax_affine(logits, colsum_rows=N)
    else:
        dact, ws = ops.softmax_affine(logits), None
    act = dact.cpu().view(B, N, KC)                                          # the assignment as stored: the inputs of this op
    dv, dc = vraw.to(cuda), cw2.to(cuda)
    tall = torch.full((B + 3, F * KC), -9.0, device=cuda)
    aux = {}
    out = ops.vlad_finalize(dv, dact.view(B, N, KC), dc, out=tall, aux=aux)
    assert out.data_ptr() == tall.data_ptr() and bool((tall[B:] == -9.0).all())
    assert aux["asum"].shape == (B, KC) and aux["inv_c"].shape == (B, KC) and aux["inv_g"].shape == (B,)
    refs = _vlad_refs(vraw, act, cw2)
    _vlad_compare(f"vlad/N{N}/F{F}/two-pass", tall[:B], aux, refs)
    aux1 = {}
    plain = ops.vlad_finalize(dv, dact.view(B, N, KC), dc, aux=aux1)      # its own buffer (the atomics' order differs from launch to launch: not bit-equal)
    assert plain.shape == (B, F * KC)
    _vlad_compare(f"vlad/N{N}/F{F}/own-buffer", plain, aux1, refs)
    if ws is not None:
        aux2 = {}
        one = ops.vlad_finalize(dv, dact.view(B, N, KC), dc, aux=aux2, ws=ws)
        _vlad_compare(f"vlad/N{N}/F{F}/ws", one, aux2, refs)
    _free()


@pytest.mark.parametrize("N", [64, 1024])
def test_vlad_finalize_zero_cluster_column(cuda, N):
    """vraw[:, :, 5] = a_sum * cw2[:, 5] exactly (assignments 1 / 64, weights in multiples of 2^-8: every product and partial sum is exact
    in float32 in any order): that cluster's residual is 0, its norm is clamped at 1e-12, its column comes out 0 and the rest of the
    descriptor stays unit-norm"""
    ops = _ops()
    B, F, KC = 5, 96, 64
    g = _gen(N)
    act = torch.full((B, N, KC), 1.0 / 64)
    cw2 = torch.randint(-512, 513, (F, KC), generator=g).float() / 256
    vraw = torch.randn(B, F, KC, generator=g)
    vraw[:, :, 5] = ((N / 64.0) * cw2[:, 5].double()).float()
    assert torch.equal(vraw[:, :, 5].double(), (N / 64.0) * cw2[:, 5].double().expand(B, F))
    aux = {}
    dout = ops.vlad_finalize(vraw.to(cuda), act.to(cuda), cw2.to(cuda), aux=aux)
    out = dout.cpu().view(B, F, KC)
    assert bool((aux["asum"].cpu() == N / 64.0).all())
    assert bool((out[:, :, 5] == 0).all()) and bool(torch.isfinite(out).all())
    assert bool(((out.double().pow(2).sum((1, 2)).sqrt() - 1).abs() < 1e-6).all())
    _vlad_compare(f"vlad/zero-column/N{N}", dout, aux, _vlad_refs(vraw, act, cw2))      # inv_c of the empty cluster: 1 / 1e-12 in both


# ================================================================== linear (K <= 8), apply_transform
def _seqdot(x, w):
    """float32 x @ w.T with the products added in sequence over K"""
    acc = torch.zeros(x.shape[0], w.shape[0])
    for c in range(x.shape[1]):
        acc = acc + x[:, c:c + 1] * w[:, c]
    return acc


# every epilogue at the first layers' own shape (3 -> 64); the other K and N (N not a multiple of 64) with one epilogue each
LINEAR_CASES = [(3, 64, m) for m in ("plain", "bias", "bn-relu", "bias-bn-leaky", "bn-sigmoid")] + \
               [(8, 64, "bias-bn-leaky"), (3, 50, "bn-relu"), (8, 100, "bias"), (8, 100, "bn-sigmoid"), (1, 7, "plain")]


@pytest.mark.parametrize("K,N,mode", LINEAR_CASES)
def test_linear_small_k_against_fp64(cuda, K, N, mode):
    """the per-point first layers at M = 44 x 4096 rows; x and out= are column slices of wider tensors"""
    ops = _ops()
    M = 44 * 4096
    g = _gen(K * 100 + N)
    xw = torch.randn(M, K + 5, generator=g)
    x = xw[:, 2:2 + K]
    w = torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g) if "bias" in mode else None
    sc, sh = (torch.randn(N, generator=g), torch.randn(N, generator=g)) if "bn" in mode else (None, None)
    act = {"relu": RELU, "leaky": LEAKY, "sigmoid": SIGMOID}.get(mode.split("-")[-1], NONE)
    pre, terms, p32 = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t(), _seqdot(x, w)
    if bias is not None:
        pre, terms, p32 = pre + bias.double(), terms + bias.double().abs(), p32 + bias
    if sc is not None:
        pre, terms, p32 = pre * sc.double() + sh.double(), terms * sc.double().abs() + sh.double().abs(), p32 * sc + sh
    kw = {k: v.to(cuda) for k, v in dict(bias=bias, scale=sc, shift=sh).items() if v is not None}
    buf = torch.full((M, N + 6), -2.0, device=cuda)
    out = ops.linear(xw.to(cuda)[:, 2:2 + K], w.to(cuda), act=act, slope=SLOPE, out=buf[:, 3:3 + N], **kw)
    assert out.data_ptr() == buf[:, 3:3 + N].data_ptr()
    assert bool((buf[:, :3] == -2.0).all()) and bool((buf[:, 3 + N:] == -2.0).all())
    _check(f"linear_smallk/K{K}/N{N}/{mode}", out, _act(pre, act), _act(p32, act), _act_scale(pre, terms, act), SUM_X)
    own = ops.linear(xw.to(cuda)[:, 2:2 + K], w.to(cuda), act=act, slope=SLOPE, **kw)
    assert own.shape == (M, N) and torch.equal(own, out)
    _free()


@pytest.mark.parametrize("B", [1, 44])
def test_apply_transform_k3_per_cloud_weights(cuda, B):
    """y[m] = x[m] @ trans[m // N] on the small-K kernel's per-cloud weight addressing (rows_per_w, w_sb), against torch.bmm in float64"""
    ops = _ops()
    N, K = 4096, 3
    g = _gen(B)
    x = torch.randn(B * N, K, generator=g) * 5
    trans = torch.randn(B, K, K, generator=g)
    ref = torch.bmm(x.double().view(B, N, K), trans.double()).view(B * N, K)
    terms = torch.bmm(x.double().abs().view(B, N, K), trans.double().abs()).view(B * N, K)
    f32 = torch.zeros(B, N, K)
    for c in range(K):
        f32 = f32 + x.view(B, N, K)[:, :, c:c + 1] * trans[:, c:c + 1, :]
    buf = torch.full((B * N, K + 5), -2.0, device=cuda)
    out = ops.apply_transform(x.to(cuda), trans.to(cuda), N, out=buf[:, 1:1 + K])
    assert out.data_ptr() == buf[:, 1:1 + K].data_ptr() and bool((buf[:, 0] == -2.0).all()) and bool((buf[:, 1 + K:] == -2.0).all())
    _check(f"apply_transform/K3/B{B}", out, ref, f32.view(B * N, K), terms, SUM_X)
    assert torch.equal(ops.apply_transform(x.to(cuda), trans.to(cuda), N), out)


@pytest.mark.parametrize("B", [3, 44])
def test_apply_transform_k64_batched_gemm(cuda, B):
    """The feature transform on the batched GEMM.  ops.gemm keeps the exact f32-input MFMA for B = 3 (12288 rows: below the 16384 rows of the
    transposed short-reduction kernel, and 64 output columns are too few for the generic split-bf16 form) and takes the split-bf16
    three-product kernel lpd_gemm_x3t_rows for B = 44.  B = 3 pins the exact product: SUM_X in-sequence float32 floors.  B = 44 pins the
    split form: X3_TERM of sum |term| for the dropped lo * lo products and the operands' third bf16 piece, on top of the float32 sum.
    out= a column slice in both."""
    ops = _ops()
    from lpdnet_hip import _lib
    N, K = 4096, 64
    g = _gen(B + K)
    x = torch.randn(B * N, K, generator=g)
    trans = torch.eye(K) + 0.3 * torch.randn(B, K, K, generator=g)
    ref = torch.bmm(x.double().view(B, N, K), trans.double()).view(B * N, K)
    terms = torch.bmm(x.double().abs().view(B, N, K), trans.double().abs()).view(B * N, K)
    f32 = torch.zeros(B, N, K)
    for c in range(K):
        f32 = f32 + x.view(B, N, K)[:, :, c:c + 1] * trans[:, c:c + 1, :]
    floor = max(_scaled(f32.view(B * N, K), ref, terms, exact_zero=False), U23)
    split = bool(ops.GEMM_BF16X3 and ops.X3T_ROWS and B * N >= 16384 and _lib.load().lpd_gemm_x3t_rows_applies(N, K, K, 0, K, K))
    assert split == (B == 44), "the case no longer pins the product form its docstring names"
    bound = SUM_X * floor + (X3_TERM if split else 0.0)
    got = ops.apply_transform(x.to(cuda), trans.to(cuda), N)
    err = _scaled(got, ref, terms)
    print(f"MEASURE apply_transform/K64/B{B}/{'split-bf16' if split else 'f32-mfma'} err={err:.3e} floor={floor:.3e} bound={bound:.3e}")
    assert got.shape == (B * N, K) and err <= bound
    buf = torch.full((B * N, K + 8), -2.0, device=cuda)
    out = ops.apply_transform(x.to(cuda), trans.to(cuda), N, out=buf[:, 4:4 + K])
    assert out.data_ptr() == buf[:, 4:4 + K].data_ptr() and bool((buf[:, :4] == -2.0).all()) and bool((buf[:, 4 + K:] == -2.0).all())
    err = _scaled(out, ref, terms)
    print(f"MEASURE apply_transform/K64/B{B}/out-slice err={err:.3e} floor={floor:.3e} bound={SUM_X * floor + X3_TERM:.3e}")
    assert err <= (bound if torch.equal(out, got) else SUM_X * floor + X3_TERM)     # a strided result may take the other product form
    _free()


# ================================================================== gating
@pytest.mark.parametrize("mode", ["bn", "bias", "plain"])
@pytest.mark.parametrize("B,D", ls.FWD_GATING_CASES)
def test_gating_against_fp64(cuda, B, D, mode):
    """h * sigmoid(affine(h @ Wg)) with the column loop (D > 256), the k tail (D / 4 not a multiple of 8) and the second hrow fill trip
    (D > 1024); h and Wg are column slices of wider tensors (the wrapper allocates the result itself)"""
    ops = _ops()
    g = _gen(B * 7 + D)
    hw = torch.randn(B, D + 4, generator=g)
    Ww = torch.randn(D, D + 8, generator=g) / D ** 0.5
    h, Wg = hw[:, 1:1 + D], Ww[:, 3:3 + D]
    bias, sc, sh = torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    z = h.double() @ Wg.double()
    terms = h.double().abs() @ Wg.double().abs()
    z32 = torch.zeros(B, D)
    for k in range(D):
        z32 = z32 + h[:, k:k + 1] * Wg[k]
    kw = {}
    if mode == "bn":
        z, terms, z32 = z * sc.double() + sh.double(), terms * sc.double().abs() + sh.double().abs(), z32 * sc + sh
        kw = dict(scale=sc.to(cuda), shift=sh.to(cuda))
    elif mode == "bias":
        z, terms, z32 = z + bias.double(), terms + bias.double().abs(), z32 + bias
        kw = dict(bias=bias.to(cuda))
    s = torch.sigmoid(z)
    ref = h.double() * s
    scale = h.double().abs() * (s + s * (1 - s) * terms)
    out = ops.gating(hw.to(cuda)[:, 1:1 + D], Ww.to(cuda)[:, 3:3 + D], **kw)
    assert out.shape == (B, D)
    _check(f"gating/B{B}/D{D}/{mode}", out, ref, h * torch.sigmoid(z32), scale, SUM_X)


# ================================================================== retrieval_topk / hard_negatives
def _stable_topk(d, k):
    """(distance, index) order: a stable argsort of the float64 distances"""
    return np.argsort(d, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("nq,ndb,k", [(1, 7, 7), (5, 7, 3), (5, 300, 25), (4097, 300, 25), (5, 100, 100), (1, 64, 64), (4097, 7, 7)])
def test_retrieval_topk_exact_ties_lower_index_first(cuda, nq, ndb, k):
    """descriptors with entries in {-2 .. 2}: every norm, product and distance is a small integer, exact in float32 in the expansion
    |q|^2 + |d|^2 - 2 q.d as in the direct form; a third of the database rows are copies of other rows, and the queries are database rows"""
    rng = np.random.default_rng(nq + ndb + k)
    dim = 32
    D = rng.integers(-2, 3, (ndb, dim)).astype(np.float32)
    D[rng.integers(0, ndb, ndb // 3)] = D[rng.integers(0, ndb, ndb // 3)]
    Q = D[rng.integers(0, ndb, nq)].copy()
    Q[::2] += rng.integers(-1, 2, (Q[::2].shape[0], dim)).astype(np.float32)
    d = ((Q[:, None, :].astype(np.float64) - D[None].astype(np.float64)) ** 2).sum(-1) if nq * ndb <= 10 ** 5 else \
        (Q.astype(np.float64) ** 2).sum(1)[:, None] + (D.astype(np.float64) ** 2).sum(1)[None] - 2 * Q.astype(np.float64) @ D.astype(np.float64).T
    want = _stable_topk(d, k)
    idx, dist = _ops().retrieval_topk(torch.from_numpy(Q).to(cuda), torch.from_numpy(D).to(cuda), k)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), np.take_along_axis(d, want, 1))
    assert (np.diff(np.take_along_axis(d, want, 1), axis=1) == 0).any() or k == 1        # the case does hold ties


@pytest.mark.parametrize("bq,nc,k", [(1, 7, 7), (5, 7, 3), (5, 300, 25), (4097, 64, 10), (5, 100, 100), (2, 4000, 26)])
def test_hard_negatives_exact_ties_lower_position_first(cuda, bq, nc, k):
    """the same on the direct form; cand[b] lists some table rows twice (and copies of rows besides), which forces the positional rule"""
    rng = np.random.default_rng(bq + nc + k)
    dim, T = 48, max(2 * nc, 50)
    table = rng.integers(-2, 3, (T, dim)).astype(np.float32)
    table[rng.integers(0, T, T // 4)] = table[rng.integers(0, T, T // 4)]
    cand = np.stack([rng.permutation(T)[:nc] for _ in range(bq)]).astype(np.int32)
    rep = rng.integers(0, nc, (bq, max(1, nc // 3)))
    src = rng.integers(0, nc, (bq, max(1, nc // 3)))
    for b in range(bq):
        cand[b, rep[b]] = cand[b, src[b]]                                     # the same table row at several positions
    Q = table[cand[:, 0]].copy()
    Q[::2] += rng.integers(-1, 2, (Q[::2].shape[0], dim)).astype(np.float32)
    d = ((table[cand].astype(np.float64) - Q[:, None, :].astype(np.float64)) ** 2).sum(-1)
    want = _stable_topk(d, k)
    wide = np.zeros((T, dim + 8), np.float32)
    wide[:, :dim] = table
    pos, dist = _ops().hard_negatives(torch.from_numpy(wide).to(cuda)[:, :dim], torch.from_numpy(Q).to(cuda), torch.from_numpy(cand).to(cuda), k)
    assert pos.dtype == torch.int32 and np.array_equal(pos.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), np.take_along_axis(d, want, 1))
    assert (np.diff(np.take_along_axis(d, want, 1), axis=1) == 0).any() or k == 1


def _unit_rows(n, dim, seed):
    v = torch.randn(n, dim, generator=_gen(seed), dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float()


def _rank_checks(tag, idx, dist, d64, bound):
    """for every query and rank: the returned distance is the fp64 distance of the returned row within the bound, distances do not
    decrease, indices are distinct, and the r-th returned row is no farther than the r-th nearest plus the bound.  bound [nq, k or 1]"""
    idx, dist = idx.cpu().long(), dist.cpu().double()
    k = idx.shape[1]
    dsel = torch.gather(d64, 1, idx)
    best = torch.sort(d64, dim=1).values[:, :k]
    e1 = ((dist - dsel).abs() / bound).max().item()
    e2 = ((dsel - best) / bound).max().item()
    print(f"MEASURE {tag} |dist - d64(idx)| / bound = {e1:.3f}   (d64(idx_r) - r-th smallest) / bound = {e2:.3f}")
    assert e1 <= 1.0 and e2 <= 1.0
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    assert all(len(set(r)) == k for r in idx.tolist())
    assert int(idx.min()) >= 0 and int(idx.max()) < d64.shape[1]


@pytest.mark.parametrize("nq,ndb", [(400, 4500), (4500, 400)])
def test_retrieval_topk_real_descriptors(cuda, nq, ndb):
    """unit-norm 256-d rows at Oxford-like sizes, each query a database row plus 0.05 randn; k = 25.  Bound: 4 x the float32 floor of the
    expansion |q|^2 + |d|^2 - 2 q.d clamped at 0 (largest absolute error of a float32 CPU evaluation from the same inputs), which itself
    must respect the derived 2 dim 2^-24 (|q|^2 + |d|^2 + 2 |q.d|)"""
    dim, k = 256, 25
    D = _unit_rows(ndb, dim, ndb)
    Q = D[torch.randint(0, ndb, (nq,), generator=_gen(nq))] + 0.05 * torch.randn(nq, dim, generator=_gen(nq + 1))
    q64, db64 = Q.double(), D.double()
    d64 = (q64.pow(2).sum(1)[:, None] - 2 * q64 @ db64.t() + db64.pow(2).sum(1)[None]).clamp_min(0)
    d32 = (Q.pow(2).sum(1)[:, None] + D.pow(2).sum(1)[None] - 2.0 * (Q @ D.t())).clamp_min(0)
    ferr = (d32.double() - d64).abs()
    ceiling = 2 * dim * 2.0 ** -24 * (q64.pow(2).sum(1)[:, None] + db64.pow(2).sum(1)[None] + 2 * (q64 @ db64.t()).abs())
    assert bool((ferr <= ceiling).all())
    floor = ferr.max().item()
    print(f"MEASURE retrieval_topk/{nq}x{ndb} fp32 floor of the expansion {floor:.3e} (absolute), derived ceiling {ceiling.max().item():.3e}")
    idx, dist = _ops().retrieval_topk(Q.to(cuda), D.to(cuda), k)
    _rank_checks(f"retrieval_topk/{nq}x{ndb}", idx, dist, d64, torch.full((nq, 1), 4 * floor, dtype=torch.float64))


@pytest.mark.parametrize("nc", [4000, ls.HARD_NEG_NC_MAX])
def test_hard_negatives_real_descriptors(cuda, nc):
    """nc = 4000 (the training harness) and the largest candidate list the LDS distance table takes (144 KiB through hipFuncSetAttribute);
    the direct form sum (t - q)^2: bound 4 x its float32 floor (relative), which must respect 2 dim 2^-24"""
    dim, k, bq, T = 256, 25, 6, 40000
    table = _unit_rows(T, dim, nc)
    assert ls.hard_negatives_lds_bytes(nc) == 4 * nc
    cand = torch.stack([torch.randperm(T, generator=_gen(nc + b))[:nc] for b in range(bq)]).to(torch.int32)
    Q = table[cand[:, 17].long()] + 0.05 * torch.randn(bq, dim, generator=_gen(nc + 99))
    rows = table[cand.long()]                                                                  # [bq, nc, dim]
    d64 = (rows.double() - Q.double()[:, None]).pow(2).sum(-1)
    d32 = (rows - Q[:, None]).pow(2).sum(-1)
    rel = (d32.double() - d64).abs() / d64
    assert bool((rel <= 2 * dim * 2.0 ** -24).all())
    floor = max(rel.max().item(), U23)
    print(f"MEASURE hard_negatives/nc{nc} fp32 floor of the direct form {floor:.3e} (relative), derived ceiling {2 * dim * 2.0 ** -24:.3e}")
    pos, dist = _ops().hard_negatives(table.to(cuda), Q.to(cuda), cand.to(cuda), k)
    _rank_checks(f"hard_negatives/nc{nc}", pos, dist, d64, 4 * floor * torch.sort(d64, dim=1).values[:, :k].clamp_min(1e-30))


def test_hard_negatives_refuses_more_candidates_than_lds(cuda):
    nc = ls.HARD_NEG_NC_MAX + 1
    table = torch.zeros(nc, 16, device=cuda)
    cand = torch.arange(nc, dtype=torch.int32, device=cuda).view(1, nc)
    with pytest.raises(_err()):
        _ops().hard_negatives(table, torch.zeros(1, 16, device=cuda), cand, 5)
    torch.cuda.synchronize()


# ================================================================== metric loss, best_pos_distance
def _first_arg(t, largest):
    """first arg-max / arg-min along dim 1 (numpy's rule), as an int64 column"""
    a = t.detach().numpy()
    return torch.from_numpy((a.argmax(1) if largest else a.argmin(1)).astype(np.int64)).view(-1, 1)


def _loss_ref(q, pos, neg, other, m1, m2, use_min, lazy, ign, quad):
    """the formula in the header of csrc/lpd_loss.hip on torch autograd (any dtype); clamp passes gradient where x >= 0, max / min route to
    the FIRST extremum, the hard count is a constant.  -> (loss, info for the gradient scales)"""
    dpos = (pos - q).pow(2).sum(2)
    pstar = _first_arg(dpos, not use_min)
    positive = dpos.gather(1, pstar)                                          # [bq, 1]
    info = dict(pstar=pstar)
    total, total_abs = 0, 0

    def part(refv, m, key):
        d = (neg - refv).pow(2).sum(2)
        x = m + positive - d
        act = x >= 0
        L = torch.where(act, x, torch.zeros_like(x))
        La = torch.where(act, abs(m) + positive + d, torch.zeros_like(x))
        if lazy:
            j = _first_arg(L, True)
            t, ta = L.gather(1, j).squeeze(1), La.gather(1, j).squeeze(1)
            act = act & (torch.arange(x.shape[1]).view(1, -1) == j)
        else:
            t, ta = L.sum(1), La.sum(1)
        w = 1.0 / (float((t.detach() > 1e-16).sum()) + 1e-16) if ign else 1.0 / x.shape[0]
        info[key] = (act, w)
        return t.sum() * w, ta.detach().sum().item() * w

    l1, a1 = part(q, m1, "a1")
    total, total_abs = l1, a1
    if quad:
        l2, a2 = part(other, m2, "a2")
        total, total_abs = total + l2, total_abs + a2
    info["abs"] = total_abs
    return total, info


def _loss_inputs(bq, P, Ng, D, seed):
    g = _gen(seed)
    q = torch.randn(bq, 1, D, generator=g) / D ** 0.5
    pos = q + torch.randn(bq, P, D, generator=g) * 0.3 / D ** 0.5
    spread = torch.rand(bq, Ng, 1, generator=g) * 1.2 + 0.1                  # negatives from nearer than the positives to far: hinges on both sides of 0
    neg = q + torch.randn(bq, Ng, D, generator=g) * spread / D ** 0.5
    other = q + torch.randn(bq, 1, D, generator=g) * 0.5 / D ** 0.5
    return q, pos, neg, other


def _loss_compare(tag, tensors, m1, m2, use_min, lazy, ign, quad, cuda):
    import loss.pointnetvlad_loss as L
    q, pos, neg, other = tensors
    outs = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in tensors]
        val, info = _loss_ref(*leaves, m1, m2, use_min, lazy, ign, quad)
        if val.requires_grad:
            val.backward()
        outs[dt] = (val.detach(), [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves], info)
    ref, gref, info = outs[torch.float64]
    dl = [t.to(cuda).requires_grad_(True) for t in tensors]
    if quad:
        got = L.quadruplet_loss(*dl, m1, m2, use_min=use_min, lazy=lazy, ignore_zero_loss=ign)
    else:
        got = L.triplet_loss(dl[0], dl[1], dl[2], m1, use_min=use_min, lazy=lazy, ignore_zero_loss=ign)
    got.backward()
    _check(tag + "/loss", got.detach().view(1), ref.view(1), outs[torch.float32][0].view(1), torch.tensor([info["abs"]], dtype=torch.float64), ELEM_X)
    # sum |term| of every gradient element
    q64, p64, n64, o64 = [t.double() for t in tensors]
    a1, w1 = info["a1"]
    a2, w2 = info.get("a2", (torch.zeros_like(a1), 0.0))
    c1, c2 = a1.double() * w1, a2.double() * w2                                          # [bq, Ng]
    cpos = (c1 + c2).sum(1).view(-1, 1, 1)
    onehot = torch.zeros(p64.shape[:2]).scatter_(1, info["pstar"], 1.0).unsqueeze(2).double()
    pstar_abs = (p64.abs() * onehot).sum(1, keepdim=True)
    s_neg = 2 * (c1.unsqueeze(2) * (n64.abs() + q64.abs()) + c2.unsqueeze(2) * (n64.abs() + o64.abs()))
    s_pos = onehot * cpos * 2 * (p64.abs() + q64.abs())
    s_q = cpos * 2 * (pstar_abs + q64.abs()) + 2 * (c1.unsqueeze(2) * (n64.abs() + q64.abs())).sum(1, keepdim=True)
    s_o = 2 * (c2.unsqueeze(2) * (n64.abs() + o64.abs())).sum(1, keepdim=True)
    # dq and dother are sums over the negatives: their float32 floor adds the terms in sequence (torch's autograd adds them pairwise)
    info32 = outs[torch.float32][2]
    b1, v1 = info32["a1"]
    b2, v2 = info32.get("a2", (torch.zeros_like(b1), 0.0))
    k1, k2 = b1.float() * v1, b2.float() * v2
    ps32 = torch.gather(pos, 1, info32["pstar"].view(-1, 1, 1).expand(-1, 1, pos.shape[2]))
    seq_q = -(k1 + k2).sum(1).view(-1, 1, 1) * (2 * (ps32 - q))
    seq_o = torch.zeros_like(other)
    for n in range(neg.shape[1]):
        seq_q = seq_q + k1[:, n].view(-1, 1, 1) * (2 * (neg[:, n:n + 1] - q))
        seq_o = seq_o + k2[:, n].view(-1, 1, 1) * (2 * (neg[:, n:n + 1] - other))
    f32g = [seq_q, outs[torch.float32][1][1], outs[torch.float32][1][2], seq_o]
    names = ["q", "pos", "neg", "other"]
    for i, sc in enumerate([s_q, s_pos, s_neg, s_o]):
        if i == 3 and not quad:
            assert dl[3].grad is None
            continue
        assert bool(torch.isfinite(dl[i].grad).all())
        _check(f"{tag}/d{names[i]}", dl[i].grad, gref[i], f32g[i], sc, SUM_X if i in (0, 3) else ELEM_X)
    return got.item()


@pytest.mark.parametrize("quad", [True, False], ids=["quadruplet", "triplet"])
@pytest.mark.parametrize("use_min,lazy,ign", [(u, l, i) for u in (False, True) for l in (False, True) for i in (False, True)])
@pytest.mark.parametrize("bq,P,Ng", [(2, 2, 18), (6, 4, 40)])
def test_metric_loss_flags_against_fp64_autograd(cuda, bq, P, Ng, use_min, lazy, ign, quad):
    _loss_compare(f"metric_loss/{bq}x{P}x{Ng}/min{int(use_min)}lazy{int(lazy)}ign{int(ign)}/{'quad' if quad else 'tri'}",
                  _loss_inputs(bq, P, Ng, 256, bq + Ng), 0.5, 0.2, use_min, lazy, ign, quad, cuda)


@pytest.mark.parametrize("D", [100, 256, 300, 1000])
@pytest.mark.parametrize("lazy", [False, True])
def test_metric_loss_descriptor_sizes(cuda, D, lazy):
    """the d += 256 loops: a short single trip (100), exactly one (256), a short second (300) and four with a short last (1000)"""
    _loss_compare(f"metric_loss/D{D}/lazy{int(lazy)}", _loss_inputs(6, 4, 40, D, D), 0.5, 0.2, True, lazy, False, True, cuda)


def _grid_vec(shape, seed):
    """entries in multiples of 1/8 from -1 .. 1: every difference, square and sum below is exact in float32"""
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float() / 8


@pytest.mark.parametrize("pair_is_nearest", [True, False])
def test_metric_loss_forced_ties(cuda, pair_is_nearest):
    """exactly representable inputs.  Positives 0 and 2 are identical and are the nearest (or the farthest) of the three: where the
    selection falls on them the gradient goes to positive 0 only.  Negatives 1 and 4 are identical and the nearest to the query, so their
    hinge is the lazy maximum of the first term: negative 1 takes it, negative 4 gets nothing; without `lazy` both get the same."""
    import loss.pointnetvlad_loss as L
    bq, P, Ng, D = 3, 3, 6, 300
    q, pos, neg, other = _grid_vec((bq, 1, D), 1), _grid_vec((bq, P, D), 2), _grid_vec((bq, Ng, D), 3), _grid_vec((bq, 1, D), 4)
    pos[:, 0] = q[:, 0] + (0.125 if pair_is_nearest else 3.0)
    pos[:, 2] = pos[:, 0]
    neg[:, 1] = q[:, 0] - 0.125
    neg[:, 4] = neg[:, 1]
    for use_min in (False, True):
        for lazy in (False, True):
            _loss_compare(f"metric_loss/ties/near{int(pair_is_nearest)}/min{int(use_min)}lazy{int(lazy)}", (q, pos, neg, other), 64.0, 64.0,
                          use_min, lazy, False, True, cuda)
            dl = [t.to(cuda).requires_grad_(True) for t in (q, pos, neg, other)]
            L.quadruplet_loss(*dl, 64.0, 64.0, use_min=use_min, lazy=lazy, ignore_zero_loss=False).backward()
            gp, gn = dl[1].grad.cpu(), dl[2].grad.cpu()
            if use_min == pair_is_nearest:                                   # the selection falls on the identical pair
                assert bool((gp[:, 2] == 0).all()) and bool((gp[:, 1] == 0).all()) and bool((gp[:, 0].abs().sum(1) > 0).all())
            else:
                assert bool((gp[:, 0] == 0).all()) and bool((gp[:, 2] == 0).all()) and bool((gp[:, 1].abs().sum(1) > 0).all())
            if lazy:
                assert bool((gn[:, 4] == 0).all()) and bool((gn[:, 1].abs().sum(1) > 0).all())
            else:
                assert torch.equal(gn[:, 4], gn[:, 1]) and bool((gn[:, 1].abs().sum(1) > 0).all())


@pytest.mark.parametrize("quad", [True, False], ids=["quadruplet", "triplet"])
@pytest.mark.parametrize("lazy", [True, False])
def test_metric_loss_all_hinges_zero_under_ignore_zero_loss(cuda, quad, lazy):
    """every negative far away: every hinge is clamped to 0, the hard count is 0, the loss is 0 and every gradient is 0 and finite"""
    import loss.pointnetvlad_loss as L
    bq, P, Ng, D = 3, 3, 6, 300
    q, pos = _grid_vec((bq, 1, D), 1), _grid_vec((bq, P, D), 2)
    neg, other = torch.full((bq, Ng, D), 40.0), torch.full((bq, 1, D), -40.0)
    dl = [t.to(cuda).requires_grad_(True) for t in (q, pos, neg, other)]
    val = (L.quadruplet_loss(*dl, 0.5, 0.2, use_min=True, lazy=lazy, ignore_zero_loss=True) if quad
           else L.triplet_loss(dl[0], dl[1], dl[2], 0.5, use_min=True, lazy=lazy, ignore_zero_loss=True))
    val.backward()
    assert val.item() == 0.0
    for t in dl[:3]:
        assert bool(torch.isfinite(t.grad).all()) and bool((t.grad == 0).all())
    ref, _ = _loss_ref(q.double(), pos.double(), neg.double(), other.double(), 0.5, 0.2, True, lazy, True, quad)
    assert ref.item() == 0.0


def test_metric_loss_lds_guard(cuda):
    """the largest (bq, P, Ng) the 60-KiB guard lets through runs and matches; one negative more raises"""
    import loss.pointnetvlad_loss as L
    bq, P, Ng = ls.METRIC_LOSS_FITS
    _loss_compare(f"metric_loss/lds/{bq}x{P}x{Ng}", _loss_inputs(bq, P, Ng, 64, 7), 0.5, 0.2, True, False, False, True, cuda)
    bq, P, Ng = ls.METRIC_LOSS_REFUSED
    t = [x.to(cuda) for x in _loss_inputs(bq, P, Ng, 64, 8)]
    with pytest.raises(_err()):
        L.quadruplet_loss(*t, 0.5, 0.2, use_min=True, lazy=False, ignore_zero_loss=False)
    torch.cuda.synchronize()


@pytest.mark.parametrize("values", ["grid", "randn"])
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("D", [100, 256, 300, 1000])
def test_best_pos_distance_backward(cuda, D, P, values):
    """min / max squared distance to the positives and their gradients against fp64 autograd; P = 1: arg-min == arg-max and both gradients
    add.  `grid`: exactly representable inputs (the distances are exact), and at P = 5 positives 1 and 3 are identical and are the minimum
    (even rows) or the maximum (odd rows): positive 1 takes the gradient, positive 3 none"""
    import loss.pointnetvlad_loss as L
    bq = 8
    if values == "grid":
        q, pos = _grid_vec((bq, 1, D), D + P), _grid_vec((bq, P, D), D + P + 1)
        if P == 5:
            pos[::2, 1] = q[::2, 0] + 0.125
            pos[1::2, 1] = q[1::2, 0] + 3.0
            pos[:, 3] = pos[:, 1]
    else:
        g0 = _gen(D * P)
        q = torch.randn(bq, 1, D, generator=g0) / D ** 0.5
        pos = q + torch.randn(bq, P, D, generator=g0) * torch.rand(bq, P, 1, generator=g0) / D ** 0.5
    g = _gen(D)
    gm, gx = torch.randn(bq, generator=g), torch.randn(bq, generator=g)
    outs = {}
    for dt in (torch.float64, torch.float32):
        ql, pl = q.to(dt).clone().requires_grad_(True), pos.to(dt).clone().requires_grad_(True)
        d = (pl - ql).pow(2).sum(2) if dt == torch.float64 else _seqsum((pl - ql).pow(2), 2)
        imin, imax = _first_arg(d, False), _first_arg(d, True)
        mn, mx = d.gather(1, imin).squeeze(1), d.gather(1, imax).squeeze(1)
        (mn * gm.to(dt) + mx * gx.to(dt)).sum().backward()
        outs[dt] = (mn.detach(), mx.detach(), ql.grad, pl.grad, imin, imax)
    mn64, mx64, gq64, gp64, imin, imax = outs[torch.float64]
    dq, dp = q.to(cuda).requires_grad_(True), pos.to(cuda).requires_grad_(True)
    mn, mx = L.best_pos_distance(dq, dp)
    (mn * gm.to(cuda) + mx * gx.to(cuda)).sum().backward()
    tag = f"best_pos/D{D}/P{P}/{values}"
    _check(tag + "/min", mn, mn64, outs[torch.float32][0], mn64, SUM_X)
    _check(tag + "/max", mx, mx64, outs[torch.float32][1], mx64, SUM_X)
    if values == "grid":
        assert torch.equal(mn.detach().cpu().double(), mn64) and torch.equal(mx.detach().cpu().double(), mx64)     # exact inputs: exact distances
    q64, p64 = q.double(), pos.double()
    oh_min = torch.zeros(bq, P).scatter_(1, imin, 1.0).unsqueeze(2).double()
    oh_max = torch.zeros(bq, P).scatter_(1, imax, 1.0).unsqueeze(2).double()
    s_p = 2 * (p64.abs() + q64.abs()) * (oh_min * gm.abs().double().view(-1, 1, 1) + oh_max * gx.abs().double().view(-1, 1, 1))
    _check(tag + "/dpos", dp.grad, gp64, outs[torch.float32][3], s_p, ELEM_X)
    _check(tag + "/dq", dq.grad, gq64, outs[torch.float32][2], s_p.sum(1, keepdim=True), ELEM_X)
    if values == "grid" and P == 5:
        assert bool((dp.grad[:, 3] == 0).all()) and bool((dp.grad[:, 1].abs().sum(1) > 0).all())


# ================================================================== argument checks: errors, not faults
def test_argument_checks_raise(cuda):
    ops = _ops()
    bad = (_err(), ValueError)
    a = torch.randn(3 * 208, 64, device=cuda)
    with pytest.raises(bad):
        ops.softmax_affine(a, colsum_rows=200)                                         # not a multiple of 16
    with pytest.raises(bad):
        ops.softmax_affine(torch.randn(16, 65, device=cuda))                           # more than 64 columns
    vraw, act, cw2 = torch.randn(3, 96, 64, device=cuda), torch.rand(3, 208, 64, device=cuda), torch.randn(96, 64, device=cuda)
    with pytest.raises(bad):
        ops.vlad_finalize(vraw, act, cw2, ws=torch.zeros(3, 64, device=cuda))          # ws of the wrong shape
    with pytest.raises(bad):
        ops.vlad_finalize(vraw, act, cw2, ws=torch.zeros(4, 128, device=cuda))
    with pytest.raises(bad):
        ops.gating(torch.randn(2, 8200, device=cuda), torch.zeros(8200, 8200, device=cuda))    # D > 8192
    with pytest.raises(bad):
        ops.transpose(torch.randn(10, 7, device=cuda))                                 # 2-D
    with pytest.raises(bad):
        ops.affine_act(torch.randn(10, 8, device=cuda)[:, :6], torch.ones(6, device=cuda), torch.zeros(6, device=cuda))       # C = 6
    with pytest.raises(bad):
        ops.retrieval_topk(torch.randn(4, 32, device=cuda), torch.randn(7, 32, device=cuda), 8)                                # k > ndb
    with pytest.raises(bad):
        ops.apply_transform(torch.randn(100, 3, device=cuda), torch.randn(3, 3, 3, device=cuda), 32)                           # rows != B * N
    torch.cuda.synchronize()
    assert torch.equal(ops.mul(torch.ones(4, device=cuda), torch.full((4,), 2.0, device=cuda)).cpu(), torch.full((4,), 2.0))    # the stream still works
