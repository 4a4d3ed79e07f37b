"""Inputs, float64 references, float32 floors, number-format terms and float32 emulations of the cases of tests/tn_routes.py.  Nothing here
needs a GPU: tests/test_tn_routes_cpu.py checks the emulations against the bounds, tests/test_tn_routes_gpu.py the kernels.

Inputs (seeded, CPU).  dW = A^T B cases: column a of A times 2^-(a % 13), column b of B times 2^-(b % 7); bf16 operands are graded first and
rounded second, so the bf16 values are the exact inputs.  lpd_gemm_bf16s is a forward product: row i of A times 2^-(i % 13), column n
of W times 2^-(n % 7) (as tests/test_gemm_routes_gpu.py).  edge_dw_sel: column n of Y times 2^-(n % 7), column c of dpre times 2^-(c % 13),
about 30 % of the BatchNorm scales negative, mean / invstd the batch statistics of z = Y W2^T, red = (sum dpre, sum dpre xhat) in float64.

Reference and measure (fp64_checks.check_bound): ref = float64 of the same inputs; scale = float64 sum |term| of the element; the floor
comes from a float32 accumulation in sequence over the rows (fp64_checks.seq_matmul), never taken below 2^-23; asserted is
|got - ref| <= (TERM + 2 floors) scale per element.  TERM is the number format's, with 2^-9 per bf16 rounding as in
tests/test_gemm_routes_gpu.py (whose docstring says how to read a single element between the bound and 4 x of it):
  fp32 x fp32 rows       three products  X3_TERM = 3 * 2^-18
  bf16 A x fp32 B        two products    X2_TERM = 2^-18: the bf16 rows are exact, only the residual of B after hi + lo is lost
  gemm_bf16s             bf16 A x (W hi + W lo): X2_TERM, and the fp32 sum is stored as bf16 (check_bound(round16=True): half an ulp)
  bf16 x bf16, gemm_tn_bf16   exact products in fp32 accumulators: 0
  operand transform      A' = act(s A + t) is the float32 multiply-then-add evaluated on the CPU and taken as the exact input; + AFFINE_TERM
                         = 2^-22 as for the same loader in tests/test_gemm_routes_gpu.py, and for bf16 rows + 2^-9: A' is rounded to bf16
                         again before the products (the floor takes the unrounded A', so the rounding is counted once, in TERM)
  edge_dw_sel            dW2[c][:] = s_c (S[c][:] - m1_c s - m2_c invstd_c (W2[c][:] G - mu_c s)) with S = D^T Y, G = Y^T Y, s = 1^T Y; the
                         scale is the sum of the absolute values of the pieces, |s_c| (|D|^T |Y| + |m1_c| |s| + |m2_c invstd_c| (|W2[c]| |Y|^T |Y|
                         + |mu_c| |s|)), so the cancellation between them does not shrink it; TERM is that of the S and G products: 0 for
                         bf16 Y and dpre (one exact product), X3_TERM for fp32.  The floor sums S, G and s in float32 in sequence and
                         finishes in float64 as dw2_finish_kernel does.
A floor over very many elements costs more than the case is worth: past 2^29 multiply-adds the in-sequence sum is taken over the first
columns of A only (at least 13: every grade) and the other elements take float32(ref) -- the floor can only come out smaller, the bound tighter.
"""
import torch

from fp64_checks import AFFINE_TERM, X2_TERM, X3_TERM, _seqsum, seq_matmul, seq_matmul_x3

BIG = 2.0 ** 100           # what surrounds the operand slices and fills the rows past `rows`
LEAKY, T_SLOPE = 2, 0.2    # the operand transform of the cases
FLOOR_BUDGET = 1 << 29


def grade(n, m):
    return 2.0 ** -(torch.arange(n) % m).float()


def make_inputs(c):
    g = torch.Generator().manual_seed(c["seed"])
    w = c["wrapper"]
    M, KA, KB, nb = c["M"], c["KA"], c["KB"], c["nb"]
    if w == "gemm_bf16s":
        K, N = KA, KB
        A = (torch.randn(M, K, generator=g) * grade(M, 13).view(M, 1)).bfloat16().float()
        W = torch.randn(K, N, generator=g) * grade(N, 7).view(1, N) * K ** -0.5
        return dict(A=A, W=W)
    if w == "dw_sel":
        k, E = c["k"], M * c["k"]
        Y = torch.randn(E, 128, generator=g) * grade(128, 7)
        dpre = torch.randn(M, 128, generator=g) * grade(128, 13)
        if c["a16"]:
            Y, dpre = Y.bfloat16().float(), dpre.bfloat16().float()
        arg = torch.randint(0, k, (M, 128), generator=g).to(torch.uint8)
        W2 = torch.randn(128, 128, generator=g) / 128 ** 0.5
        gamma = torch.rand(128, generator=g) - 0.3                 # ~30 % negative scales (tests/test_ops_gpu.py _bn_for)
        Z = Y.double() @ W2.double().t()
        mean = Z.mean(0).float()
        invstd = ((Z.var(0, unbiased=False) + 1e-5) ** -0.5).float()
        scale = gamma * invstd
        zsel = Z.view(M, k, 128).gather(1, arg.long().view(M, 1, 128)).squeeze(1)
        xhat = (zsel - mean.double()) * invstd.double()
        red = torch.stack([dpre.double().sum(0), (dpre.double() * xhat).sum(0)])
        return dict(Y=Y, dpre=dpre, arg=arg, W2=W2, scale=scale, mean=mean, invstd=invstd, red=red)
    A = torch.randn(nb, M, KA, generator=g) * grade(KA, 13)
    B = torch.randn(nb, M, KB, generator=g) * grade(KB, 7)
    if c["a16"]:
        A = A.bfloat16().float()
    if c["b16"]:
        B = B.bfloat16().float()
    d = dict(A=A, B=B)
    if c["affine"]:
        sc = 0.5 + torch.rand(KA, generator=g)
        sc[::5] *= -1
        d["a_sc"], d["a_sh"] = sc, 0.3 * torch.randn(KA, generator=g)
    return d


def term_of(c):
    w = c["wrapper"]
    if w == "gemm_bf16s":
        return X2_TERM
    if w == "dw_sel":
        return 0.0 if c["a16"] else X3_TERM
    t = 0.0 if (c["a16"] and c["b16"]) else (X2_TERM if c["a16"] else X3_TERM)
    if c["affine"]:
        t += AFFINE_TERM + (2.0 ** -9 if c["a16"] else 0.0)
    return t


def transformed(c, d):
    """A' of a transform case: the float32 multiply, then add, then LeakyReLU -- the arithmetic of the loader"""
    if not c["affine"]:
        return d["A"]
    v = d["a_sc"] * d["A"] + d["a_sh"]
    return torch.where(v > 0, v, v * T_SLOPE)


def _dw_parts(d, c):
    M, k = c["M"], c["k"]
    D = torch.zeros(M, k, 128, dtype=torch.float32)
    D.scatter_(1, d["arg"].long().view(M, 1, 128), d["dpre"].view(M, 1, 128))
    return D.view(M * k, 128), d["Y"]


def _dw_finish(S, G, s, d, E, absolute=False):
    """dw2_finish_kernel in float64; absolute: the sum of the absolute values of the pieces (S, G, s given as sums of absolute values)"""
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    sc, mu, istd, W2 = f(d["scale"]), f(d["mean"]), f(d["invstd"]), f(d["W2"])
    m1, m2 = f(d["red"][0] / E), f(d["red"][1] / E)
    S, G, s = S.double(), G.double(), s.double()
    zy = W2 @ G
    sign = 1.0 if absolute else -1.0
    inner = zy + sign * mu.view(-1, 1) * s.view(1, -1)
    return sc.view(-1, 1) * (S + sign * m1.view(-1, 1) * s.view(1, -1) + sign * (m2 * istd).view(-1, 1) * inner)


def reference(c, d):
    """-> (ref, scale, f32): float64 result, float64 sum |term| per element, float32 in-sequence evaluation"""
    w = c["wrapper"]
    if w == "gemm_bf16s":
        A, W = d["A"], d["W"]
        return A.double() @ W.double(), A.double().abs() @ W.double().abs(), seq_matmul(A, W)
    if w == "dw_sel":
        D, Y = _dw_parts(d, c)
        E = c["M"] * c["k"]
        D64, Y64 = D.double(), Y.double()
        ref = _dw_finish(D64.t() @ Y64, Y64.t() @ Y64, Y64.sum(0), d, E)
        scale = _dw_finish(D64.abs().t() @ Y64.abs(), Y64.abs().t() @ Y64.abs(), Y64.abs().sum(0), d, E, absolute=True)
        f32 = _dw_finish(seq_matmul(D.t(), Y), seq_matmul(Y.t(), Y), _seqsum(Y, 0), d, E)
        return ref, scale, f32
    A1, B = transformed(c, d), d["B"]
    At64, B64 = A1.double().transpose(1, 2), B.double()
    ref, scale = At64 @ B64, At64.abs() @ B64.abs()
    nb, M, KA, KB = c["nb"], c["M"], c["KA"], c["KB"]
    cols = KA if nb * M * KA * KB <= FLOOR_BUDGET else min(KA, max(13, FLOOR_BUDGET // (nb * M * KB)))
    f32 = ref.float()
    f32[:, :cols] = seq_matmul(A1[:, :, :cols].transpose(1, 2), B)
    return ref, scale, f32


def emulate(c, d):
    """the case's own number format in float32, accumulated in sequence: three, two or one bf16 product per term (a bf16 operand has no
    lo image: its products with it are exact zeros), the transform's re-rounding for bf16 rows, the bf16 store of gemm_bf16s"""
    w = c["wrapper"]
    if w == "gemm_bf16s":
        return seq_matmul_x3(d["A"], d["W"]).bfloat16().float()
    if w == "dw_sel":
        D, Y = _dw_parts(d, c)
        return _dw_finish(seq_matmul_x3(D.t(), Y), seq_matmul_x3(Y.t(), Y), _seqsum(Y, 0), d, c["M"] * c["k"])
    A1 = transformed(c, d)
    if c["affine"] and c["a16"]:
        A1 = A1.bfloat16().float()
    return seq_matmul_x3(A1.transpose(1, 2), d["B"])
