"""Kernels whose code path depends on the launch size, run at sizes that reach those paths (tests/launch_sizes.py states each regime;
tests/test_launch_sizes_cpu.py checks the shapes reach it).

  - The fused edge-MLP kernels walk several consecutive point tiles per block once a launch needs more than one resident round of
    blocks; the last block of a launch may run short.  Eval outputs and the backward's G / gsum are per-point results: they must be
    bit-identical to a run with one tile per block (LPD_DEBUG=edge-mlp-tiles=1, a fresh interpreter).  The backward's BatchNorm1 sums
    (dbeta1, dgamma1) add up over every tile a block walks; they are held against a float64 evaluation of the formula of
    csrc/lpd_edge.hip (edge_mlp_train_bwd_kernel), in a plain regime and a biased one where sum G pre1 - beta1 sum G cancels.
  - The reductions behind lpd_reduce_grid (at most 768 blocks) and the BatchNorm-backward products (at most 256 / 512 blocks) walk
    grid-stride loops past their caps; they are held against float64 at sizes with a ragged last stride, and under
    LPD_DEBUG=reduce-grid=7 (long loops at small sizes) against the same bounds and the default launch.

Sum errors are measured against a scale that does not cancel: |got - ref| / sum |term| per channel, worst channel.
"""
import os
import subprocess
import sys

import pytest
import torch

import launch_sizes as ls
from test_ops_gpu import _bn_for, _edge_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT, SLOPE = 2, 0.01                  # LeakyReLU (ops.ACT_LEAKY), as the DG stages use it
EDGE_NAMES = sorted(ls.EDGE_SHAPES)
MODES = ["f32", "bf16", "bf16-noz"]
REGIMES = ["plain", "biased"]
EVAL_FORMS = [(128, True), (128, False), (64, True), (64, False), ("x1", False)]      # (CM = CO, exact)
# dbeta1 / dgamma1 against fp64, scaled by sum |G| / sum |G xhat1| per channel (worst channel): see test_edge_mlp_train_bwd_sums_vs_fp64
SUM_BOUND = {"f32": 2e-6, "bf16": 2e-3, "bf16-noz": 3e-2}
SUM_FLOOR = 1e-7


def _ops():
    from lpdnet_hip import ops
    return ops


def _relg(a, b):
    """_rel on the device (large tensors)"""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _digest(t):
    """a position-weighted integer sum of the raw bits (exact, order-free): equal digests <=> equal tensors, short of a collision"""
    v = t.contiguous().view(-1)
    v = v.view(torch.int16 if v.element_size() == 2 else (torch.uint8 if v.element_size() == 1 else torch.int32))
    total, step = 0, 1 << 25
    for s in range(0, v.numel(), step):
        c = v[s:s + step].long()
        w = torch.arange(s, s + c.numel(), device=c.device, dtype=torch.int64) % 1000003 + 1
        total = (total + int((c * w).sum())) % (1 << 64)
    return total, v.numel(), str(t.dtype)


def _snap(st, bn):
    """BNStats with mean / invstd rounded to bf16 and scale / shift recomputed from them: the statistics kernels add fp64 partial sums
    with atomics (order not fixed), so the fp32 statistics of two processes may differ in the last bit; these may not"""
    ops = _ops()
    mean, invstd = st.mean.bfloat16().float(), st.invstd.bfloat16().float()
    scale = bn.weight.detach() * invstd
    shift = bn.bias.detach() - mean * scale
    return ops.BNStats(scale.contiguous(), shift.contiguous(), mean.contiguous(), invstd.contiguous(), st.count)


_INPUTS = {}


def _inputs(name):
    """P, Q, idx (CPU, seeded) of one edge shape; 128 channels (the 64-channel cases take the first 64)"""
    if name not in _INPUTS:
        s = ls.EDGE_SHAPES[name]
        _INPUTS[name] = _edge_inputs(s["B"], s["N"], 128, s["k"], 7000 + s["N"])
    return _INPUTS[name]


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ eval: the fused edge MLP
def _eval_run(name, form, cuda):
    """-> dict of outputs (device) and the arguments for the reference"""
    ops = _ops()
    s = ls.EDGE_SHAPES[name]
    B, N, k = s["B"], s["N"], s["k"]
    P, Q, idx, s1, b1 = _inputs(name)
    CM, exact = (128, False) if form[0] == "x1" else form
    g = torch.Generator().manual_seed(11 + CM)
    W2 = torch.randn(CM, CM, generator=g) / CM ** 0.5
    s2, b2 = torch.randn(CM, generator=g), torch.randn(CM, generator=g)
    args = [P[:, :CM].contiguous().to(cuda), Q[:, :CM].contiguous().to(cuda), idx.to(cuda), N, s1[:CM].to(cuda), b1[:CM].to(cuda),
            W2.to(cuda), s2.to(cuda), b2.to(cuda)]
    if form[0] == "x1":
        assert ops.edge_mlp_x1_applies(B * N, N, CM, CM)
        x2p, x1p = ops.split_panels_empty(B, N, CM, cuda), ops.split_panels_empty(B, N, CM, cuda)
        ops.edge_mlp(*args, act=ACT, slope=SLOPE, out=x2p, x1_out=x1p)
        return {"x2": x2p, "x1": x1p}, args
    return {"x2": ops.edge_mlp(*args, act=ACT, slope=SLOPE, exact=exact)}, args


def _eval_ref(args, B, N, k, chunk=8192):
    """fp64: x2 = max_t act(s2 (act(s1 (P[nbr] + Q) + b1) W2^T) + b2), x1 = act(max_t (s1 (P[nbr] + Q) + b1))"""
    P, Q, idx, _, s1, b1, W2, s2, b2 = args
    M = B * N
    nb = (idx.long().view(B, N, k) + (torch.arange(B, device=P.device) * N).view(B, 1, 1)).view(M, k)
    x2, x1 = torch.empty(M, W2.shape[0], dtype=torch.float64, device=P.device), torch.empty(M, P.shape[1], dtype=torch.float64, device=P.device)
    Wd, Pd = W2.double().t(), P.double()
    for i0 in range(0, M, chunk):
        i1 = min(M, i0 + chunk)
        y = s1.double() * (Pd[nb[i0:i1]] + Q[i0:i1].double().unsqueeze(1)) + b1.double()
        m = y.max(dim=1).values
        x1[i0:i1] = torch.where(m > 0, m, m * SLOPE)
        y = torch.where(y > 0, y, y * SLOPE)
        z = torch.matmul(y, Wd) * s2.double() + b2.double()
        z = torch.where(z > 0, z, z * SLOPE)
        x2[i0:i1] = z.max(dim=1).values
    return x2, x1


def _eval_key(name, form):
    return f"eval/{name}/{form[0]}/{'exact' if form[1] else 'x3'}"


# ------------------------------------------------------------------ train: edge_mlp_train_bwd + edge_dense_bwd_apply
def _bwd_run(name, mode, regime, cuda, chain=False):
    """The forward (edge_split_fwd, edge_mlp_train) and the two backward launches on seeded inputs; every statistic the backward reads
    is snapped (_snap) so that a second process reproduces the inputs bit for bit."""
    ops = _ops()
    s = ls.EDGE_SHAPES[name]
    B, N, k = s["B"], s["N"], s["k"]
    C, M = 128, B * N
    bf16, noz = mode != "f32", mode == "bf16-noz"
    P, Q, idx, _, _ = _inputs(name)
    P, Q, idx = P.to(cuda), Q.to(cuda), idx.to(cuda)
    g = torch.Generator().manual_seed(N + 1)
    W2 = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    bn1, bn2 = _bn_for(C, 3).to(cuda).train(), _bn_for(C, 4).to(cuda).train()
    dcat = torch.randn(M, 512, generator=g)
    with torch.no_grad():
        w1 = bn1.weight
        w1.copy_(torch.where(w1.abs() < 0.2, torch.where(w1 < 0, -0.2, 0.2).to(w1), w1))
        if regime == "biased":      # |beta1| 3..5 x |gamma1|: sum G pre1 - beta1 sum G cancels; gradients with a clear mean
            sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).to(cuda)
            bn1.bias.copy_(sign * (3.0 + 2.0 * torch.rand(C, generator=g).to(cuda)) * w1.abs())
            dcat[:, 0:256] += 1.0
    dcat = dcat.to(cuda)
    dx1, dx2 = dcat[:, 0:128], dcat[:, 128:256]
    s1sum, usel, arg1, st1 = ops.edge_split_fwd(P, Q, idx, N, bn=bn1)
    del usel
    st1 = _snap(st1, bn1)
    Y, Z, zsel, arg2, st2 = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, bn2, ACT, SLOPE, bf16, store_z=not noz)
    st2 = _snap(st2, bn2)
    dpre2, red2 = ops.bn_sel_bwd_reduce(dx2, zsel, st2, ACT, SLOPE, dtype=torch.bfloat16 if bf16 else torch.float32)
    red2 = red2.float().bfloat16().double()
    G, gsum, red1 = ops.edge_mlp_train_bwd(Z, arg2, dpre2, W2, st2, red2, Y, arg1, dx1, bn1, k, ACT, SLOPE)
    graph = ops.GraphT(idx, N)
    dP, dQ = torch.empty(M, C, device=cuda), torch.empty(M, C, device=cuda)
    ops.edge_dense_bwd_apply(G, gsum, s1sum, P, Q, graph, st1, red1, k, dP=dP, dQ=dQ)
    r = dict(G=G, gsum=gsum, red1=red1, dP=dP, dQ=dQ, Z=Z, Y=Y, arg1=arg1, arg2=arg2, dpre2=dpre2, red2=red2, dx1=dx1, W2=W2, st1=st1,
             st2=st2, bn1=bn1, P=P, Q=Q, idx=idx, B=B, N=N, k=k)
    if chain:      # the materialised chain the two launches replace (tests/test_ops_gpu.py test_edge_mlp_train_bwd_equals_the_chain)
        if bf16:
            Zc = Z if Z is not None else ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, _bn_for(C, 4).to(cuda).train(), ACT,
                                                             SLOPE, True)[1]
        else:
            Zc = ops.edge_mlp_train(P, Q, idx, N, st1.scale, st1.shift, W2, _bn_for(C, 4).to(cuda).train(), ACT, SLOPE, False, z_bf16=False)[1]
        dY = (ops.gemm_bf16s_bnbwd if bf16 else ops.gemm_f32s_bnbwd)(Zc, arg2, dpre2, k, W2, st2, red2)
        del Zc
        dq_a, dp_a = torch.empty(M, C, device=cuda), torch.empty(M, C, device=cuda)
        if bf16:
            dU, dg_a, db_a = ops.edge_bn_bwd_bf16(dx1, arg1, k, Y, st1, ACT, SLOPE, dense=dY, dQ=dq_a, post_bn=bn1)
            del dY
            ops.gather_sum_rows_bf16(dU, graph, dp_a)
        else:
            dU, dg_a, db_a = ops.edge_bn_bwd(dx1, arg1, k, Y, st1, ACT, SLOPE, dense=dY, dQ=dq_a, post_bn=bn1)
            del dY
            ops.gather_sum_rows(dU, graph, dp_a)
        del dU
        r["chain"] = dict(dP=dp_a, dQ=dq_a, dgamma=dg_a, dbeta=db_a)
    return r


def _bwd_ref(r, chunk=4096):
    """float64 evaluation of the kernel comment's definition (csrc/lpd_edge.hip, edge_mlp_train_bwd_kernel) on the kernel's own forward
    outputs, then the closed-form dP / dQ of edge_dense_bwd_apply:
      dZ = s2 (delta_{t,arg2} dpre2 - m1 - xhat2 m2),  dY1e = dZ W2,  G = (dY1e + delta_{t,arg1} dx1) act'(pre1),
      dbeta1 = sum G,  dgamma1 = sum G xhat1 (xhat1 = (pre1 - beta1) / gamma1),  gsum = sum_t G,
      dU = s1 (G - dbeta1 / E - xhat dgamma1 / E) over U = P[nbr] + Q,  dQ = sum_t dU,  dP = sum of dU over the incoming edges.
    Z absent (the form without Z): Z = Y1e W2^T in fp64.  Returns the sums, sum |G| / sum |G xhat1|, gsum, the worst |G - ref| and
    max |ref G|, dP, dQ."""
    B, N, k = r["B"], r["N"], r["k"]
    M, E, C = B * N, B * N * r["k"], 128
    dev = r["G"].device
    d = torch.float64
    st1, st2 = r["st1"], r["st2"]
    s2, mu2, is2 = st2.scale.double(), st2.mean.double(), st2.invstd.double()
    m1, m2 = r["red2"][0] / E, r["red2"][1] / E
    W2 = r["W2"].double()
    beta1, gamma1 = r["bn1"].bias.detach().double(), r["bn1"].weight.detach().double()
    tk = torch.arange(k, device=dev).view(1, k, 1)
    nb = (r["idx"].long().view(B, N, k) + (torch.arange(B, device=dev) * N).view(B, 1, 1)).view(M, k)
    db = torch.zeros(C, dtype=d, device=dev)
    dg, ab, ag = torch.zeros_like(db), torch.zeros_like(db), torch.zeros_like(db)
    gsum = torch.empty(M, C, dtype=d, device=dev)
    A = torch.zeros(M, C, dtype=d, device=dev)                      # sum of G over the incoming edges of each row
    gerr, gmax = 0.0, 0.0
    for i0 in range(0, M, chunk):
        i1 = min(M, i0 + chunk)
        e0, e1 = i0 * k, i1 * k
        y = r["Y"][e0:e1].to(d)
        z = r["Z"][e0:e1].to(d) if r["Z"] is not None else y @ W2.t()
        sel2 = (r["arg2"][i0:i1].long().unsqueeze(1) == tk)
        dZ = s2 * (torch.where(sel2, r["dpre2"][i0:i1].to(d).unsqueeze(1), 0.0) - m1 - (z.view(-1, k, C) - mu2) * is2 * m2)
        gy = (dZ.view(-1, C) @ W2).view(-1, k, C)
        sel1 = (r["arg1"][i0:i1].long().unsqueeze(1) == tk)
        gy = gy + torch.where(sel1, r["dx1"][i0:i1].to(d).unsqueeze(1), 0.0)
        yv = y.view(-1, k, C)
        G = gy * torch.where(yv > 0, 1.0, SLOPE)
        xh = (torch.where(yv > 0, yv, yv / SLOPE) - beta1) / gamma1
        db += G.sum((0, 1))
        dg += (G * xh).sum((0, 1))
        ab += G.abs().sum((0, 1))
        ag += (G * xh).abs().sum((0, 1))
        gsum[i0:i1] = G.sum(1)
        A.index_add_(0, nb[i0:i1].reshape(-1), G.view(-1, C))
        gerr = max(gerr, (r["G"][e0:e1].to(d) - G.view(-1, C)).abs().max().item())
        gmax = max(gmax, G.abs().max().item())
    # dP / dQ in closed form (fp64, from the reference sums)
    s1, mu1, is1 = st1.scale.double(), st1.mean.double(), st1.invstd.double()
    n1, n2 = db / E, dg / E
    P, Q = r["P"].double(), r["Q"].double()
    flat = nb.reshape(-1)
    deg = torch.bincount(flat, minlength=M).to(d).unsqueeze(1)
    R = torch.zeros(M, C, dtype=d, device=dev).index_add_(0, flat, Q.repeat_interleave(k, dim=0))
    S = torch.zeros(M, C, dtype=d, device=dev)
    for i0 in range(0, M, 65536):
        S[i0:i0 + 65536] = P[nb[i0:i0 + 65536]].sum(1)
    dP = s1 * (A - deg * n1 - n2 * is1 * (deg * (P - mu1) + R))
    dQ = s1 * (gsum - k * n1 - n2 * is1 * (S + k * (Q - mu1)))
    return dict(dbeta=db, dgamma=dg, abs_b=ab, abs_g=ag, gsum=gsum, gerr=gerr, gmax=gmax, dP=dP, dQ=dQ)


def _sum_err(got, ref, scale):
    return ((got.double() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def _bwd_key(name, mode, regime):
    return f"bwd/{name}/{mode}/{regime}"


# ------------------------------------------------------------------ the child with one tile per block
def _child_one_tile(path):
    """LPD_DEBUG=edge-mlp-tiles=1: every eval and backward case of this file -> digests of the per-point outputs and the sums"""
    cuda = torch.device("cuda:0")
    out = {}
    for name in EDGE_NAMES:
        for form in EVAL_FORMS:
            o, _ = _eval_run(name, form, cuda)
            out[_eval_key(name, form)] = {key: _digest(v) for key, v in o.items()}
            del o
            _free()
        for mode in MODES:
            for regime in REGIMES:
                r = _bwd_run(name, mode, regime, cuda)
                out[_bwd_key(name, mode, regime)] = dict(G=_digest(r["G"]), gsum=_digest(r["gsum"]), red1=r["red1"].cpu(),
                                                         inputs=_digest(r["Y"]), dpre2=_digest(r["dpre2"]))
                del r
                _free()
    torch.save(out, path)


def _run_child(env, fn, path):
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import test_launch_sizes_gpu as t\n"
            "t.%s(%r)\n") % (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), fn, str(path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LPD_DEBUG=env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


@pytest.fixture(scope="module")
def one_tile(tmp_path_factory):
    return _run_child("edge-mlp-tiles=1", "_child_one_tile", tmp_path_factory.mktemp("one_tile") / "out.pt")


# ------------------------------------------------------------------ the tests: fused edge MLP
@pytest.mark.parametrize("form", EVAL_FORMS, ids=lambda f: f"{f[0]}-{'exact' if f[1] else 'x3'}")
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_mlp_eval_tile_loop(cuda, one_tile, name, form):
    """Eval edge MLP at a launch with a tile loop and a short last block: within the bounds of test_edge_mlp of fp64 (x1: those of
    test_edge_mlp_with_the_dg1_kagg_riding_along) and bit-identical to the launch with one tile per block."""
    ops = _ops()
    s = ls.EDGE_SHAPES[name]
    B, N, k = s["B"], s["N"], s["k"]
    assert ls.edge_launch(name, "x1" if form[0] == "x1" else "x3") == ls.EDGE_REGIMES[name]["x1" if form[0] == "x1" else "x3"]
    o, args = _eval_run(name, form, cuda)
    ref2, ref1 = _eval_ref(args, B, N, k)
    if form[0] == "x1":
        assert _relg(ops.split_to_rows(o["x2"]), ref2) < 4e-5
        assert _relg(ops.split_to_rows(o["x1"]), ref1) < 2e-5
    else:
        assert _relg(o["x2"], ref2) < (2e-5 if form[1] else 4e-5)
    want = one_tile[_eval_key(name, form)]
    for key, v in o.items():
        assert _digest(v) == want[key], key
    del o, args, ref2, ref1
    _free()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_mlp_train_bwd_sums_vs_fp64(cuda, one_tile, name, mode, regime):
    """edge_mlp_train_bwd + edge_dense_bwd_apply at a launch whose blocks walk 3 / 16 tiles (the last block 2), against float64:
      - G, gsum per element, and bit-identical to the launch with one tile per block (the same inputs: their digests match);
      - dbeta1 / dgamma1: |got - ref| / sum |G| (sum |G xhat1|) per channel, worst channel, at most SUM_BOUND and at most
        2 x the one-tile launch's error + SUM_FLOOR;
      - dP, dQ within the bounds of test_edge_mlp_train_bwd_equals_the_chain, against fp64 and (plain regime) against the chain.
    Measured (worst of the two shapes; dbeta1 / dgamma1; the one-tile launch within a few per cent of the same in every case):
      f32       plain 4.1e-8 / 4.2e-8   biased 3.4e-7 / 1.2e-7     -> SUM_BOUND 2e-6
      bf16      plain 3.8e-4 / 3.4e-4   biased 1.5e-4 / 3.8e-5     -> 2e-3  (the dZ operand of the product is rounded to bf16)
      bf16-noz  plain 7.9e-6 / 7.4e-6   biased 1.2e-2 / 2.2e-3     -> 3e-2  (the Z term is Y1e K with K rounded to bf16 once: the same
                                                                            rounding for every edge, so it does not average out of the sums)
    The fp32 accumulation of sum G / sum G pre1 over 16 tiles costs nothing measurable here: the tile loop matches one tile per block."""
    assert ls.edge_launch(name, "bwd") == ls.EDGE_REGIMES[name]["bwd"]
    bf16 = mode != "f32"
    r = _bwd_run(name, mode, regime, cuda, chain=regime == "plain")
    ref = _bwd_ref(r)
    eb, eg = _sum_err(r["red1"][0], ref["dbeta"], ref["abs_b"]), _sum_err(r["red1"][1], ref["dgamma"], ref["abs_g"])
    one = one_tile[_bwd_key(name, mode, regime)]
    eb1, eg1 = _sum_err(one["red1"][0].to(cuda), ref["dbeta"], ref["abs_b"]), _sum_err(one["red1"][1].to(cuda), ref["dgamma"], ref["abs_g"])
    gerr = ref["gerr"] / ref["gmax"]
    print(f"\nMEASURE {_bwd_key(name, mode, regime)} dbeta1 {eb:.3e} dgamma1 {eg:.3e} | one tile: dbeta1 {eb1:.3e} dgamma1 {eg1:.3e} "
          f"| G {gerr:.3e} gsum {_relg(r['gsum'], ref['gsum']):.3e} dP {_relg(r['dP'], ref['dP']):.3e} dQ {_relg(r['dQ'], ref['dQ']):.3e}")
    # the same inputs in both processes, then the same per-point outputs
    assert one["inputs"] == _digest(r["Y"]) and one["dpre2"] == _digest(r["dpre2"])
    assert one["G"] == _digest(r["G"]) and one["gsum"] == _digest(r["gsum"])
    # per element against fp64 (bf16: G is stored rounded; the form without Z takes the Z term as a bf16 product)
    gtol = {"f32": 1e-4, "bf16": 1e-2, "bf16-noz": 2e-2}[mode]
    assert gerr < gtol
    assert _relg(r["gsum"], ref["gsum"]) < gtol
    tol = 2e-2 if bf16 else 3e-4
    assert _relg(r["dP"], ref["dP"]) < tol and _relg(r["dQ"], ref["dQ"]) < tol
    # the sums: fixed bound, and no worse than one tile per block
    assert eb < SUM_BOUND[mode] and eg < SUM_BOUND[mode], (eb, eg)
    assert eb <= 2 * eb1 + SUM_FLOOR and eg <= 2 * eg1 + SUM_FLOOR, (eb, eb1, eg, eg1)
    if "chain" in r:
        c = r["chain"]
        r1 = r["red1"].float()
        # the sums also on the scale that does not cancel: the chain carries the error of its own storage mode (the bf16 chain that of
        # the stored Z).  _rel divides by max |dbeta1|, which at 10^6 edges is far below sum |G|: against the form without Z (fp64-grade
        # in the plain regime) the bf16 chain's own rounding alone measures 0.07 - 0.15 there, so _rel is kept for the forms with Z
        cb = SUM_BOUND[mode] + SUM_BOUND["bf16" if bf16 else "f32"]
        assert _sum_err(r1[0], c["dbeta"].double(), ref["abs_b"]) < cb and _sum_err(r1[1], c["dgamma"].double(), ref["abs_g"]) < cb
        if mode != "bf16-noz":
            assert _relg(r1[0], c["dbeta"]) < tol and _relg(r1[1], c["dgamma"]) < tol
        assert _relg(r["dP"], c["dP"]) < tol and _relg(r["dQ"], c["dQ"]) < tol
    del r, ref
    _free()


# ------------------------------------------------------------------ capped grids: the BatchNorm-backward products
@pytest.mark.parametrize("mode", sorted(ls.BNBWD))
def test_bnbwd_products_past_their_block_cap(cuda, mode):
    """gemm_f32s_bnbwd (<= 256 blocks) / gemm_bf16s_bnbwd (<= 512 blocks) at E = 480 000 rows (15 000 tiles: a ragged last stride)
    against fp64: dY = dZ W2, dZ = s2 (delta_{t,arg} dpre - dbeta / E - xhat dgamma / E).  Bounds of the op tests: fp32 2e-5 of the
    largest element (split-bf16 products), bf16 one rounding of the result on top."""
    ops = _ops()
    M, k = ls.BNBWD_SHAPE["M"], ls.BNBWD_SHAPE["k"]
    wanted, grid, ragged = ls.bnbwd_launch(mode, M, k)
    assert grid == ls.BNBWD[mode][1] and ragged
    E, C = M * k, 128
    g = torch.Generator().manual_seed(21)
    bf = mode == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    Z = (torch.randn(E, C, generator=g) * 2 + 0.5).to(cuda).to(dt)
    arg = torch.randint(0, k, (M, C), generator=g, dtype=torch.uint8).to(cuda)
    dpre = torch.randn(M, C, generator=g).to(cuda).to(dt)
    W2 = (torch.randn(C, C, generator=g) / C ** 0.5).to(cuda)
    scale = (torch.rand(C, generator=g) + 0.5).to(cuda)
    scale[::3] *= -1
    mean, invstd = (torch.randn(C, generator=g) * 0.5).to(cuda), (torch.rand(C, generator=g) + 0.3).to(cuda)
    st = ops.BNStats(scale, torch.zeros_like(scale), mean, invstd, E)
    red = (torch.randn(2, C, generator=g, dtype=torch.float64) * (M ** 0.5)).to(cuda)
    dY = (ops.gemm_bf16s_bnbwd if bf else ops.gemm_f32s_bnbwd)(Z, arg, dpre, k, W2, st, red)
    tk = torch.arange(k, device=cuda).view(1, k, 1)
    err, big = 0.0, 0.0
    for i0 in range(0, M, 4096):
        i1 = min(M, i0 + 4096)
        z = Z[i0 * k:i1 * k].double().view(-1, k, C)
        sel = arg[i0:i1].long().unsqueeze(1) == tk
        dZ = scale.double() * (torch.where(sel, dpre[i0:i1].double().unsqueeze(1), 0.0) - red[0] / E - (z - mean.double()) * invstd.double() * red[1] / E)
        ref = dZ.view(-1, C) @ W2.double()
        got = dY[i0 * k:i1 * k].double()
        d = (got - ref).abs()
        if bf:
            d = (d - ref.abs() * 2.0 ** -8).clamp_min(0.0)      # one rounding of the result to bf16
        err, big = max(err, d.max().item()), max(big, ref.abs().max().item())
    print(f"\nMEASURE bnbwd/{mode} {err / big:.3e}")
    assert err / big < (2e-5 if not bf else 2e-3), err / big


# ------------------------------------------------------------------ capped grids: the reductions behind lpd_reduce_grid
def _reduce_run(op, C, R, cuda):
    """-> (outputs: {name: tensor (device)}, sums: {name: (got, ref fp64, scale)}, per-element refs: {name: (ref fp64, is bf16)})"""
    ops = _ops()
    g = torch.Generator().manual_seed(1000 * C + R % 997)
    bn = torch.nn.BatchNorm1d(C).to(cuda)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=g))
        bn.weight[::5] *= -1
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
    w, b = bn.weight.detach().double(), bn.bias.detach().double()
    d = torch.float64

    def stats_of(Xd):      # BNStats from fp64 statistics (deterministic in every process)
        mean = Xd.mean(0)
        invstd = 1.0 / torch.sqrt(Xd.var(0, unbiased=False) + bn.eps)
        scale = w * invstd
        return ops.BNStats(scale.float(), (b - mean * scale).float(), mean.float(), invstd.float(), Xd.shape[0])

    def act_grad(pre):      # pre: the fp32 value the kernels test (multiply, then add), so that a pre within rounding of 0 takes their branch
        return torch.where(pre > 0, 1.0, SLOPE)

    outs, sums, elems = {}, {}, {}
    if op == "colstats":
        X = (torch.randn(R, C, generator=g) * 1.5 + 0.7).to(cuda)
        Xd = X.double()
        st = ops.bn_train_stats(X, bn)
        sums["mean"] = (st.mean, Xd.mean(0), Xd.abs().mean(0))
        ref_is = 1.0 / torch.sqrt(Xd.var(0, unbiased=False) + bn.eps)
        sums["invstd"] = (st.invstd, ref_is, ref_is)
        outs.update(mean=st.mean, invstd=st.invstd)
        return outs, sums, elems
    if op in ("bn_act_bwd", "bn_act_bwd_bf16"):
        bf = op.endswith("bf16")
        X = (torch.randn(R, C, generator=g) + 0.3).to(cuda)
        dY = (torch.randn(R, C, generator=g) / 7 + 0.05).to(cuda)
        if bf:
            X, dY = X.bfloat16(), dY.bfloat16()
        Xd, dYd = X.double(), dY.double()
        st = stats_of(Xd)
        dx, dgm, dbt = (ops.bn_act_bwd_bf16 if bf else ops.bn_act_bwd)(dY, X, st, ACT, SLOPE)
        xhat = (Xd - st.mean.double()) * st.invstd.double()
        dpre = dYd * act_grad(st.scale * X.float() + st.shift)
        rb, rg = dpre.sum(0), (dpre * xhat).sum(0)
        sums["dbeta"] = (dbt, rb, dpre.abs().sum(0))
        sums["dgamma"] = (dgm, rg, (dpre * xhat).abs().sum(0))
        elems["dX"] = (st.scale.double() * (dpre - rb / R - xhat * rg / R), bf)
        outs.update(dX=dx, dbeta=dbt, dgamma=dgm)
        return outs, sums, elems
    if op == "bn_sel_bwd_reduce":
        xsel = (torch.randn(R, C, generator=g) * 1.3 + 0.2).to(cuda)
        dOut = (torch.randn(R, C, generator=g) + 0.5).to(cuda)
        st = stats_of(xsel.double())
        for dt in (torch.float32, torch.bfloat16):
            tag = "bf16" if dt == torch.bfloat16 else "f32"
            dpre, red = ops.bn_sel_bwd_reduce(dOut, xsel, st, ACT, SLOPE, dtype=dt)
            xs = xsel.double()
            rdpre = dOut.double() * act_grad(st.scale * xsel + st.shift)
            xhat = (xs - st.mean.double()) * st.invstd.double()
            sums[f"dbeta_{tag}"] = (red[0], rdpre.sum(0), rdpre.abs().sum(0))
            sums[f"dgamma_{tag}"] = (red[1], (rdpre * xhat).sum(0), (rdpre * xhat).abs().sum(0))
            elems[f"dpre_{tag}"] = (rdpre, dt == torch.bfloat16)
            outs.update({f"dpre_{tag}": dpre, f"red_{tag}": red})
        return outs, sums, elems
    if op == "edge_split_bwd":
        N, k = 1024 if R < 4096 else 4096, 20
        B = R // N
        P = torch.randn(R, C, generator=g).to(cuda)
        Q = (torch.randn(R, C, generator=g) + 0.3).to(cuda)
        idx = torch.randint(0, N, (R, k), generator=g, dtype=torch.int32).to(cuda)
        dOut = (torch.randn(R, C, generator=g) + 0.2).to(cuda)
        bnu = _bn_for(C, C + 1).to(cuda).train()
        S, usel, arg, st = ops.edge_split_fwd(P, Q, idx, N, bn=bnu)
        st = _snap(st, bnu)
        graph = ops.GraphT(idx, N)
        dP, dQ = torch.empty(R, C, device=cuda), torch.empty(R, C, device=cuda)
        dgm, dbt = ops.edge_split_bwd(dOut, usel, arg, S, P, Q, graph, st, ACT, SLOPE, k, dP, dQ)
        E = R * k
        nb = (idx.long().view(B, N, k) + (torch.arange(B, device=cuda) * N).view(B, 1, 1)).view(R, k)
        jsel = nb.gather(1, arg.long())                                                      # [R, C] the selected neighbour of each channel
        Pd, Qd = P.double(), Q.double()
        us = Pd.gather(0, jsel) + Qd
        s, mu, iv = st.scale.double(), st.mean.double(), st.invstd.double()
        Gs = dOut.double() * act_grad(st.scale * (P.gather(0, jsel) + Q) + st.shift)
        xs = (us - mu) * iv
        rb, rg = Gs.sum(0), (Gs * xs).sum(0)
        sums["dbeta"] = (dbt, rb, Gs.abs().sum(0))
        sums["dgamma"] = (dgm, rg, (Gs * xs).abs().sum(0))
        n1, n2 = rb / E, rg / E
        flat = nb.reshape(-1)
        deg = torch.bincount(flat, minlength=R).to(d).unsqueeze(1)
        Rq = torch.zeros(R, C, dtype=d, device=cuda).index_add_(0, flat, Qd.repeat_interleave(k, dim=0))
        A = torch.zeros(R * C, dtype=d, device=cuda).index_add_(0, (jsel * C + torch.arange(C, device=cuda)).reshape(-1), Gs.reshape(-1)).view(R, C)
        Sd = Pd[nb].sum(1)
        elems["dP"] = (s * (A - deg * n1 - n2 * iv * (deg * (Pd - mu) + Rq)), False)
        elems["dQ"] = (s * (Gs - k * n1 - n2 * iv * (Sd + k * (Qd - mu))), False)
        outs.update(dP=dP, dQ=dQ, dbeta=dbt, dgamma=dgm)
        return outs, sums, elems
    raise KeyError(op)


REDUCE_SUM_BOUND = 1e-5      # |got - ref| / sum |term| per channel (statistics: / mean |x|, invstd: relative)
REDUCE_ELEM_BOUND = 1e-5     # fp32 outputs: _rel of fp64; bf16 outputs: one rounding (2^-8 of the element) on top


def _check_reduce(tag, sums, elems, outs):
    for key, (got, ref, scale) in sums.items():
        e = _sum_err(got, ref, scale)
        print(f"MEASURE {tag} {key} {e:.3e}")
        assert e < REDUCE_SUM_BOUND, (key, e)
    for key, (ref, bf) in elems.items():
        got = outs[key].double()
        dd = (got - ref).abs()
        if bf:
            dd = (dd - ref.abs() * 2.0 ** -8).clamp_min(0.0)
        e = dd.max().item() / ref.abs().max().item()
        print(f"MEASURE {tag} {key} {e:.3e}")
        assert e < REDUCE_ELEM_BOUND, (key, e)


@pytest.mark.parametrize("op,C,R", ls.REDUCE_CASES)
def test_reductions_past_the_grid_cap(cuda, op, C, R):
    """Every launch of the call wants more than 768 blocks and walks a ragged last stride: sums and per-element outputs against fp64."""
    outs, sums, elems = _reduce_run(op, C, R, cuda)
    _check_reduce(f"reduce/{op}/{C}/{R}", sums, elems, outs)
    del outs, sums, elems
    _free()


def _child_reduce_grid(path):
    cuda = torch.device("cuda:0")
    out = {}
    for op, C, R in ls.REDUCE_SMALL_CASES:
        outs, sums, elems = _reduce_run(op, C, R, cuda)
        out[f"{op}/{C}/{R}"] = {key: v.cpu() for key, v in outs.items()}
        del outs, sums, elems
    torch.save(out, path)


@pytest.fixture(scope="module")
def reduce_grid_7(tmp_path_factory):
    return _run_child(f"reduce-grid={ls.REDUCE_SMALL_CAP}", "_child_reduce_grid", tmp_path_factory.mktemp("reduce_grid") / "out.pt")


@pytest.mark.parametrize("op,C,R", ls.REDUCE_SMALL_CASES)
def test_reductions_under_a_small_odd_grid_cap(cuda, reduce_grid_7, op, C, R):
    """LPD_DEBUG=reduce-grid=7: the same operators at small sizes walk long grid-stride loops.  Their sums stay within the fp64-scaled
    bounds of the default launch; their per-element outputs equal the default launch's up to what a different order of the fp64
    atomics can change: the fp32 means of those sums by one unit, i.e. fp32 outputs within 1e-6 of the largest element, bf16 outputs
    within one unit of the element (2^-7); an output that reads no sum (bn_sel_bwd_reduce's dpre) is bit-identical."""
    outs, sums, elems = _reduce_run(op, C, R, cuda)
    _check_reduce(f"reduce/{op}/{C}/{R}/default", sums, elems, outs)
    small = {key: v.to(cuda) for key, v in reduce_grid_7[f"{op}/{C}/{R}"].items()}
    sums7 = {key: (small[key.replace("dbeta_", "red_").replace("dgamma_", "red_")][0 if key.startswith("dbeta") else 1]
                   if key.startswith(("dbeta_", "dgamma_")) else small[key], ref, scale) for key, (_, ref, scale) in sums.items()}
    _check_reduce(f"reduce/{op}/{C}/{R}/cap7", sums7, elems, small)
    for key, (ref, bf) in elems.items():
        a, b = small[key], outs[key]
        if key.startswith("dpre"):
            assert torch.equal(a, b), key
        elif bf:
            assert bool(((a.float() - b.float()).abs() <= b.float().abs() * 2.0 ** -7).all()), key
        else:
            assert _relg(a, b) < 1e-6, (key, _relg(a, b))
    del outs, sums, elems, small
    _free()
