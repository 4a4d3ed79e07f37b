"""The training step's backward kernels (csrc/lpd_train.hip) against float64, at the sizes the training step runs
(tests/launch_sizes.py states each launch regime; tests/test_launch_sizes_cpu.py checks the shapes reach it).

  - The materialised edge chain of lpdnetorigin (edge_build -> group_max -> edge_bn_bwd -> group_sum / gather_sum_rows) at the
    training shape B = 44, N = 4096, k = 20, C = 64 and at C = 128 / 256: every launch walks past the 4096-block cap of grid_for with
    a part-filled last trip.  The whole chain (autograd._EdgeChain) against an fp64 autograd of the same chain.
  - The transposed graph (lpd_graph_transpose) on both of its paths, row by row.
  - The NetVLAD head backward (vlad_finalize_bwd in every slice regime, softmax_bwd), the T-Net / max-pool pieces (colmax_arg,
    colmax_bwd, cloud_outer) and the first layer's weight gradient (dw_smallk).

Sum errors are measured against a scale that does not cancel: |got - ref| / sum |term| per element or channel, worst one.
Each test states its bounds next to the error measured on the MI355X.
"""
import pytest
import torch

import launch_sizes as ls
from oracle import synth

pytestmark = pytest.mark.gpu

LEAKY = 0.01
ACTS = {"leaky": (2, LEAKY), "relu": (1, 0.0)}        # (ops.ACT_LEAKY, slope), (ops.ACT_RELU, -)
U24 = 2.0 ** -24


def _ops():
    from lpdnet_hip import ops
    return ops


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _relg(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _scaled(got, ref, scale):
    """max |got - ref| / scale (scale: sum |term| of the same element)"""
    return ((got.double() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def _gen(seed, cuda):
    return torch.Generator(device=cuda).manual_seed(seed)


def _knn_idx(B, N, k, seed, cuda):
    """kNN graph [B, N, k] int32 of synth clouds: the in-degree spread of the real graphs"""
    pts = torch.from_numpy(synth.cloud(seed, B, N)).to(cuda)
    return _ops().knn(pts.transpose(1, 2).contiguous(), k)


def _nbr(idx, B, N):
    """global neighbour rows [M, k] (int64)"""
    k = idx.shape[-1]
    return (idx.long().view(B, N, k) + (torch.arange(B, device=idx.device) * N).view(B, 1, 1)).view(B * N, k)


def _bn(C, seed, cuda):
    """train-mode BatchNorm with |weight| >= 0.3 (about a third negative: the arg-min selection) and running statistics to update"""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        w = 0.3 + torch.rand(C, generator=g)
        bn.weight.copy_(torch.where(torch.rand(C, generator=g) < 0.35, -w, w))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(cuda).train()


def _act64(pre, act, slope):
    return torch.where(pre > 0, pre, pre * (slope if act == 2 else 0.0))


# ------------------------------------------------------------------ A. the materialised edge chain, op by op
STAT_BOUND = 2e-7        # mean: / mean |U|; invstd, scale, running statistics: relative
OUT_ULPS = 3.0           # group_max out: |got - ref| in units of 2^-24 (|scale xsel| + |shift|)
SUM_BOUND = 2e-7         # dgamma / dbeta: / sum |term| per channel
DX_BOUND = 5e-7          # dX: / max |ref|
DQ_BOUND = 5e-6          # dQ: / sum_t of the dX terms' |.| per element
GSUM_BOUND = 2e-6        # group_sum: / sum_t |dX| per element
CHUNK = 8192             # points per chunk of the fp64 references


def _first_index(mask, k):
    """first t with mask[:, t, :] (k where none)"""
    tk = torch.arange(k, device=mask.device).view(1, k, 1)
    return torch.where(mask, tk, k).min(1).values


def _check_group_max(X, k, st, act, slope, tag):
    """group_max(keep_sel=True) on X [M k, C] -> (arg, xsel); arg / xsel exactly, out in ulps of fp64"""
    ops = _ops()
    M, C = X.shape[0] // k, X.shape[1]
    buf = torch.full((M, C + 8), -5.0, device=X.device)
    out = buf[:, 4:4 + C]
    arg, xsel = ops.group_max(X, k, st.scale, st.shift, act, slope, out, keep_sel=True)
    pos = st.scale >= 0
    ulps, ties = 0.0, 0
    for i0 in range(0, M, CHUNK):
        i1 = min(M, i0 + CHUNK)
        x = X[i0 * k:i1 * k].view(-1, k, C)
        mx, mn = x.max(1).values, x.min(1).values
        want = torch.where(pos, _first_index(x == mx.unsqueeze(1), k), _first_index(x == mn.unsqueeze(1), k))
        assert torch.equal(arg[i0:i1].long(), want), tag
        assert torch.equal(xsel[i0:i1], torch.where(pos, mx, mn)), tag
        ties += int(((x == torch.where(pos, mx, mn).unsqueeze(1)).sum(1) > 1).sum())
        xs = xsel[i0:i1].double()
        sx = st.scale.double() * xs
        ref = _act64(sx + st.shift.double(), act, slope)
        ulps = max(ulps, ((out[i0:i1].double() - ref).abs() / (U24 * (sx.abs() + st.shift.double().abs())).clamp_min(1e-300)).max().item())
    assert (buf[:, :4] == -5.0).all() and (buf[:, 4 + C:] == -5.0).all(), tag
    return arg, xsel, ulps, ties / (M * C)


def _edge_bn_bwd_ref(X, arg, dOut, dense, st, act, slope, k):
    """float64 of out = max_t act(BN(X)) backward with the selection fixed to `arg` and the BNStats `st`:
      gy = dense + delta_{t,arg} dOut,  dpre = gy act'(pre) (pre = the fp32 value the kernels test),  xhat = (X - mean) invstd,
      dbeta = sum dpre,  dgamma = sum dpre xhat,  dX = scale (dpre - dbeta / E - xhat dgamma / E),  dQ = sum_t dX.
    -> (dbeta, dgamma, sum |dpre|, sum |dpre xhat|, a function of the chunk -> (dX [n k, C], sum_t of |scale| (|dpre| + |dbeta / E|
    + |xhat dgamma / E|) [n, C]: the scale of dQ that does not cancel))"""
    M, C = arg.shape
    E = M * k
    d = torch.float64
    sc, sh, mu, iv = st.scale, st.shift, st.mean.double(), st.invstd.double()
    ns = slope if act == 2 else 0.0
    tk = torch.arange(k, device=X.device).view(1, k, 1)

    def terms(i0, i1):
        x = X[i0 * k:i1 * k].view(-1, k, C)
        gy = torch.where(arg[i0:i1].long().unsqueeze(1) == tk, dOut[i0:i1].to(d).unsqueeze(1), 0.0)
        if dense is not None:
            gy = gy + dense[i0 * k:i1 * k].view(-1, k, C).to(d)
        dpre = gy * torch.where(sc * x + sh > 0, 1.0, ns).to(d)
        return dpre, (x.to(d) - mu) * iv

    db = torch.zeros(C, dtype=d, device=X.device)
    dg, ab, ag = torch.zeros_like(db), torch.zeros_like(db), torch.zeros_like(db)
    for i0 in range(0, M, CHUNK):
        dpre, xh = terms(i0, min(M, i0 + CHUNK))
        db += dpre.sum((0, 1))
        dg += (dpre * xh).sum((0, 1))
        ab += dpre.abs().sum((0, 1))
        ag += (dpre * xh).abs().sum((0, 1))

    def dx(i0, i1):
        dpre, xh = terms(i0, i1)
        r = sc.double() * (dpre - db / E - xh * dg / E)
        return r.view(-1, C), (sc.double().abs() * (dpre.abs() + (db / E).abs() + (xh * dg / E).abs())).sum(1)
    return db, dg, ab, ag, dx


@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("has_q", [True, False], ids=["pq", "p"])
@pytest.mark.parametrize("name", sorted(ls.CHAIN_SHAPES))
def test_edge_chain_ops_past_the_grid_cap(cuda, name, has_q, act):
    """edge_build (with its fp64 statistics), group_max(keep_sel=True), edge_bn_bwd in its gather, xsel and dense + dQ forms and
    group_sum at sizes where every launch passes the 4096-block cap (2.75 / 2.125 / 2.25 trips at C = 64 / 128 / 256), on a kNN graph:
      - U = P[nbr] + Q bit for bit; mean / invstd / scale within STAT_BOUND of fp64, running statistics like torch.nn.BatchNorm;
      - arg the first arg-max (scale >= 0) / arg-min (scale < 0) and xsel = X at arg exactly, also on X in multiples of 1/8 (ties in
        most rows); out within OUT_ULPS of fp64 act(scale xsel + shift);
      - dgamma / dbeta within SUM_BOUND of sum |term|, dX within DX_BOUND of max |ref|, dQ and group_sum within DQ_BOUND of sum_t |dX|.
    Measured on the MI355X, worst of the 12 cases (bound):
      statistics 5.9e-8 (2e-7: one fp32 rounding of the fp64 values); out 1.98 ulps, 1.45 on the tied inputs (3); 74 % of the
      quantised selections tie; dbeta / dgamma 8.6e-10 / 1.5e-9 (2e-7: the fp32 result of a non-cancelling sum may be off by 6e-8);
      dX 1.6e-7 (5e-7); dQ 1.8e-6 (5e-6); group_sum 6.7e-7 (2e-6)."""
    ops = _ops()
    B, N, k, C = ls.CHAIN_SHAPES[name]
    for kernel in ls.CHAIN_KERNELS:
        assert ls.chain_launch(kernel, B * N, C)[1] == ls.GRID_CAP
    M, E = B * N, B * N * k
    a, slope = ACTS[act]
    g = _gen(100 * C + 2 * has_q + (act == "relu"), cuda)
    pq = torch.randn(M, 2 * C, device=cuda, generator=g)
    pq[:, C:] += 0.5
    P, Q = pq[:, :C], (pq[:, C:] if has_q else None)             # column halves of one buffer, as _EdgeChain passes them
    idx = _knn_idx(B, N, k, C + 7, cuda)
    nbr = _nbr(idx, B, N)
    bn = _bn(C, C + has_q, cuda)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    U, st = ops.edge_build(P, Q, idx, N, bn=bn)
    # U bit for bit, and the fp64 statistics of U
    s1 = torch.zeros(C, dtype=torch.float64, device=cuda)
    sa = torch.zeros_like(s1)
    for i0 in range(0, M, CHUNK):
        i1 = min(M, i0 + CHUNK)
        want = P[nbr[i0:i1]] + (Q[i0:i1].unsqueeze(1) if has_q else 0.0)
        u = U[i0 * k:i1 * k].view(-1, k, C)
        assert torch.equal(u, want)
        s1 += u.double().sum((0, 1))
        sa += u.double().abs().sum((0, 1))
    mean = s1 / E
    s2 = torch.zeros_like(s1)
    for i0 in range(0, M, CHUNK):
        s2 += ((U[i0 * k:min(M, i0 + CHUNK) * k].double() - mean) ** 2).sum(0)
    var = s2 / E
    invstd = 1.0 / torch.sqrt(var + bn.eps)
    w = bn.weight.detach().double()
    errs = {"mean": ((st.mean.double() - mean).abs() / (sa / E)).max().item(),
            "invstd": ((st.invstd.double() - invstd).abs() / invstd).max().item(),
            "scale": ((st.scale.double() - w * invstd).abs() / (w * invstd).abs()).max().item(),
            "shift": ((st.shift.double() - (bn.bias.double() - mean * w * invstd)).abs()
                      / (bn.bias.double().abs() + (mean * w * invstd).abs())).max().item()}
    rm = 0.9 * rm0.double() + 0.1 * mean
    rv = 0.9 * rv0.double() + 0.1 * var * E / (E - 1)
    errs["running_mean"] = ((bn.running_mean.double() - rm).abs() / (0.9 * rm0.double().abs() + 0.1 * sa / E)).max().item()
    errs["running_var"] = ((bn.running_var.double() - rv).abs() / rv).max().item()
    assert int(bn.num_batches_tracked) == 1
    tag = f"chain/{name}/{'pq' if has_q else 'p'}/{act}"
    print(f"\nMEASURE {tag} edge_build " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    for key, v in errs.items():
        assert v < STAT_BOUND, (key, v)
    # group_max on U, then on values in multiples of 1/8 (exact ties)
    arg, xsel, ulps, _ = _check_group_max(U, k, st, a, slope, tag)
    Xq = torch.randint(-4, 5, (E, C), device=cuda, generator=g, dtype=torch.float32) / 8.0
    _, _, ulps_q, tie_frac = _check_group_max(Xq, k, st, a, slope, tag + "/ties")
    del Xq
    print(f"MEASURE {tag} group_max out {ulps:.2f} ulps, ties: out {ulps_q:.2f} ulps, {tie_frac:.2f} of the selections tie")
    assert ulps < OUT_ULPS and ulps_q < OUT_ULPS and tie_frac > 0.5
    # edge_bn_bwd: gather form, xsel form, dense form with dQ
    dOut = torch.randn(M, C + 8, device=cuda, generator=g)[:, 4:4 + C]
    dense = 0.2 * torch.randn(E, C, device=cuda, generator=g)
    dense0 = dense.clone()                                       # the dense form overwrites `dense` with dX
    ref_sel = _edge_bn_bwd_ref(U, arg, dOut, None, st, a, slope, k)
    ref_dense = _edge_bn_bwd_ref(U, arg, dOut, dense0, st, a, slope, k)
    dQbuf = torch.full((M, 2 * C), -3.0, device=cuda)
    forms = {"gather": lambda: ops.edge_bn_bwd(dOut, arg, k, U, st, a, slope),
             "xsel": lambda: ops.edge_bn_bwd(dOut, arg, k, U, st, a, slope, xsel=xsel),
             "dense": lambda: ops.edge_bn_bwd(dOut, arg, k, U, st, a, slope, dense=dense, dQ=dQbuf[:, C:])}
    for form, run in forms.items():
        ref = ref_dense if form == "dense" else ref_sel
        dX, dgam, dbet = run()
        db, dg, ab, ag, dxf = ref
        eb, eg = _scaled(dbet, db, ab), _scaled(dgam, dg, ag)
        ex, eq, big = 0.0, 0.0, 0.0
        for i0 in range(0, M, CHUNK):
            i1 = min(M, i0 + CHUNK)
            r, rabs = dxf(i0, i1)
            ex = max(ex, (dX[i0 * k:i1 * k].double() - r).abs().max().item())
            big = max(big, r.abs().max().item())
            if form == "dense":
                eq = max(eq, _scaled(dQbuf[i0:i1, C:], r.view(-1, k, C).sum(1), rabs))
        print(f"MEASURE {tag} edge_bn_bwd/{form} dbeta {eb:.2e} dgamma {eg:.2e} dX {ex / big:.2e}" + (f" dQ {eq:.2e}" if form == "dense" else ""))
        assert eb < SUM_BOUND and eg < SUM_BOUND, (form, eb, eg)
        assert ex / big < DX_BOUND, (form, ex / big)
        assert eq < DQ_BOUND, (form, eq)
        if form == "dense":
            assert dX.data_ptr() == dense.data_ptr() and (dQbuf[:, :C] == -3.0).all()
        # group_sum into a column slice of a wider buffer, as _EdgeChain.bwd does (dpq[:, c:])
        if form == "xsel":
            gbuf = torch.full((M, 2 * C), -3.0, device=cuda)
            ops.group_sum(dX, k, gbuf[:, C:])
            es = 0.0
            for i0 in range(0, M, CHUNK):
                i1 = min(M, i0 + CHUNK)
                x = dX[i0 * k:i1 * k].view(-1, k, C).double()
                es = max(es, _scaled(gbuf[i0:i1, C:], x.sum(1), x.abs().sum(1)))
            print(f"MEASURE {tag} group_sum {es:.2e}")
            assert es < GSUM_BOUND and (gbuf[:, :C] == -3.0).all()
            del gbuf
        del dX
    del U, dense, dense0, dQbuf, pq, ref_sel, ref_dense
    _free()


# ------------------------------------------------------------------ A. the chain as autograd._EdgeChain runs it
CAP_BOUND = {"dpq": 2e-5, "dw_b": 1e-5, "sums": 2e-7}


@pytest.mark.parametrize("has_q,act", [(True, "leaky"), (False, "relu")], ids=["dg-leaky", "sn-relu"])
def test_edge_chain_against_fp64_autograd_at_the_training_shape(cuda, has_q, act):
    """autograd._EdgeChain.fwd / .bwd at B = 44, N = 4096, k = 20, C = 64 (the forward inside ops.train_forward_gemm(B), as
    _LPDNetOrignTrainFn runs it) against a float64 torch autograd of the same chain on the same inputs:
      gather (+ Q) -> BatchNorm (batch statistics) -> act -> 1x1 product -> BatchNorm -> act -> max over k.
    The fp64 side takes the GPU's discrete decisions: the arg of the max and the branch of each activation (a pre-activation within
    rounding of 0 may fall on either side).  dPQ within CAP_BOUND of max |ref|; dW_b (a sum over the edges that cancels: the
    BatchNorm backward makes sum_e dz = 0) and the four BatchNorm parameter gradients within CAP_BOUND of sum |term| per element.
    Measured on the MI355X (bound): dPQ 5.8e-6 (2e-5), dW_b 1.9e-6 (1e-5), BatchNorm sums 4.0e-8 (2e-7).  The model-level gradient
    gates are 1e-2 / 3e-3."""
    from lpdnet_hip import autograd
    ops = _ops()
    B, N, k, C = ls.CHAIN_SHAPES["c64"]
    M = B * N
    a, slope = ACTS[act]
    g = _gen(17 + has_q, cuda)
    pq = torch.randn(M, 2 * C if has_q else C, device=cuda, generator=g)
    idx = _knn_idx(B, N, k, 11, cuda)
    bn_a, bn_b = _bn(C, 1, cuda), _bn(C, 2, cuda)
    w_b = torch.randn(C, C, device=cuda, generator=g) / C ** 0.5
    out = torch.empty(M, C, device=cuda)
    with ops.train_forward_gemm(B):
        S = autograd._EdgeChain.fwd(pq, C, has_q, idx, N, k, bn_a, w_b, bn_b, a, slope, out)
    assert int(S["arg"].max()) < k                                        # (the fp64 side gathers at it)
    dout = torch.randn(M, C, device=cuda, generator=g)
    arg = S["arg"].long()
    mask_a = S["ya"] > 0                                                  # the branch the GPU took at every edge of layer a
    pre_b = S["st_b"].scale * S["zsel"] + S["st_b"].shift                 # ... and at the selected edges of layer b
    mask_b = pre_b > 0
    dpq, dw_b, dg_b, db_b, dg_a, db_a = autograd._EdgeChain.bwd(dout, S, w_b, idx, N, k, C, has_q, a, slope)
    del S
    _free()
    # float64 autograd
    d = torch.float64
    ns = slope if a == 2 else 0.0

    def leaf(t):
        return t.detach().to(d).requires_grad_(True)
    P64 = leaf(pq[:, :C])
    Q64 = leaf(pq[:, C:]) if has_q else None
    ga, ba, gb, bb, W64 = leaf(bn_a.weight), leaf(bn_a.bias), leaf(bn_b.weight), leaf(bn_b.bias), leaf(w_b)
    scales = {}

    def keep_scales(name, pre_t, gam, bet):
        def hook(gr):
            with torch.no_grad():
                xh = (pre_t.detach() - bet.detach()) / gam.detach()         # pre = gamma xhat + beta
                scales[name] = (gr.abs().sum(0), (gr * xh).abs().sum(0))
        return hook
    nbr = _nbr(idx, B, N).view(-1)
    u = P64[nbr]
    if has_q:
        u = (u.view(M, k, C) + Q64.unsqueeze(1)).view(-1, C)
    pa = torch.nn.functional.batch_norm(u, None, None, ga, ba, training=True, eps=bn_a.eps)
    pa.register_hook(keep_scales("a", pa, ga, ba))
    ya = torch.where(mask_a, pa, pa * ns)
    z = ya @ W64.t()

    def keep_w_scale(gz):
        with torch.no_grad():
            scales["w"] = gz.abs().t() @ ya.detach().abs()
    z.register_hook(keep_w_scale)
    pb = torch.nn.functional.batch_norm(z, None, None, gb, bb, training=True, eps=bn_b.eps)
    pb.register_hook(keep_scales("b", pb, gb, bb))
    sel = pb.view(M, k, C).gather(1, arg.unsqueeze(1)).squeeze(1)
    o = torch.where(mask_b, sel, sel * ns)
    (o * dout.to(d)).sum().backward()
    del u, pa, ya, z, pb, sel, o
    ref_dpq = torch.cat([P64.grad, Q64.grad], 1) if has_q else P64.grad
    errs = {"dpq": _relg(dpq, ref_dpq), "dw_b": _scaled(dw_b, W64.grad, scales["w"])}
    sums = {"dbeta_b": _scaled(db_b, bb.grad, scales["b"][0]), "dgamma_b": _scaled(dg_b, gb.grad, scales["b"][1]),
            "dbeta_a": _scaled(db_a, ba.grad, scales["a"][0]), "dgamma_a": _scaled(dg_a, ga.grad, scales["a"][1])}
    print(f"\nMEASURE capstone/{'dg' if has_q else 'sn'}/{act} " + " ".join(f"{key} {v:.2e}" for key, v in {**errs, **sums}.items()))
    assert errs["dpq"] < CAP_BOUND["dpq"] and errs["dw_b"] < CAP_BOUND["dw_b"], errs
    assert max(sums.values()) < CAP_BOUND["sums"], sums
    del P64, Q64, ref_dpq, dpq
    _free()


# ------------------------------------------------------------------ B. the transposed graph
GATHER_BOUND = 1e-6      # gather_sum_rows: / sum |dU| over the incoming edges, per element


def _graph_idx(name, cuda):
    B, N, k, _ = ls.GRAPH_CASES[name]
    if name == "global":      # random rows, a hub and rows of in-degree 0 (j = 3 mod 7), as the op test builds them
        g = _gen(N, cuda)
        idx = torch.randint(0, N, (B, N, k), device=cuda, generator=g, dtype=torch.int32)
        idx = torch.where(idx % 7 == 3, (idx + 1) % N, idx)
        idx[:, :, 0] = idx[:, :1, 0]
        return idx
    return _knn_idx(B, N, k, N + k, cuda)


@pytest.mark.parametrize("name", sorted(ls.GRAPH_CASES))
def test_graph_transpose_row_by_row(cuda, name):
    """ops.GraphT (lpd_graph_transpose) on the global-atomic path (N = 40 000) and the LDS path (the training shape; N = 16384, k = 64):
    rowptr equal to the running sum of the per-cloud in-degrees (bincount), each row's edges equal to its incoming edges as a sorted
    list; gather_sum_rows into a column slice within GATHER_BOUND of fp64 (C = 64 at the training shape: 4096 blocks, 2.75 trips).
    Measured on the MI355X: gather_sum_rows 2.0e-7 (GATHER_BOUND 1e-6)."""
    ops = _ops()
    B, N, k, path = ls.GRAPH_CASES[name]
    assert ls.graph_transpose_path(N) == path
    M, E = B * N, B * N * k
    idx = _graph_idx(name, cuda)
    flat = _nbr(idx, B, N).reshape(-1)
    graph = ops.GraphT(idx, N)
    deg = torch.bincount(flat, minlength=M)
    want = torch.zeros(M + 1, dtype=torch.int64, device=cuda)
    want[1:] = torch.cumsum(deg, 0)
    assert torch.equal(graph.rowptr.long(), want)
    if name == "global":
        assert int(deg.max()) >= N and int((deg == 0).sum()) > M // 10       # the hub and the rows nobody points to
    seg = torch.repeat_interleave(torch.arange(M, device=cuda), deg)
    got = torch.sort(seg * E + graph.edges.long()).values
    assert torch.equal(got, seg * E + torch.argsort(flat, stable=True))
    del seg, got
    C = 128 if name == "global" else 64
    dU = torch.randn(E, C, device=cuda, generator=_gen(C + N, cuda))
    buf = torch.full((M, C + 8), 3.0, device=cuda)
    ops.gather_sum_rows(dU, graph, buf[:, 4:4 + C])
    ref = torch.zeros(M, C, dtype=torch.float64, device=cuda).index_add_(0, flat, dU.double())
    scale = torch.zeros(M, C, dtype=torch.float64, device=cuda).index_add_(0, flat, dU.abs().double())
    e = _scaled(buf[:, 4:4 + C], ref, torch.where(scale > 0, scale, 1.0))
    print(f"\nMEASURE graph/{name} gather_sum_rows C={C} {e:.2e}")
    assert e < GATHER_BOUND
    assert (buf[:, :4] == 3.0).all() and (buf[:, 4 + C:] == 3.0).all()
    del dU, buf, ref, scale
    _free()


# ------------------------------------------------------------------ C. the NetVLAD head backward
VLAD_BOUND = 1e-5        # dVraw: / the sum of the terms' |.| per element (T below)
VLAD_SUM_BOUND = 1e-6    # dasum, dcw2: / the same sums over T


@pytest.mark.parametrize("B,F", sorted(ls.VLAD_BWD_CASES))
def test_vlad_finalize_bwd_in_every_regime(cuda, B, F):
    """vlad_finalize_bwd after the fp32 forward vlad_finalize(..., aux=aux), at G = 8 / 4 / 2 / 1 slices per cloud and on the
    one-block-per-cloud kernel (B = 520; F = 32 < 8 G), against a float64 autograd of r = vraw - asum cw2, per-cluster L2
    normalisation over f, flatten, L2 normalisation (clamps at 1e-12, as the oracle's netvlad).  Scaled by T, the terms of
    dr = ic (du - u <du, u>), du = ig (dv - v <dv, v>) with every sum taken over |term| (the kernels' fp32 dot products): dVraw within VLAD_BOUND of T per element,
    dasum = -sum_f dr cw2 and dcw2 = -sum_b asum dr within VLAD_SUM_BOUND of the same sums over T.
    Measured on the MI355X, worst regime: dVraw 2.5e-6 (1e-5), dasum 3.8e-8 and dcw2 1.9e-7 (1e-6)."""
    ops = _ops()
    KC = 64
    assert ls.vlad_bwd_slices(B, F) == ls.VLAD_BWD_CASES[(B, F)]
    g = _gen(B * F, cuda)
    vraw = torch.randn(B, F, KC, device=cuda, generator=g)
    act = torch.softmax(2 * torch.randn(B, 96, KC, device=cuda, generator=g), dim=-1)
    cw2 = torch.randn(F, KC, device=cuda, generator=g)
    aux = {}
    v = ops.vlad_finalize(vraw, act, cw2, aux=aux)
    dOut = torch.randn(B, F * KC, device=cuda, generator=g)
    dVraw, dasum, dcw2 = ops.vlad_finalize_bwd(dOut, v, aux, cw2, B, F, KC)
    d = torch.float64
    vr, asum, c2 = (t.detach().to(d).requires_grad_(True) for t in (vraw, aux["asum"], cw2))
    r = vr - asum.unsqueeze(1) * c2.unsqueeze(0)
    r = r / torch.clamp(torch.sqrt((r * r).sum(1, keepdim=True)), min=1e-12)
    r = r.reshape(B, F * KC)
    r = r / torch.clamp(torch.sqrt((r * r).sum(1, keepdim=True)), min=1e-12)
    (r * dOut.to(d)).sum().backward()
    dr = vr.grad
    with torch.no_grad():       # T: the terms of dr = ic (du - u <du, u>), du = ig (dv - v <dv, v>), every sum taken over |term|
        r0 = vr - asum.unsqueeze(1) * c2.unsqueeze(0)
        ic = 1.0 / r0.norm(dim=1, keepdim=True)
        u = r0 * ic
        ig = 1.0 / u.reshape(B, -1).norm(dim=1).view(B, 1, 1)
        v64, dv = u * ig, dOut.to(d).view(B, F, KC)
        du_abs = ig * (dv.abs() + v64.abs() * (dv * v64).abs().sum((1, 2), keepdim=True))
        T = ic * (du_abs + u.abs() * (du_abs * u.abs()).sum(1, keepdim=True))
    e_v = _scaled(dVraw, dr, T)
    e_a = _scaled(dasum, asum.grad, (T * c2.detach().abs().unsqueeze(0)).sum(1))
    e_c = _scaled(dcw2, c2.grad, (asum.detach().abs().unsqueeze(1) * T).sum(0))
    print(f"\nMEASURE vlad_bwd/B={B}/F={F}/G={ls.vlad_bwd_slices(B, F)} dVraw {e_v:.2e} dasum {e_a:.2e} dcw2 {e_c:.2e}")
    assert e_v < VLAD_BOUND and e_a < VLAD_SUM_BOUND and e_c < VLAD_SUM_BOUND, (e_v, e_a, e_c)


SOFTMAX_BOUND = 1e-6     # / A (|g| + sum_c |A g|) per element


@pytest.mark.parametrize("with_dasum", [True, False], ids=["dasum", "no-dasum"])
@pytest.mark.parametrize("rows,rpc", [(44 * 4096, 4096), (3 * 4097, 4097)], ids=["train", "rows%4=3"])
def test_softmax_bwd(cuda, rows, rpc, with_dasum):
    """softmax_bwd at the training step's 180 224 rows x 64 clusters and at a row count that is not a multiple of 4 (the last block
    part-filled): dS = A (g - sum_c A g), g = dA + dasum[cloud], against fp64 within SOFTMAX_BOUND.  Measured on the MI355X: 3.4e-7."""
    ops = _ops()
    g = _gen(rows + with_dasum, cuda)
    A = torch.softmax(3 * torch.randn(rows, 64, device=cuda, generator=g), dim=-1)
    dA = torch.randn(rows, 64, device=cuda, generator=g)
    dasum = torch.randn(rows // rpc, 64, device=cuda, generator=g) if with_dasum else None
    dS = ops.softmax_bwd(A, dA, dasum, rpc)
    gd = dA.double() + (dasum.double().repeat_interleave(rpc, 0) if with_dasum else 0.0)
    Ad = A.double()
    ref = Ad * (gd - (Ad * gd).sum(1, keepdim=True))
    e = _scaled(dS, ref, Ad * (gd.abs() + (Ad * gd).abs().sum(1, keepdim=True)))
    print(f"\nMEASURE softmax_bwd/{rows}/{'dasum' if with_dasum else 'plain'} {e:.2e}")
    assert e < SOFTMAX_BOUND


# ------------------------------------------------------------------ D. the point-layer pieces
@pytest.mark.parametrize("B,N,C,ld", [(44, 4096, 1024, 1024), (5, 4093, 1000, 1012)])
def test_colmax_arg_and_bwd(cuda, B, N, C, ld):
    """colmax_arg / colmax_bwd on post-ReLU values in multiples of 1/4 (exact zeros, ties at the maximum, all-zero columns), at the
    T-Net / pointnet pool size and with N % 4 != 0, C % 64 != 0, ld > C: the maximum bit for bit, arg the first maximal row, and
    the backward's dense gradient exactly dOut at (arg, c), zero elsewhere."""
    ops = _ops()
    g = _gen(B * N + C, cuda)
    buf = torch.relu(torch.round(4 * torch.randn(B * N, ld, device=cuda, generator=g)) / 4)
    buf[:, C:] = 1e9                                    # beyond C: must not be read as a column
    zc = torch.randint(0, C, (B, 8), device=cuda, generator=g)
    buf.view(B, N, ld).scatter_(2, zc.unsqueeze(1).expand(B, N, 8), 0.0)      # eight all-zero columns per cloud
    x = buf[:, :C]
    out, arg = ops.colmax_arg(x, B, N)
    x3 = x.reshape(B, N, C)
    mx = x3.max(1).values
    assert torch.equal(out, mx)
    first = torch.empty(B, C, dtype=torch.int64, device=cuda)
    tn = torch.arange(N, device=cuda).view(1, N, 1)
    ties = 0
    for b0 in range(0, B, 4):
        eq = x3[b0:b0 + 4] == mx[b0:b0 + 4].unsqueeze(1)
        first[b0:b0 + 4] = torch.where(eq, tn, N).min(1).values
        ties += int((eq.sum(1) > 1).sum())
    assert torch.equal(arg.long(), first)
    assert bool((mx.gather(1, zc) == 0).all()) and bool((arg.gather(1, zc) == 0).all())
    print(f"\nMEASURE colmax/{B}x{N}x{C} {ties / (B * C):.2f} of the columns tie at the maximum")
    assert ties > B * C // 10
    dOut = torch.randn(B, C, device=cuda, generator=g)
    dIn = ops.colmax_bwd(dOut, arg, N)
    want = torch.zeros(B, N, C, device=cuda).scatter_(1, first.unsqueeze(1), dOut.unsqueeze(1)).view(B * N, C)
    assert torch.equal(dIn, want)


OUTER_BOUND = 2e-7       # / sum_n |x_i dy_j| per element


@pytest.mark.parametrize("N", [4096, 1000])
@pytest.mark.parametrize("KD", [3, 8])
def test_cloud_outer(cuda, KD, N):
    """cloud_outer (the T-Net transform's gradient, dT[b] = X_b^T dY_b) with strided X and dY against fp64 within OUTER_BOUND.
    Measured on the MI355X: 1.9e-8."""
    ops = _ops()
    B = 44
    g = _gen(KD * N, cuda)
    xb = torch.randn(B * N, KD + 9, device=cuda, generator=g) + 0.3
    yb = torch.randn(B * N, KD + 5, device=cuda, generator=g)
    X, dY = xb[:, 1:1 + KD], yb[:, 4:4 + KD]
    dT = ops.cloud_outer(X, dY, B, N)
    Xd, Yd = X.double().view(B, N, KD), dY.double().view(B, N, KD)
    ref = torch.einsum("bni,bnj->bij", Xd, Yd)
    e = _scaled(dT, ref, torch.einsum("bni,bnj->bij", Xd.abs(), Yd.abs()))
    print(f"\nMEASURE cloud_outer/KD={KD}/N={N} {e:.2e}")
    assert e < OUTER_BOUND


DW_BOUND = 2e-7          # / sum_m |dy_o x_c| per element


@pytest.mark.parametrize("rows", sorted(ls.DW_SMALLK_ROWS))
@pytest.mark.parametrize("Kin", [3, 8])
@pytest.mark.parametrize("Co", [64, 128, 256])
def test_dw_smallk(cuda, Co, Kin, rows):
    """dw_smallk (the weight gradient of a layer with Kin <= 8 inputs, autograd._dweight) with strided dY and X, at M = 180 224
    rows (the four-row unrolled loop divides every thread's rows: 704 blocks, stride 2816 at Co = 64) and at M = 175 001 (the tail
    loop runs), against fp64 within DW_BOUND.  Measured on the MI355X: 2.5e-8."""
    ops = _ops()
    M = ls.DW_SMALLK_ROWS[rows]
    assert ls.dw_smallk_launch(M, Co)[2] == (rows == "exact")
    g = _gen(Co * Kin + M, cuda)
    yb = torch.randn(M, Co + 4, device=cuda, generator=g)
    xb = torch.randn(M, 12, device=cuda, generator=g) + 0.2
    dY, X = yb[:, 4:], xb[:, 1:1 + Kin]
    dW = ops.dw_smallk(dY, X)
    ref = dY.double().t() @ X.double()
    e = _scaled(dW, ref, dY.double().abs().t() @ X.double().abs())
    print(f"\nMEASURE dw_smallk/Co={Co}/Kin={Kin}/M={M} {e:.2e}")
    assert e < DW_BOUND
