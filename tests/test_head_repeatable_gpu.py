"""The NetVLAD head gives the same bits for the same input in every launch: the per-cloud column sums of the soft assignment
(lpd_softmax_affine / lpd_softmax_affine_parts) and the a_sum / sums of squares of lpd_vlad_finalize are per-block partials added in
a fixed order, not float atomics.  Accuracy against fp64 is gated in tests/test_fwd_ops_gpu.py; here only repeatability, at sizes
with many blocks per cloud (the order of 16 .. 64 atomics per column used to vary)."""
import numpy as np
import pytest
import torch

from oracle import lpd_oracle as orc

pytestmark = pytest.mark.gpu

REPEATS = 4


@pytest.mark.parametrize("ncols", [64, 40])      # the 64-column kernel (one partial per 64 rows) / the generic one (one per 16 rows)
def test_softmax_column_sums_repeat_bit_for_bit(cuda, ncols):
    from lpdnet_hip import ops
    B, N = 5, 2048
    g = torch.Generator().manual_seed(ncols)
    a = (torch.randn(B * N, ncols, generator=g) * 3).to(cuda)
    sc, sh = torch.rand(ncols, generator=g).add(0.5).to(cuda), torch.randn(ncols, generator=g).to(cuda)
    out0, ws0 = ops.softmax_affine(a, sc, sh, colsum_rows=N)
    want = out0.double().view(B, N, ncols).sum(1)
    # N values in [0, 1] per column, fp32 running sums of at most N / 4 terms each: well inside N * 2^-24 relative to N
    assert (ws0[:, :ncols].double() - want).abs().max().item() <= N * 2.0 ** -24 and bool((ws0[:, ncols:] == 0).all())
    for _ in range(REPEATS):
        out, ws = ops.softmax_affine(a, sc, sh, colsum_rows=N)
        assert torch.equal(out, out0) and torch.equal(ws, ws0)


def test_softmax_of_summed_planes_repeats_bit_for_bit(cuda):
    from lpdnet_hip import ops
    B, N = 3, 1024
    g = torch.Generator().manual_seed(2)
    parts = torch.randn(4, B * N, 64, generator=g).to(cuda)
    sc, sh = torch.rand(64, generator=g).add(0.5).to(cuda), torch.randn(64, generator=g).to(cuda)
    out0, ws0 = ops.softmax_affine_parts(parts, sc, sh, colsum_rows=N)
    assert ws0.shape == (B, 128) and bool((ws0[:, 64:] == 0).all())
    assert (ws0[:, :64].double() - out0.double().view(B, N, 64).sum(1)).abs().max().item() <= N * 2.0 ** -24
    for _ in range(REPEATS):
        out, ws = ops.softmax_affine_parts(parts, sc, sh, colsum_rows=N)
        assert torch.equal(out, out0) and torch.equal(ws, ws0)


@pytest.mark.parametrize("N", [200, 2048])      # ceil(N / 64) a_sum blocks / 16 chunks
def test_vlad_finalize_repeats_bit_for_bit(cuda, N):
    from lpdnet_hip import ops
    B, F, KC = 5, 1024, 64
    g = torch.Generator().manual_seed(N)
    act = torch.softmax(torch.randn(B, N, KC, generator=g), dim=2).to(cuda)
    vraw, cw2 = torch.randn(B, F, KC, generator=g).to(cuda), torch.randn(F, KC, generator=g).to(cuda)
    aux0 = {}
    v0 = ops.vlad_finalize(vraw, act, cw2, aux=aux0)
    assert torch.isfinite(v0).all().item() and abs(v0[0].double().norm().item() - 1.0) < 1e-5
    for _ in range(REPEATS):
        aux = {}
        assert torch.equal(ops.vlad_finalize(vraw, act, cw2, aux=aux), v0)
        assert all(torch.equal(aux[n], aux0[n]) for n in ("asum", "inv_c", "inv_g"))
    if N % 16 == 0:      # with the a_sum of the softmax pass; one workspace serves any number of calls
        _, ws = ops.softmax_affine(torch.randn(B * N, KC, generator=g).to(cuda), colsum_rows=N)
        w0 = ops.vlad_finalize(vraw, act, cw2, ws=ws)
        for _ in range(REPEATS):
            assert torch.equal(ops.vlad_finalize(vraw, act, cw2, ws=ws), w0)


@pytest.mark.parametrize("featnet", ["pointnet", "lpdnet"])
def test_eval_forward_repeats_bit_for_bit(cuda, featnet):
    from util.PointNetVlad import PointNetVlad
    N, B = 1024, 4
    m = PointNetVlad(num_points=N, featnet=featnet)
    m.load_state_dict(orc.synthetic_state(featnet, num_points=N), strict=True)
    m = m.to(cuda).eval()
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (B, 1, N, 3)).astype(np.float32)).to(cuda)
    with torch.no_grad():
        d0 = m(x)
        for _ in range(REPEATS):
            assert torch.equal(m(x), d0)
