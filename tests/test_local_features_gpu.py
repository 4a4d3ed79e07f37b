"""lpd_local_features (csrc/lpd_feat.hip) and lpdnet_hip.features on the GPU, against the fp64 reference of tests/local_features_ref.py.

The reference is given the GPU's OWN neighbour lists (the project's flip-free idiom), so kNN near-ties never enter a comparison.
Gates (local_features_ref.GATE_*): C, O, L, A, L2 2e-5 absolute; S2, dZ, sZ 1e-6 absolute; D 1e-5 relative; V 1e-4 absolute where the
fp64 eigengap (l2 - l3) / l1 > 1e-2, with at most 10 % of the points excluded.  They are 15-20x the floor of a plain fp32 restatement
(centred moments in rank order, six Jacobi sweeps) and reject raw-coordinate moments (>= 5e-2) and bf16 anywhere (>= 1e-3).
Every case prints `MEASURE local_features/<case> <column> err=... gate=...`.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import local_features_ref as R
import walk_forms
from oracle import lpd_oracle as orc

pytestmark = pytest.mark.gpu

CANDIDATES = (8, 12, 16, 20, 24, 28, 32)
_CACHE = {}


def _clouds(B, N, seed, kinds=R.KINDS):
    key = (B, N, seed, kinds)
    if key not in _CACHE:
        _CACHE[key] = R.clouds(B, N, seed, kinds)
    return _CACHE[key]


def _run(cuda, x_np, K=None, idx=None, **kw):
    """ops.knn_pm (unless lists are given) + ops.local_features -> (result numpy [B,N,W], idx numpy [B,N,K], extra)"""
    from lpdnet_hip import ops
    x = torch.from_numpy(x_np).to(cuda)
    B, N = x.shape[:2]
    rows = x.view(B * N, 3)
    idx_t = ops.knn_pm(rows, B, N, K) if idx is None else torch.from_numpy(np.ascontiguousarray(idx)).to(cuda)
    res = ops.local_features(rows, idx_t, B, N, **kw)
    torch.cuda.synchronize()
    out, kopt = res if isinstance(res, tuple) else (res, None)
    return out.cpu().numpy().reshape(B, N, -1), idx_t.cpu().numpy(), (kopt.cpu().numpy().reshape(B, N) if kopt is not None else None)


def _l2_form(monkeypatch):
    """the next launches take the L2 form whatever N (the C side reads LPD_DEBUG on every call of this entry point)"""
    monkeypatch.setenv("LPD_DEBUG", "feat-l2")


# ---- 1. fixed neighbourhood size, the LDS form --------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 20, 32])
def test_fixed_size_all_columns(cuda, k):
    x = _clouds(3, 1024, 1)
    got, idx, _ = _run(cuda, x, K=k)
    ref, gap = R.features(x, idx)
    assert got.shape == (3, 1024, 10)
    assert not R.check_columns(got, ref, gap, f"fixed/B3/N1024/k{k}")


# ---- 2. adaptive size ------------------------------------------------------------------------------------------------------------
def test_adaptive_size(cuda):
    x = _clouds(3, 1024, 2, ("mixed", "wire", "cube"))
    got, idx, kopt = _run(cuda, x, K=32, candidates=CANDIDATES, want_k=True)
    assert np.isin(kopt, CANDIDATES).all()
    ref, gap = R.features(x, idx, kopt=kopt)
    assert not R.check_columns(got, ref, gap, "adaptive/B3/N1024/K32")
    E = R.entropies(x, idx, CANDIDATES)
    at = np.take_along_axis(E, np.searchsorted(CANDIDATES, kopt)[..., None], axis=-1)[..., 0]
    excess = float((at - E.min(axis=-1)).max())
    differ = float((np.asarray(CANDIDATES)[E.argmin(axis=-1)] != kopt).mean())
    print(f"MEASURE local_features/adaptive/B3/N1024/K32 entropy_excess err={excess:.3e} gate={2 * R.GATE_RATIO:.0e}")
    print(f"MEASURE local_features/adaptive/B3/N1024/K32 kopt_differs frac={differ:.4f} cap=0.01")
    assert excess <= 2 * R.GATE_RATIO
    assert differ <= 0.01
    # fixed size = one candidate
    one, _, k1 = _run(cuda, x, idx=idx, candidates=(32,), want_k=True)
    fixed, _, _ = _run(cuda, x, idx=idx)
    assert (k1 == 32).all() and np.array_equal(one, fixed)


# ---- 3. launch edges: both forms of the neighbour read ------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", [(2, 100, 7), (1, 4096, 64), (2, 4128, 20), (2, 8192, 20)])
def test_launch_edges(cuda, monkeypatch, B, N, K):
    x = _clouds(B, N, 3, ("cube", "slab") if B > 1 else ("slab",))
    got, idx, _ = _run(cuda, x, K=K)
    ref, gap = R.features(x, idx)
    assert not R.check_columns(got, ref, gap, f"edges/B{B}/N{N}/K{K}")
    if N <= 4096:      # a cloud both forms accept: same bits
        _l2_form(monkeypatch)
        l2, _, _ = _run(cuda, x, idx=idx)
        assert np.array_equal(got.view(np.int32), l2.view(np.int32))


def test_both_forms_agree_on_a_second_cloud_kind(cuda, monkeypatch):
    x = _clouds(2, 4096, 4, ("cube", "mixed"))
    lds, idx, k_lds = _run(cuda, x, K=32, candidates=CANDIDATES, want_k=True)
    _l2_form(monkeypatch)
    l2, _, k_l2 = _run(cuda, x, idx=idx, candidates=CANDIDATES, want_k=True)
    assert np.array_equal(lds.view(np.int32), l2.view(np.int32)) and np.array_equal(k_lds, k_l2)


# (B, N, K, candidates).  B = 2, N = 67 with ldx = 3: the second cloud starts 804 bytes in, so one launch stages cloud 0 in 16-byte
# pieces and cloud 1 by the float; 3 N is no multiple of 4 (the scalar tail) and the last tile is mostly idle lanes.  K = 7: 4-byte
# list loads and a last group of three; K = 8 and 12: int4 pieces.  N = 513 (LDS form) and N = 257 (L2 form): a second tile with one
# live lane.
WALK_CASES = [(2, 67, 7, None), (2, 67, 8, None), (2, 67, 12, (4, 8, 12)), (1, 513, 8, None), (1, 257, 8, None)]


@pytest.mark.parametrize("B,N,K,cand", WALK_CASES)
def test_every_read_path_gives_the_same_bits(cuda, monkeypatch, B, N, K, cand):
    """The plain input is held to the fp64 reference; every other layout of the same input (walk_forms), and all of them again in
    the L2 form, give its bits in all ten columns and kopt."""
    from lpdnet_hip import ops
    x = _clouds(B, N, 9, ("slab", "cube"))
    idx = R.knn_lists(x, K)
    rows, idx_t = torch.from_numpy(x).to(cuda).view(B * N, 3), torch.from_numpy(idx).to(cuda)

    def run(r, i):
        out, kopt = ops.local_features(r, i, B, N, candidates=cand, want_k=True)
        torch.cuda.synchronize()
        return out.cpu().numpy(), kopt.cpu().numpy()
    base, kbase = run(rows, idx_t)
    assert np.isin(kbase, cand if cand else (K,)).all()
    ref, gap = R.features(x, idx, kopt=kbase.reshape(B, N))
    assert not R.check_columns(base.reshape(B, N, 10), ref, gap, f"walk/B{B}/N{N}/K{K}" + ("/adaptive" if cand else ""))
    variants = walk_forms.forms(rows, idx_t)
    for l2 in (False, True):
        if l2:
            _l2_form(monkeypatch)
        for name, r, i in variants + ([("plain", rows, idx_t)] if l2 else []):
            got, kgot = run(r, i)
            assert np.array_equal(got.view(np.int32), base.view(np.int32)) and np.array_equal(kgot, kbase), (name, "L2" if l2 else "LDS")


# ---- 4. translated clouds: the moments must be centred on the query point -------------------------------------------------------
def test_translated_clouds(cuda):
    x = (_clouds(4, 1024, 1).astype(np.float64) + np.array([100.0, -50.0, 20.0])).astype(np.float32)
    idx = R.knn_lists(x, 20)      # fp64 argsort on the CPU: the product kNN is not under test here
    got, _, _ = _run(cuda, x, idx=idx)
    ref, gap = R.features(x, idx)
    assert not R.check_columns(got, ref, gap, "translated/B4/N1024/k20")


# ---- 5. degenerate neighbourhoods -------------------------------------------------------------------------------------------------
def test_degenerate_inputs(cuda):
    same = np.full((1, 64, 3), 0.37, dtype=np.float32)
    got, _, _ = _run(cuda, same, idx=R.knn_lists(same, 8))
    assert (got == 0).all()
    t = np.arange(64, dtype=np.float32) / 64
    line = np.stack((t, 2 * t, -t), axis=1)[None].astype(np.float32)
    got, _, _ = _run(cuda, line, idx=R.knn_lists(line, 8))
    assert np.isfinite(got).all()
    for c, want in ((0, 0.0), (2, 1.0), (3, 0.0)):
        err = float(np.abs(got[..., c] - want).max())
        print(f"MEASURE local_features/line/N64/K8 {R.COLUMNS[c]} err={err:.3e} gate={R.GATE_RATIO:.0e}")
        assert err <= R.GATE_RATIO
    gx, gy = np.meshgrid(np.arange(8), np.arange(8))
    lattice = np.stack((gx.ravel() * 0.125, gy.ravel() * 0.125, 0.0 * gx.ravel()), axis=1)[None].astype(np.float32)
    got, _, _ = _run(cuda, lattice, idx=R.knn_lists(lattice, 8))
    assert np.isfinite(got).all()
    assert (got[..., 0] == 0).all() and (got[..., 7] == 0).all() and (got[..., 8] == 0).all()
    err = float(np.abs(got[..., 4] - 1.0).max())
    print(f"MEASURE local_features/lattice/N64/K8 V err={err:.3e} gate={R.GATE_V:.0e}")
    assert err <= R.GATE_V


# ---- 6. output addressing ------------------------------------------------------------------------------------------------------------
def test_output_addressing(cuda):
    from lpdnet_hip import ops
    x = _clouds(3, 1024, 1)
    full, idx, _ = _run(cuda, x, K=20)
    rows8, _, _ = _run(cuda, x, idx=idx, columns=(0, 1, 2, 3, 4), copy_xyz=True)
    assert rows8.shape[-1] == 8
    assert np.array_equal(rows8.view(np.int32), np.concatenate((x, full[..., :5]), axis=-1).view(np.int32))
    gaps, _, _ = _run(cuda, x, idx=idx, columns=(1, 4, 9))
    assert np.array_equal(gaps.view(np.int32), full[..., [1, 4, 9]].view(np.int32))
    # ldo larger than the row: the padding is left untouched
    xt = torch.from_numpy(x).to(cuda).view(-1, 3)
    buf = torch.full((xt.shape[0], 12), -7.5, device=cuda)
    out = ops.local_features(xt, torch.from_numpy(idx).to(cuda), 3, 1024, columns=(1, 4, 9), copy_xyz=True, out=buf)
    assert out is buf
    b = buf.cpu().numpy().reshape(3, 1024, 12)
    assert np.array_equal(b[..., :3], x) and np.array_equal(b[..., 3:6].view(np.int32), gaps.view(np.int32)) and (b[..., 6:] == -7.5).all()


# ---- 7. argument errors: an error code and a message, nothing launched ------------------------------------------------------------------
def test_argument_errors(cuda):
    from lpdnet_hip import LpdHipError, _lib, ops
    N = 64
    xt = torch.from_numpy(_clouds(1, N, 5)).to(cuda).view(-1, 3)
    lib = _lib.load()
    out = torch.full((N, 16), -7.5, device=cuda)

    def call(K, cand=None, sel=0x3ff, copy_xyz=0, ldo=16, n=N):
        idx = torch.zeros((1, n, max(K, 1)), dtype=torch.int32, device=cuda)
        arr = (ctypes.c_int32 * max(1, len(cand or ())))(*(cand or ()))
        rc = lib.lpd_local_features(xt.data_ptr(), 3, idx.data_ptr(), 1, n, K, arr if cand else None, len(cand or ()), sel, copy_xyz,
                                    out.data_ptr(), ldo, None, None)
        return rc, lib.lpd_last_error().decode()

    assert call(20)[0] == 0                       # the valid call these are variations of
    out.fill_(-7.5)
    bad = [call(3), call(65), call(40, n=32),     # K = 3, K = 65, K > N
           call(20, cand=(12, 8)), call(20, cand=(8, 8)), call(20, cand=(3, 8)), call(20, cand=(8, 24)),      # unsorted / out of range
           call(64, cand=tuple(range(4, 21))),    # 17 candidates
           call(20, sel=0), call(20, sel=1 << 10), call(20, ldo=9), call(20, sel=0x1f, copy_xyz=1, ldo=7)]
    for rc, msg in bad:
        assert rc == -1 and msg.startswith("lpd_local_features:"), (rc, msg)
    torch.cuda.synchronize()
    assert (out == -7.5).all()                    # no launch wrote anything
    idx = torch.zeros((1, N, 20), dtype=torch.int32, device=cuda)
    with pytest.raises(LpdHipError, match="candidate"):
        ops.local_features(xt, idx, 1, N, candidates=(12, 8))
    with pytest.raises(LpdHipError):
        ops.local_features(xt, idx, 1, N, out=torch.empty((N, 4), device=cuda))      # ldo too small
    with pytest.raises(LpdHipError):
        ops.local_features(xt.cpu(), idx, 1, N)


# ---- 8. the caller's stream ------------------------------------------------------------------------------------------------------------
def test_runs_on_the_current_stream(cuda):
    from lpdnet_hip import ops
    x = torch.from_numpy(_clouds(3, 1024, 1)).to(cuda).view(-1, 3)
    idx = ops.knn_pm(x, 3, 1024, 20)
    want = ops.local_features(x, idx, 3, 1024)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    gate = torch.cuda.Event()
    with torch.cuda.stream(s):
        got = ops.local_features(x, idx, 3, 1024)
        gate.record(s)
    assert s.cuda_stream != torch.cuda.default_stream(cuda).cuda_stream
    gate.synchronize()            # only stream s is waited for: the result is there when ITS work is done
    assert torch.equal(got, want)
    torch.cuda.synchronize()


# ---- 9.-12. the public surface -----------------------------------------------------------------------------------------------------------
N_PUB, B_PUB = 1024, 4


def _x3(cuda, n=B_PUB, seed=6):
    return torch.from_numpy(_clouds(n, N_PUB, seed)).unsqueeze(1).to(cuda)      # [n,1,N,3]


def _model(cuda, featnet="lpdnet", use_mfea=False):
    from lpdnet_hip import features
    from util.PointNetVlad import PointNetVlad
    m = PointNetVlad(num_points=N_PUB, featnet=featnet)
    if use_mfea:
        features.convert_to_local_features(m)
    m.load_state_dict(orc.synthetic_state(featnet, num_points=N_PUB, use_mFea=use_mfea), strict=True)
    return m.to(cuda)


def _desc_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().amax(dim=1) / b.abs().amax(dim=1)).max().item()


def test_features_equal_the_two_step_form(cuda):
    from lpdnet_hip import features, ops
    x = _x3(cuda)
    rows = x.view(-1, 3)
    for kw in (dict(k=20), dict(candidates=CANDIDATES)):
        got = features.local_features(x, **kw)
        K = max(kw["candidates"]) if "candidates" in kw else 20
        two = ops.local_features(rows, ops.knn_pm(rows, B_PUB, N_PUB, K), B_PUB, N_PUB, candidates=kw.get("candidates"))
        assert got.shape == (B_PUB, N_PUB, 10) and torch.equal(got.reshape(-1, 10), two)
        assert torch.equal(features.local_features(x[:, 0], **kw), got)      # [B,N,3] input
    # a shuffled cloud gives the shuffled features (the lists of the shuffled cloud are those of the cloud, renamed)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(N_PUB)).to(cuda)
    base = features.local_features(x, k=20).cpu().numpy()
    shuf = features.local_features(x[:, :, perm], k=20).cpu().numpy()
    xs = x[:, 0, perm].cpu().numpy()
    idx = ops.knn_pm(x[:, 0, perm].reshape(-1, 3).contiguous(), B_PUB, N_PUB, 20).cpu().numpy()
    ref, gap = R.features(xs, idx)
    assert not R.check_columns(shuf, ref, gap, "shuffled/B4/N1024/k20")
    # ... and against the unshuffled result itself wherever the shuffle did not flip a kNN near-tie (V: where it is well defined)
    d = np.abs(shuf - base[:, perm.cpu().numpy()])
    assert np.median(d[..., [0, 1, 2, 3, 6]]) <= R.GATE_RATIO
    five = features.append_local_features(x)
    assert five.shape == (B_PUB, 1, N_PUB, 8) and torch.equal(five[..., :3], x)
    assert torch.equal(five[0, 0, :, 3:], features.local_features(x, k=20, columns=features.DEFAULT_COLUMNS)[0])


@pytest.mark.parametrize("featnet", ["lpdnet", "lpdnetorigin"])
def test_converted_model_gives_the_xyz_model_s_descriptors(cuda, featnet):
    from lpdnet_hip import features, harness
    plain = _model(cuda, featnet)
    wrapped = features.LocalFeatureInput(features.convert_to_local_features(copy.deepcopy(plain)))
    assert wrapped.module.emb_nn.use_mFea and not plain.emb_nn.use_mFea
    x = _x3(cuda)
    for train in (False, True):
        plain.train(train)
        wrapped.train(train)
        want, got = plain(x), wrapped(x)
        rel = _desc_rel(got, want)
        print(f"MEASURE local_features/converted/{featnet}/{'train' if train else 'eval'} err={rel:.3e} gate=1e-04")
        assert got.shape == (B_PUB, 256) and rel < 1e-4
    # one optimisation step through the wrapper: the five new columns of conv1 receive a gradient
    opt = torch.optim.SGD(wrapped.parameters(), lr=1e-5)
    c = _x3(cuda, 6, seed=7)[:, 0]      # [6,N,3]: query, 2 positives, 2 negatives, other negative
    loss = harness.train_step(wrapped, opt, c[None, 0:1], c[None, 1:3], c[None, 3:5], c[None, 5:6])
    w = dict(wrapped.module.emb_nn.named_parameters())[features._conv1_key(wrapped.module.emb_nn)]
    g = w.grad[:, 3:]
    assert torch.isfinite(loss).item() and w.shape[1] == 8
    assert torch.isfinite(g).all().item() and g.abs().max().item() > 0


# Descriptors of one input from two DIFFERENT launch sequences (whole batch / slices, one batch / per-batch calls) are compared at the
# figure tests/test_model_gpu.py::test_module_api_surface uses for that; what the wrapper itself decides -- the tensor it hands to
# the wrapped model -- and the descriptors of that same tensor are compared bit for bit (the NetVLAD head adds its column sums and
# sums of squares in a fixed order: two forwards of one input give the same bits).
LAUNCH_SEQ_TOL = 1e-6


def _wrapper_and_input(cuda):
    from lpdnet_hip import features
    model = _model(cuda, "lpdnet", use_mfea=True).eval()
    return features.LocalFeatureInput(model).eval(), _x3(cuda)


def test_wrapper_with_feature_weights_matches_the_oracle(cuda):
    from lpdnet_hip import features
    wrapper, x = _wrapper_and_input(cuda)
    seen = []
    hook = wrapper.module.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
    with torch.no_grad():
        got = wrapper(x)
        hook.remove()
        x8 = features.append_local_features(x, zorder=True)
        assert len(seen) == 1 and torch.equal(seen[0], x8)      # the wrapped model is fed exactly append_local_features(x, zorder=True)
        direct = wrapper.module(x8)
    rel = _desc_rel(got, direct)
    print(f"MEASURE local_features/wrapper_vs_module/lpdnet/eval err={rel:.3e} gate={LAUNCH_SEQ_TOL:.0e}")
    assert rel < LAUNCH_SEQ_TOL
    sd = orc.synthetic_state("lpdnet", num_points=N_PUB, use_mFea=True)
    ref = orc.pointnetvlad_forward(sd, x8.cpu(), featnet="lpdnet", train=False)
    rel = _desc_rel(got, ref)
    print(f"MEASURE local_features/wrapper_vs_oracle/lpdnet/eval err={rel:.3e} gate=1e-04")
    assert rel < 1e-4
    # the feature columns matter in this model: the xyz-only input padded with zeros gives other descriptors
    with torch.no_grad():
        zero = wrapper.module(torch.cat((x8[..., :3], torch.zeros_like(x8[..., 3:])), dim=-1))
    assert _desc_rel(zero, got) > 1e-3


def test_wrapper_descriptors_equal_the_module_s_bit_for_bit(cuda):
    """wrapper(x3) equals wrapper.module(append_local_features(x3, zorder=True)) bit for bit: the wrapped model is fed the identical
    tensor, and an eval forward is a fixed sequence of fixed-order sums (no float atomics on the way)."""
    from lpdnet_hip import features
    wrapper, x = _wrapper_and_input(cuda)
    with torch.no_grad():
        got = wrapper(x)
        direct = wrapper.module(features.append_local_features(x, zorder=True))
    print(f"MEASURE local_features/wrapper_vs_module_bitwise/lpdnet/eval err={_desc_rel(got, direct):.3e} gate=0")
    assert torch.equal(got, direct)


def test_get_latent_vectors_through_the_wrapper(cuda):
    from lpdnet_hip import features, harness
    wrapper = features.LocalFeatureInput(_model(cuda, "lpdnet", use_mfea=True))
    clouds = _clouds(7, N_PUB, 8)
    for train in (True, False):
        wrapper.train(train)
        got = harness.get_latent_vectors(wrapper, clouds, 3)      # 3 + 3 + ragged 1
        assert wrapper.training is train and wrapper.module.training is train and wrapper.module.emb_nn.training is train
    wrapper.eval()
    with torch.no_grad():
        want = torch.cat([wrapper(torch.from_numpy(clouds[s:s + 3]).unsqueeze(1).to(cuda)) for s in (0, 3, 6)], dim=0)
    rel = _desc_rel(torch.from_numpy(got), want)
    print(f"MEASURE local_features/get_latent_vectors/n7/batch3 err={rel:.3e} gate={LAUNCH_SEQ_TOL:.0e}")
    assert got.shape == (7, 256) and got.dtype == np.float32 and rel < LAUNCH_SEQ_TOL


def test_sliced_eval_batches_through_the_wrapper(cuda, monkeypatch):
    """PointNetVlad.forward runs large eval batches as slices, two in flight (engine.EVAL_CHUNK x 4096 points each): the 8-column
    input of a use_mFea trunk is sliced like the 3-column one."""
    from lpdnet_hip import engine, features
    wrapper = features.LocalFeatureInput(_model(cuda, "lpdnet", use_mfea=True)).eval()
    x = _x3(cuda, 7, seed=8)
    with torch.no_grad():
        whole = wrapper(x)
        monkeypatch.setattr(engine, "EVAL_CHUNK", 1)      # 4096 points per slice: 4 + 3 clouds
        sliced = wrapper(x)
    rel = _desc_rel(sliced, whole)
    print(f"MEASURE local_features/sliced_eval/n7 err={rel:.3e} gate={LAUNCH_SEQ_TOL:.0e}")
    assert sliced.shape == (7, 256) and rel < LAUNCH_SEQ_TOL
