"""lpd_sample_items / lpd_gather_tuples and lpdnet_hip.tuples.TupleBank on the GPU against tests/tuples_ref.py.

Sampling is integer arithmetic: `out` and `count` equal the numpy restatement exactly.  Gathering without augmentation is a
bit-copy.  Gates of the augmentations (derived, not tuned):
  rotation   |err| <= 3 * 2^-24 * (|x||c| + |y||s|): two products and a sum, fused or not; z bit-equal
  jitter     every |delta| <= clip exactly; the normals behind it within 1e-4 of the float64 restatement on the same uniforms (a
             wrong formula errs by O(1); the fp32 rounding of 2 pi u alone is about 2e-6); output within
             2^-23 * max(1, |ref|) + sigma * 1e-4
Measured on an MI355X (MEASURE lines of this file): see DESIGN.md section 13d."""
import ctypes

import numpy as np
import pytest
import torch

import tuples_ref as R

pytestmark = pytest.mark.gpu
Z_CAP = 1e-4


# ---- lpd_sample_items ------------------------------------------------------------------------------------------------------------
def _problem(T, R_rows, L, X, seed):
    """a CSR of 41 lists over T items (empty ones, duplicates, overlaps, items outside [0, T); list 40 = all of [0, T)) and the rows'
    list numbers / extras, some outside their ranges.  Row 0 names nothing; row 1 names the full list (when L > 0)."""
    g = np.random.default_rng(seed)
    lists = []
    for l in range(40):
        n = int(g.integers(0, max(2, min(T, 600)))) if l % 7 else 0
        it = g.integers(0, T, size=n)
        if n > 4:
            it[:2] = it[2:4]                      # duplicates
            it[4 % n] = T + int(g.integers(0, 5))      # outside, above
            it[-1] = -1 - int(g.integers(0, 5))        # outside, below
        lists.append(it)
    lists.append(g.permutation(T))
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate(lists).astype(np.int32)
    rows = g.integers(-1, 43, size=(R_rows, L)).astype(np.int32)      # -1 unused, 41 / 42 outside
    rows[rows == 40] = 39                                            # the full list only where it is put on purpose
    extra = g.integers(-2, T + 2, size=(R_rows, X)).astype(np.int32)
    rows[0, :] = -1
    extra[0, :] = -1
    if L > 0 and R_rows > 1:
        rows[1, 0] = 40
    return off, idx, rows, extra


SAMPLE_CASES = [  # T, R, m, L, X
    (37, 5, 18, 1, 0), (64, 5, 1, 19, 3), (4097, 5, 4000, 19, 3), (70001, 5, 4000, 1, 3), (70001, 3, 18, 0, 0), (70001, 3, 18, 0, 3),
    (262144, 2, 4000, 19, 3)]


def _run_sample(cuda, off, idx, T, rows, extra, m, invert, seed):
    from lpdnet_hip import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)      # noqa: E731
    out, cnt = ops.sample_items(d(off), d(idx), T, d(rows), d(extra) if extra.shape[1] else None, m, invert, seed)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("T,R_rows,m,L,X", SAMPLE_CASES)
def test_sample_items_equals_the_restatement(cuda, T, R_rows, m, L, X, invert):
    off, idx, rows, extra = _problem(T, R_rows, L, X, seed=T + 7 * L + X)
    seed = 0x0123456789ABCDEF ^ (T << 20)
    want, wcnt = R.sample_items(off, idx, T, rows, extra, m, invert, seed)
    got, cnt = _run_sample(cuda, off, idx, T, rows, extra, m, invert, seed)
    assert np.array_equal(cnt, wcnt), (cnt, wcnt)
    assert np.array_equal(got, want)
    # what the cases are for: an empty pool, a pool smaller than m, distinct in-range items
    assert (wcnt[0] == 0) if invert == 0 else (wcnt[0] == T)
    if L > 0:
        assert wcnt[1] == (T if invert == 0 else 0)
    for r in range(R_rows):
        k = min(m, int(cnt[r]))
        assert len(set(got[r, :k].tolist())) == k and (got[r, :k] >= 0).all() and (got[r, :k] < T).all() and (got[r, k:] == -1).all()
    if m > 1 and (L > 0 or invert == 0):
        assert (wcnt < m).any()      # m > count occurs


def test_sample_items_repeatable_and_seeded(cuda):
    T, m = 4097, 18
    off, idx, rows, extra = _problem(T, 5, 19, 3, seed=1)
    a = _run_sample(cuda, off, idx, T, rows, extra, m, 1, 5)
    b = _run_sample(cuda, off, idx, T, rows, extra, m, 1, 5)
    c = _run_sample(cuda, off, idx, T, rows, extra, m, 1, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[1], c[1]) and not np.array_equal(a[0], c[0])
    big = (a[1] >= m) & (a[1] > 100)
    assert big.any() and all(not np.array_equal(a[0][r], c[0][r]) for r in np.nonzero(big)[0])


def test_argument_errors_launch_nothing(cuda):
    from lpdnet_hip import LpdHipError, _lib, ops
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    off = torch.tensor([0, 2], dtype=torch.int32, device=cuda)
    idx = torch.tensor([1, 3], dtype=torch.int32, device=cuda)
    rows = torch.zeros((1, 1), dtype=torch.int32, device=cuda)
    out = torch.full((1, 4), 7, dtype=torch.int32, device=cuda)
    cnt = torch.full((1,), 7, dtype=torch.int32, device=cuda)
    names = ["off", "idx", "n_lists", "nnz", "T", "lists", "L", "extra", "X", "R", "invert", "m", "seed", "out", "count", "stream"]
    good = [p(off), p(idx), 1, 2, 10, p(rows), 1, None, 0, 1, 0, 4, 0, p(out), p(cnt), None]
    for kw in (dict(off=None), dict(out=None), dict(count=None), dict(idx=None), dict(T=0), dict(T=262145), dict(m=0), dict(m=4097), dict(L=65),
               dict(L=-1), dict(lists=None), dict(X=65), dict(X=1), dict(R=0), dict(R=65536), dict(invert=2), dict(n_lists=-1)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        rc, msg = lib.lpd_sample_items(*a), lib.lpd_last_error().decode()
        assert rc == -1 and msg.startswith("lpd_sample_items:"), (kw, rc, msg)
    table = torch.ones((4, 8, 3), device=cuda)
    items = torch.zeros((2,), dtype=torch.int32, device=cuda)
    gout = torch.full((2, 8, 3), 7.0, device=cuda)
    gnames = ["table", "T", "N", "items", "B", "rot", "sigma", "clip", "seed", "out", "stream"]
    ggood = [p(table), 4, 8, p(items), 2, None, 0.0, 0.05, 0, p(gout), None]
    for kw in (dict(table=None), dict(items=None), dict(out=None), dict(T=0), dict(N=0), dict(N=(1 << 20) + 1), dict(B=0), dict(B=65536),
               dict(sigma=-1.0), dict(clip=0.0), dict(out=p(table))):
        a = list(ggood)
        for k, v in kw.items():
            a[gnames.index(k)] = v
        rc, msg = lib.lpd_gather_tuples(*a), lib.lpd_last_error().decode()
        assert rc == -1 and msg.startswith("lpd_gather_tuples:"), (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out == 7).all() and (cnt == 7).all() and (gout == 7).all()      # nothing was launched
    for bad in (lambda: ops.sample_items(off, idx, 10, rows, None, 0, 0, 0), lambda: ops.sample_items(off, idx, 0, rows, None, 1, 0, 0),
                lambda: ops.sample_items(off, idx, 10, rows.view(-1), None, 1, 0, 0), lambda: ops.sample_items(off, idx, 10, rows, rows.expand(2, 1), 1, 0, 0),
                lambda: ops.sample_items(off, idx, 10, rows, None, 1, 2, 0), lambda: ops.gather_tuples(table[:, :, :2], items),
                lambda: ops.gather_tuples(table, items, rot=torch.zeros((3, 2), device=cuda)), lambda: ops.gather_tuples(table, items, sigma=-1.0),
                lambda: ops.gather_tuples(table, items, out=torch.zeros((2, 8, 2), device=cuda))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.sample_items(off.long(), idx, 10, rows, None, 1, 0, 0)
    with pytest.raises(TypeError):
        ops.gather_tuples(table, items.long())
    with pytest.raises(LpdHipError):
        ops.gather_tuples(table.cpu(), items)


# ---- lpd_gather_tuples -----------------------------------------------------------------------------------------------------------
_TABLES = {}


def _table(cuda, T, N):
    if (T, N) not in _TABLES:
        t = np.random.default_rng(T * 10007 + N).uniform(-1, 1, size=(T, N, 3)).astype(np.float32)
        t[0, 0, :] = [-0.0, 0.0, 1e-40]      # a negative zero and a denormal survive a bit-copy
        _TABLES[(T, N)] = (t, torch.from_numpy(t).to(cuda))
    return _TABLES[(T, N)]


def _gather(cuda, tab, items, **kw):
    from lpdnet_hip import ops
    if kw.get("rot") is not None:
        kw["rot"] = torch.from_numpy(np.asarray(kw["rot"], dtype=np.float32)).to(cuda)
    out = ops.gather_tuples(tab, torch.tensor(items, dtype=torch.int32, device=cuda), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("B,N", [(44, 4096), (3, 130), (5, 1)])
def test_gather_without_augmentation_is_a_bit_copy(cuda, B, N):
    T = 50
    host, tab = _table(cuda, T, N)
    items = [int(v) for v in np.random.default_rng(B).integers(0, T, size=B)]
    items[0] = 0
    items[1] = items[0]              # a repeated item
    items[2] = -1 if B == 3 else T      # outside: zeros
    if B > 4:
        items[4] = -1
    got = _gather(cuda, tab, items)
    want = np.zeros((B, N, 3), dtype=np.float32)
    for b, it in enumerate(items):
        if 0 <= it < T:
            want[b] = host[it]
    assert got.shape == (B, N, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[2] == 0).all() and np.array_equal(got[0], got[1])


def _angles(B, seed=3):
    a = np.random.default_rng(seed).uniform(-np.pi / 2, np.pi / 2, size=B)
    a[0] = 0.0
    return np.stack((np.cos(a), np.sin(a)), 1).astype(np.float32)


@pytest.mark.parametrize("B,N", [(6, 4096), (3, 130)])
def test_rotation_against_float64(cuda, B, N):
    T = 50
    host, tab = _table(cuda, T, N)
    items = list(range(B - 1)) + [T]
    rot = _angles(B)
    got = _gather(cuda, tab, items, rot=rot)
    ref = R.gather_tuples(host, items, rot=rot)
    src = R.gather_tuples(host, items)
    c, s = np.abs(rot[:, 0].astype(np.float64))[:, None], np.abs(rot[:, 1].astype(np.float64))[:, None]
    bx = 3 * 2.0 ** -24 * (np.abs(src[..., 0]) * c + np.abs(src[..., 1]) * s)
    by = 3 * 2.0 ** -24 * (np.abs(src[..., 0]) * s + np.abs(src[..., 1]) * c)
    ex, ey = np.abs(got[..., 0] - ref[..., 0]), np.abs(got[..., 1] - ref[..., 1])
    print(f"MEASURE gather_tuples/rotation/N{N} worst err/bound x {np.max(ex / np.maximum(bx, 1e-300)):.3f} y {np.max(ey / np.maximum(by, 1e-300)):.3f}")
    assert (ex <= bx).all() and (ey <= by).all()
    assert np.array_equal(got[..., 2].view(np.uint32), src[..., 2].astype(np.float32).view(np.uint32))      # z untouched
    assert np.array_equal(got[0], host[0]) and (got[B - 1] == 0).all()      # angle 0: the cloud itself; outside: zeros


def test_jitter_saturated(cuda):
    """sigma = clip: about 32 % of the coordinates sit on the clamp.  On a table of zeros out IS delta."""
    N, B, seed = 4096, 4, 77
    zeros = torch.zeros((2, N, 3), device=cuda)
    clip = np.float32(0.05)
    got = _gather(cuda, zeros, [0, 1, 0, 1], sigma=0.05, clip=0.05, seed=seed)
    assert np.abs(got).max() <= clip      # exact, in fp32
    z = R.normals(N, range(B), seed)
    raw = float(clip) * z                 # sigma = clip
    keep = np.abs(np.abs(raw) - float(clip)) > 1e-6      # away from the clamp's edge, the two sides agree on which side they are
    share_ref = (np.abs(raw[keep]) > float(clip)).mean()
    share = (np.abs(got[keep]) == clip).mean()
    print(f"MEASURE gather_tuples/jitter/saturated share {share:.4f} restatement {share_ref:.4f}")
    assert abs(share - share_ref) <= 0.02 and 0.28 < share_ref < 0.36
    assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[1], got[3])      # one item in two slots: different noise


@pytest.mark.parametrize("N", [4096, 130])
def test_jitter_default_against_the_restatement(cuda, N):
    B, seed, sigma, clip = 3, 20261018, 0.005, 0.05
    s32 = float(np.float32(sigma))
    zeros = torch.zeros((1, N, 3), device=cuda)
    d = _gather(cuda, zeros, [0] * B, sigma=sigma, clip=clip, seed=seed)      # p = 0: out is delta, no cancellation
    z64 = R.normals(N, range(B), seed)
    inside = np.abs(s32 * z64) < float(np.float32(clip)) - 1e-6
    z32 = d.astype(np.float64) / s32
    zerr = np.abs(z32 - z64)[inside].max()
    print(f"MEASURE gather_tuples/jitter/N{N} max|z32 - z64| {zerr:.3e} cap {Z_CAP:.0e}")
    assert inside.mean() > 0.99 and zerr < Z_CAP
    T = 50
    host, tab = _table(cuda, T, N)
    items = [5, 5, 49]
    got = _gather(cuda, tab, items, sigma=sigma, clip=clip, seed=seed)
    ref = R.gather_tuples(host, items, sigma=sigma, clip=clip, seed=seed)
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + s32 * Z_CAP
    err = np.abs(got - ref)
    print(f"MEASURE gather_tuples/jitter/N{N} output worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert not np.array_equal(got[0], got[1])      # the same item in two slots gets different noise
    again = _gather(cuda, tab, items, sigma=sigma, clip=clip, seed=seed)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))      # equal bits on a second launch
    other = _gather(cuda, tab, items, sigma=sigma, clip=clip, seed=seed + 1)
    assert not np.array_equal(got, other)


@pytest.mark.parametrize("N", [4096, 130])
def test_rotation_and_jitter_together(cuda, N):
    T, B, seed, sigma, clip = 50, 4, 9, 0.005, 0.05
    host, tab = _table(cuda, T, N)
    items = [7, 7, -1, 3]
    rot = _angles(B, seed=11)
    got = _gather(cuda, tab, items, rot=rot, sigma=sigma, clip=clip, seed=seed)
    ref = R.gather_tuples(host, items, rot=rot, sigma=sigma, clip=clip, seed=seed)
    src = R.gather_tuples(host, items)
    c, s = np.abs(rot[:, 0].astype(np.float64))[:, None], np.abs(rot[:, 1].astype(np.float64))[:, None]
    rb = np.zeros_like(ref)
    rb[..., 0] = 3 * 2.0 ** -24 * (np.abs(src[..., 0]) * c + np.abs(src[..., 1]) * s)
    rb[..., 1] = 3 * 2.0 ** -24 * (np.abs(src[..., 0]) * s + np.abs(src[..., 1]) * c)
    bound = rb + 2.0 ** -23 * np.maximum(1.0, np.abs(ref)) + float(np.float32(sigma)) * Z_CAP
    err = np.abs(got - ref)
    print(f"MEASURE gather_tuples/rotation+jitter/N{N} worst err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all() and (got[2] == 0).all()
    again = _gather(cuda, tab, items, rot=rot, sigma=sigma, clip=clip, seed=seed)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


# ---- TupleBank -------------------------------------------------------------------------------------------------------------------
T_BANK, N_BANK, P_, NG = 300, 256, 2, 18


def _line_lists(T, r_pos, r_near):
    x = np.arange(T)
    d = np.abs(x[:, None] - x[None, :])
    positives = [np.nonzero((d[i] <= r_pos) & (d[i] > 0))[0].tolist() for i in range(T)]
    near = [np.nonzero(d[i] <= r_near)[0].tolist() for i in range(T)]
    return positives, near


@pytest.fixture(scope="module")
def bank(cuda):
    from lpdnet_hip import tuples
    clouds = np.random.default_rng(5).uniform(-1, 1, size=(T_BANK, N_BANK, 3))      # float64: narrowed on the device
    positives, near = _line_lists(T_BANK, 5, 25)
    b = tuples.TupleBank(clouds, positives, near, device=cuda)
    b.host_clouds, b.positives, b.near = clouds, positives, near
    return b


def test_bank_table_and_samples(cuda, bank):
    from lpdnet_hip import tuples
    assert np.array_equal(bank.table.cpu().numpy(), bank.host_clouds.astype(np.float32))
    assert tuples.run_dry_guarantee(bank.T, bank.max_near, bank.max_pos, NG) == (True, True)
    queries = [0, 150, 299, 150]
    items = bank.sample(queries, P_, NG, seed=4)
    assert items.shape == (4, 2 + P_ + NG) and items.dtype == torch.int32 and items.is_cuda
    t = items.cpu().numpy()
    for b, q in enumerate(queries):
        assert t[b, 0] == q
        pos, neg, other = t[b, 1:1 + P_], t[b, 1 + P_:1 + P_ + NG], t[b, -1]
        assert set(pos) <= set(bank.positives[q]) and len(set(pos)) == P_
        assert not set(neg) & set(bank.near[q]) and len(set(neg)) == NG and (neg >= 0).all() and (neg < T_BANK).all()
        union = set(bank.positives[q]).union(*(bank.positives[j] for j in neg))
        assert 0 <= other < T_BANK and other not in union
    assert not np.array_equal(t[1], t[3])      # the same query in two rows: different draws
    assert torch.equal(items, bank.sample(queries, P_, NG, seed=4)) and not torch.equal(items, bank.sample(queries, P_, NG, seed=5))
    # the draws are the restatement's, with the documented seeds
    off, idx = bank._near_csr
    want, _ = R.sample_items(off, idx, T_BANK, [[q] for q in queries], None, NG, 1, tuples.sub_seed(4, tuples.DRAW_NEGATIVES))
    assert np.array_equal(t[:, 1 + P_:1 + P_ + NG], want)
    off, idx = bank._pos_csr
    want, _ = R.sample_items(off, idx, T_BANK, [[q] for q in queries], None, P_, 0, tuples.sub_seed(4, tuples.DRAW_POSITIVES))
    assert np.array_equal(t[:, 1:1 + P_], want)
    # hard negatives first, not repeated in the fill
    hard = [[290, 291, 292], [10, 11, 12], [100, 101, 102], [0, 1, 2]]
    th = bank.sample(queries, P_, NG, seed=4, hard=hard).cpu().numpy()
    for b, q in enumerate(queries):
        neg = th[b, 1 + P_:1 + P_ + NG]
        assert neg[:3].tolist() == hard[b] and len(set(neg)) == NG and not set(neg[3:]) & set(bank.near[q])
    full = np.arange(100, 100 + NG).reshape(1, NG)
    assert bank.sample([299], P_, NG, seed=1, hard=torch.from_numpy(full).to(cuda)).cpu().numpy()[0, 1 + P_:-1].tolist() == full[0].tolist()
    # exclude_members: `other` is neither the query nor a negative
    te = bank.sample(queries, P_, NG, seed=4, exclude_members=True).cpu().numpy()
    assert np.array_equal(te[:, :-1], t[:, :-1]) and all(te[b, -1] not in te[b, :-1] for b in range(4))
    with pytest.raises(ValueError):
        bank.sample(queries, 11, NG, seed=0)      # at most 10 positives
    with pytest.raises(ValueError):
        bank.sample(queries, P_, NG, seed=0, hard=np.zeros((4, NG + 1), dtype=np.int32))


def test_bank_that_runs_dry_raises(cuda):
    from lpdnet_hip import tuples
    T = 20
    clouds = np.zeros((T, 4, 3), dtype=np.float32)
    everyone = [[j for j in range(T) if j != i] for i in range(T)]
    b = tuples.TupleBank(clouds, everyone, [[i] for i in range(T)], device=cuda)
    assert tuples.run_dry_guarantee(T, b.max_near, b.max_pos, 18) == (True, False)
    with pytest.raises(ValueError, match="other"):
        b.sample([3], 2, 18, seed=0)
    with pytest.raises(ValueError, match="candidates"):
        b.candidates([3], 20, seed=0)
    assert sorted(b.candidates([3], 19, seed=0).cpu().numpy()[0].tolist()) == [j for j in range(T) if j != 3]


def test_mine_equals_batched_hard_negatives(cuda, bank):
    from lpdnet_hip import harness
    g = np.random.default_rng(8)
    latent = g.standard_normal((T_BANK, 256)).astype(np.float32)
    latent /= np.linalg.norm(latent, axis=1, keepdims=True)
    dev_latent = torch.from_numpy(latent).to(cuda)
    queries = [7, 150, 280]
    cand = bank.candidates(queries, 100, seed=2)
    c = cand.cpu().numpy()
    assert c.shape == (3, 100) and all(len(set(c[b])) == 100 and not set(c[b]) & set(bank.near[q]) for b, q in enumerate(queries))
    want = harness.get_hard_negatives_batched(latent[queries], c.tolist(), 5, dev_latent)
    got = bank.mine(dev_latent, queries, 5, n_sampled=100, seed=2)
    assert got.is_cuda and got.cpu().numpy().tolist() == want
    qv = latent[queries] + 0.3 * g.standard_normal((3, 256)).astype(np.float32)
    want = harness.get_hard_negatives_batched(qv, c.tolist(), 5, dev_latent)
    assert bank.mine(dev_latent, queries, 5, n_sampled=100, seed=2, query_vecs=qv).cpu().numpy().tolist() == want


class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.seen = None

    def forward(self, x):
        self.seen = x
        return torch.zeros((x.shape[0], 256), device=x.device) + self.w


def test_assemble_equals_the_feed_of_run_model(cuda, bank):
    from lpdnet_hip import harness
    queries = [20, 250]
    items = bank.sample(queries, P_, NG, seed=9)
    feed = bank.assemble(items)
    assert feed.shape == (2 * (2 + P_ + NG), 1, N_BANK, 3) and feed.dtype == torch.float32
    t = items.cpu().numpy()
    host = torch.from_numpy(bank.host_clouds[t])      # [bq, 22, N, 3] float64, picked by the read-back item numbers
    rec = _Recorder().to(cuda)
    harness.run_model(rec, host[:, :1], host[:, 1:1 + P_], host[:, 1 + P_:1 + P_ + NG], host[:, -1:], require_grad=False)
    assert rec.seen.shape == feed.shape and torch.equal(rec.seen.view(torch.int32), feed.view(torch.int32))
    q, p, n, o = harness.run_model_feed(rec, feed, 2, P_, NG, require_grad=False)
    assert q.shape == (2, 1, 256) and p.shape == (2, P_, 256) and n.shape == (2, NG, 256) and o.shape == (2, 1, 256) and rec.seen is feed
    with pytest.raises(ValueError):
        harness.run_model_feed(rec, feed, 3, P_, NG)
    aug = bank.assemble(items, rotate=True, jitter=True, seed=3)
    assert aug.shape == feed.shape and not torch.equal(aug, feed) and torch.equal(aug, bank.assemble(items, rotate=True, jitter=True, seed=3))
    assert (aug - feed)[..., 2].abs().max().item() <= 0.05 + 2.0 ** -23      # z moves by the jitter alone


def test_train_step_from_bank(cuda):
    from lpdnet_hip import harness, tuples
    from oracle import lpd_oracle as orc
    from oracle import synth
    from util.PointNetVlad import PointNetVlad
    N, T = 1024, 24
    m = PointNetVlad(num_points=N, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
    m = m.to(cuda)
    positives, near = _line_lists(T, 2, 4)
    # every item is ONE cloud, except the four positives of query 12: its negatives and `other` equal the query (distance 0), its
    # positives do not, so the loss is at least the margin and has a gradient whatever the weights are
    c = synth.cloud(21, 5, N)
    clouds = np.repeat(c[:1], T, axis=0)
    clouds[[10, 11, 13, 14]] = c[1:]
    bk = tuples.TupleBank(clouds, positives, near, device=cuda)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    before = m.net_vlad.hidden1_weights.detach().clone()
    loss = harness.train_step_from_bank(m, opt, bk, [12], 2, 2, seed=1)
    print(f"MEASURE train_step_from_bank loss {loss.item():.6f}")
    assert loss.dim() == 0 and torch.isfinite(loss).item() and loss.item() > 0
    assert m.training and not torch.equal(before, m.net_vlad.hidden1_weights.detach())
    hard = bk.mine(torch.randn((T, 256), device=cuda), [12], 1, n_sampled=8, seed=0)
    loss2 = harness.train_step_from_bank(m, opt, bk, [12], 2, 2, seed=2, hard=hard, rotate=True, jitter=True)
    print(f"MEASURE train_step_from_bank (hard, rotate, jitter) loss {loss2.item():.6f}")
    assert torch.isfinite(loss2).item()
