"""Selection of the best-first kNN kernel on inputs made of exact ties.  -m gpu only.

The short-list instantiations (k <= 20) drain their admission queues in batches: each lane's queued candidates become 64-bit keys
(an order-preserving image of pd, then the complemented index), a sorting network orders the batch and a bitonic merge folds it into
the lane's sorted list.  The order of the keys IS the reference's rule (pd descending, lower index first), so nothing here may depend
on the order in which tiles are visited.  Every case compares EVERY row with the oracle (orc.knn_np); no row is excluded for ties.

  (a) clusters of m exact duplicates, m on both sides of the batch sizes (8, 16) and of k: ties inside the list and at the k-th boundary
  (b) 32 all-zero points: pd = +-0 among them; their rows must be 0..19
  (c) every even index one and the same point: some lanes' queues full at every tile, the others nearly empty
  (d) the inputs of (a) with k = 7: a short output from the 20-entry lists
  (e) a lattice cloud, one cloud of 4096 points: the launch that splits a query tile's walk among four waves
  (f) the same lattice, eight clouds: single-wave workgroups, long walks, many drains
Each input runs with 3 and with 64 channels (the two instantiations of the kernel) and through impl 0 (product dispatch) and 6 (forced).
The oracle's result is computed once per input and shared.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import lpd_oracle as orc

pytestmark = pytest.mark.gpu

_DUP_SIZES = (7, 8, 9, 15, 16, 17, 19, 20, 21, 24, 25, 31, 32, 33, 40)


def _clusters(C):
    g = np.random.default_rng(100 + C)
    B, N = 2, 512
    x = g.standard_normal((B, N, C)).astype(np.float32)
    for b in range(B):
        where = g.permutation(N)
        at = 0
        for m in _DUP_SIZES:
            x[b, where[at:at + m]] = g.standard_normal(C).astype(np.float32)
            at += m
    return x


def _zeros(C):
    g = np.random.default_rng(200 + C)
    x = g.standard_normal((1, 64, C)).astype(np.float32)
    x[0, :32] = 0.0
    return x


def _even_same(C):
    g = np.random.default_rng(300 + C)
    x = g.standard_normal((2, 256, C)).astype(np.float32)
    for b in range(2):
        x[b, 0::2] = g.standard_normal(C).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _lattice8(C):
    g = np.random.default_rng(400 + C)
    return (g.integers(-4, 5, size=(8, 4096, C)) / 4.0).astype(np.float32)


def _lattice1(C):
    return _lattice8(C)[:1]


_CASES = {
    "a-duplicate-clusters": (_clusters, 20),
    "b-zero-points": (_zeros, 20),
    "c-even-indices-one-point": (_even_same, 20),
    "d-duplicate-clusters-k7": (_clusters, 7),
    "e-lattice-one-cloud": (_lattice1, 20),
    "f-lattice-eight-clouds": (_lattice8, 20),
}


@functools.lru_cache(maxsize=None)
def _case(name, C):
    make, k = _CASES[name]
    x = np.ascontiguousarray(make(C))
    oidx, _ = orc.knn_np(x, k)
    oidx.setflags(write=False)
    return x, k, oidx


@pytest.mark.parametrize("impl", [0, 6])
@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_knn_batched_drain_every_row(cuda, name, C, impl):
    from lpdnet_hip import ops
    x, k, oidx = _case(name, C)
    B, N, _ = x.shape
    rows = torch.from_numpy(x.reshape(B * N, C)).to(cuda).contiguous()
    got = ops.knn_pm(rows, B, N, k, impl=impl).cpu().numpy().reshape(B, N, k)
    if name.startswith("b-"):
        assert (oidx[0, :32] == np.arange(20)).all(), "oracle: the zero points' neighbours are the first twenty zero points"
        assert (got[0, :32] == np.arange(20)).all(), got[0, :32]
    diff = (got != oidx).any(-1)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} rows differ; first: {np.argwhere(diff)[:3].tolist()}"
