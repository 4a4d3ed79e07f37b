"""Host side of the fused recall evaluation (harness.evaluate_pairs / evaluate_model): the truth-CSR builder and the aggregation are
pure functions, checked here against the reference's formulas (evaluate.py:33-93, 162-206) on hand-built inputs.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import retrieval_oracle as ro


def _harness():
    from lpdnet_hip import harness
    return harness


def test_all_pairs_is_the_reference_loop_order():
    h = _harness()
    want = [(m, n) for m in range(5) for n in range(5) if m != n]     # evaluate.py:57-60
    got = h.all_pairs(5)
    assert got.dtype == np.int32 and [tuple(r) for r in got.tolist()] == want


def test_truth_csr_lists_empty_lists_and_numpy_arrays():
    h = _harness()
    # 2 query runs (3 and 2 queries), 3 database runs; lists as Python lists and numpy arrays, some empty
    qsets = [
        [{0: [1, 2], 1: [], 2: np.array([7])}, {0: [], 1: [0], 2: []}, {0: np.array([], np.int64), 1: [4, 5, 6], 2: [3]}],
        [{0: [9], 1: [2], 2: [8, 1]}, {0: [], 1: [], 2: []}],
    ]
    pairs = np.array([(m, n) for m in range(3) for n in range(2) if m != n], np.int32)     # (0,1), (1,0), (2,0), (2,1)
    off, idx = h.build_truth_csr(qsets, [3, 2], 3, pairs)
    assert off.dtype == np.int32 and idx.dtype == np.int32 and off.shape == (5 * 3 + 1,) and off[0] == 0 and off[-1] == idx.size
    used = {(int(n), int(m)) for m, n in pairs}
    g = 0
    for n, cnt in enumerate([3, 2]):
        for i in range(cnt):
            for m in range(3):
                got = idx[off[g * 3 + m]:off[g * 3 + m + 1]].tolist()
                want = [int(t) for t in qsets[n][i][m]] if (n, m) in used else []
                assert got == want, (n, i, m)
            g += 1
    # no list at all
    off, idx = h.build_truth_csr([[{0: [], 1: []}]], [1], 2, np.array([[1, 0]], np.int32))
    assert off.tolist() == [0, 0, 0] and idx.size == 0


def _counts(rankings, truth, k, n_db):
    """what lpd_recall_pairs returns for one pair, from explicit rankings (first hit per query, one-percent flag)"""
    hist = np.zeros(k + 1, np.int64)
    n_eval = n_one = 0
    thr = min(max(int(round(n_db / 100.0)), 1), min(k, n_db))
    for rk, t in zip(rankings, truth):
        if len(t) == 0:
            continue
        n_eval += 1
        hits = [r for r, j in enumerate(rk) if j in set(t)]
        first = hits[0] if hits else k
        hist[first] += 1
        n_one += first < thr
    return hist, n_eval, n_one


@pytest.mark.parametrize("n_db", [300, 17, 250, 150])
def test_recall_curves_equal_the_reference_formula(n_db):
    """Per-pair curves and one-percent recall from the integer counts = evaluate.py:162-206 on the same rankings (the oracle's
    scoring loop), including a database run shorter than 25 (k = n_db, the curve keeps 25 entries), queries with empty truth and
    the round-half-to-even one-percent threshold (250 -> 2, 150 -> 2)."""
    h = _harness()
    g = np.random.default_rng(n_db)
    nq, k = 60, min(25, n_db)
    rankings = [g.permutation(n_db)[:k] for _ in range(nq)]
    truth = [[] if i % 7 == 0 else g.choice(n_db, size=int(g.integers(1, 6)), replace=False).tolist() for i in range(nq)]
    db = g.standard_normal((n_db, 8)).astype(np.float32)
    queries = np.concatenate([np.arange(nq, dtype=np.float32)[:, None], g.standard_normal((nq, 7)).astype(np.float32)], 1)
    want = ro._score(db, queries, truth, lambda q: rankings[int(q[0])], 25)      # (column 0 names the query)
    hist, n_eval, n_one = _counts(rankings, truth, 25, n_db)
    recall, one = h.recall_curves(hist[None], [n_eval], [n_one], 25)
    assert recall.shape == (1, 25)
    assert np.array_equal(recall[0], want[0]) and one[0] == want[2]


def test_recall_curves_raise_zero_division_like_the_reference():
    h = _harness()
    hist = np.zeros((2, 26), np.int64)
    hist[0, 3] = 4
    with pytest.raises(ZeroDivisionError):
        h.recall_curves(hist, [4, 0], [2, 0])
    with pytest.raises(ZeroDivisionError):
        ro._score(np.zeros((3, 2)), np.zeros((2, 2)), [[], []], lambda q: [0, 1, 2], 25)


def test_aggregate_evaluation_is_the_reference_aggregation():
    h = _harness()
    g = np.random.default_rng(4)
    pairs = []
    for _ in range(7):
        curve = np.cumsum(g.integers(0, 5, 25)) / 31.0 * 100
        sims = [float(v) for v in g.random(int(g.integers(0, 4)))]
        pairs.append((curve, sims, float(g.random() * 100)))
    # evaluate.py:36-90 verbatim in structure
    recall = np.zeros(25)
    count = 0
    similarity, one_percent_recall = [], []
    for pr, ps, po in pairs:
        recall += np.array(pr)
        count += 1
        one_percent_recall.append(po)
        for x in ps:
            similarity.append(x)
    want = (np.mean(np.mean(recall / count)), np.mean(similarity), np.mean(one_percent_recall))
    got = h.aggregate_evaluation(np.stack([p[0] for p in pairs]), [p[2] for p in pairs], [x for p in pairs for x in p[1]])
    assert got == want
    assert np.ndim(got[0]) == 0            # a scalar: the mean over all 25 ranks, not Recall@1


def test_evaluate_model_without_a_gpu_raises(monkeypatch):
    from lpdnet_hip import harness, _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    model = torch.nn.Linear(3, 3)
    with pytest.raises(_lib.LpdHipError):
        harness.evaluate_model(model, [np.zeros((1, 8, 3))], [np.zeros((1, 8, 3))], [[{0: []}]], 2)
    with pytest.raises(_lib.LpdHipError):
        harness.evaluate_pairs([np.zeros((3, 4), np.float32)], [np.zeros((3, 4), np.float32)], [[{0: [0]}] * 3])
    assert model.training
