"""The fused recall evaluation (lpd_recall_pairs: every (database run, query run) pair of evaluate.py:33-93 in one launch) against
the per-pair path (harness.get_recall / ops.retrieval_topk), the brute-force oracle and the reference's own KDTree routine.  -m gpu."""
import os

import numpy as np
import pytest
import torch

from oracle import lpd_oracle as orc
from oracle import retrieval_oracle as ro
from oracle import synth

pytestmark = pytest.mark.gpu


def _four_runs():
    """synthetic_runs(seed=7, 3 runs of 300 / 170 / 410) plus a fourth run of 17 descriptors (shorter than recall_num = 25), with
    truth lists for every combination (some empty)"""
    db, _, qsets = ro.synthetic_runs(seed=7, runs=3, per_run=(300, 170, 410))
    g = np.random.default_rng(8)
    short = g.standard_normal((17, 256))
    short = (short / np.linalg.norm(short, axis=1, keepdims=True)).astype(np.float32)
    vecs = list(db) + [short]
    sizes = [len(v) for v in vecs]
    for n in range(3):
        for i in range(sizes[n]):
            qsets[n][i][3] = [] if g.random() < 0.2 else g.choice(17, size=int(g.integers(1, 4)), replace=False).tolist()
    qsets.append([{m: ([] if g.random() < 0.1 else g.choice(sizes[m], size=int(g.integers(1, 5)), replace=False).tolist())
                   for m in range(4)} for _ in range(17)])
    return vecs, qsets


def _launch(vecs, qsets, cuda, k=25, pairs=None):
    from lpdnet_hip import harness, ops
    R = len(vecs)
    pairs = harness.all_pairs(R) if pairs is None else pairs
    off = np.zeros(R + 1, np.int64)
    np.cumsum([len(v) for v in vecs], out=off[1:])
    table = torch.from_numpy(np.concatenate(vecs)).to(cuda)
    to, ti = harness.build_truth_csr(qsets, np.diff(off), R, pairs)
    r = ops.recall_pairs(table, table, off.astype(np.int32), off.astype(np.int32), pairs, to, ti, k, want_topk=True)
    return pairs, r


def test_recall_pairs_topk_matches_numpy_and_retrieval_topk(cuda):
    from lpdnet_hip import ops
    vecs, qsets = _four_runs()
    pairs, r = _launch(vecs, qsets, cuda)
    topk = r.topk_idx.cpu().numpy()
    assert topk.shape == (r.out_off[-1], 25)
    for p, (m, n) in enumerate(pairs):
        rows = slice(r.out_off[p], r.out_off[p + 1])
        kp = min(25, len(vecs[m]))
        d2 = ((vecs[n][:, None, :].astype(np.float64) - vecs[m][None].astype(np.float64)) ** 2).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")[:, :kp]
        assert (topk[rows, :kp] == order).all(), (m, n)
        assert (topk[rows, kp:] == -1).all()
        idx, _ = ops.retrieval_topk(torch.from_numpy(vecs[n]).to(cuda), torch.from_numpy(vecs[m]).to(cuda), kp)
        assert (topk[rows, :kp] == idx.cpu().numpy()).all(), (m, n)


def test_recall_pairs_ties_go_to_the_lower_index(cuda):
    """duplicated database rows: a query equal to them is equidistant from all copies; the lower index ranks first, exactly as in
    retrieval_topk"""
    from lpdnet_hip import harness, ops
    g = np.random.default_rng(21)
    db = g.standard_normal((90, 256)).astype(np.float32)
    v = db[5].copy()
    for j in (17, 40, 41, 77):
        db[j] = v
    w = g.standard_normal(256).astype(np.float32)
    db[60] = w
    db[61] = w
    queries = np.stack([v, w, v + np.float32(1e-3), g.standard_normal(256).astype(np.float32)])
    qsets = [[], [{0: [40]}, {0: [61]}, {0: [77]}, {0: []}]]
    vecs = [db, queries]
    pairs = np.array([[0, 1]], np.int32)
    pairs, r = _launch(vecs, [qsets[0], qsets[1]], cuda, pairs=pairs)
    topk = r.topk_idx.cpu().numpy()
    idx, _ = ops.retrieval_topk(torch.from_numpy(queries).to(cuda), torch.from_numpy(db).to(cuda), 25)
    assert (topk == idx.cpu().numpy()).all()
    assert topk[0, :5].tolist() == [5, 17, 40, 41, 77] and topk[1, :2].tolist() == [60, 61]
    assert r.first.cpu().tolist() == [2, 1, 4, -1] and r.n_eval.cpu().tolist() == [3]
    assert r.hist.cpu().numpy()[0, [1, 2, 4]].tolist() == [1, 1, 1]
    del harness


@pytest.mark.parametrize("form", ["lists", "numpy", "resident"])
def test_evaluate_pairs_equals_get_recall_and_the_oracle(cuda, form):
    from lpdnet_hip import harness
    vecs, qsets = _four_runs()
    if form == "numpy":
        qsets = [[{m: np.asarray(t, np.int64) for m, t in e.items()} for e in run] for run in qsets]
    arg = vecs
    if form == "resident":
        off = np.zeros(5, np.int64)
        np.cumsum([len(v) for v in vecs], out=off[1:])
        arg = (torch.from_numpy(np.concatenate(vecs)).to(cuda), off)
    got = harness.evaluate_pairs(arg, arg, qsets)
    pairs = harness.all_pairs(4)
    assert len(got) == len(pairs)
    empty_truth = 0
    for (m, n), (rec, sims, opr) in zip(pairs, got):
        a = harness.get_recall(m, n, vecs, vecs, qsets)
        b = ro.get_recall_bruteforce(m, n, vecs, vecs, qsets)
        assert rec.shape == (25,)
        for want in (a, b):
            assert np.allclose(rec, want[0]) and opr == want[2]
            assert len(sims) == len(want[1]) and np.allclose(sims, want[1], atol=1e-6)
        assert np.array_equal(rec, a[0])
        empty_truth += sum(len(qsets[n][i][m]) == 0 for i in range(len(vecs[n])))
    assert empty_truth > 0


def _model(cuda, N):
    from util.PointNetVlad import PointNetVlad
    m = PointNetVlad(num_points=N, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
    return m.to(cuda)


def _cloud_runs():
    """3 database runs (26 / 27 / 25 clouds: >= 25 for the reference's KDTree query) and 3 query runs (7 / 9 / 5) of N = 256 points:
    jittered copies of 30 places; truth = the same place in the other run"""
    N = 256
    places = synth.cloud(31, 30, N).astype(np.float64)
    g = np.random.default_rng(32)

    def run(size):
        ids = np.sort(g.choice(30, size=size, replace=False))
        return ids, places[ids] + 0.01 * g.standard_normal((size, N, 3))
    db = [run(s) for s in (26, 27, 25)]
    qs = [run(s) for s in (7, 9, 5)]
    qsets = [[{m: np.nonzero(db[m][0] == pid)[0].tolist() for m in range(3)} for pid in qs[n][0]] for n in range(3)]
    return [c for _, c in db], [c for _, c in qs], qsets


def _reference_evaluation(model, db_clouds, q_clouds, qsets, batch_size):
    from lpdnet_hip import harness
    DB = [harness.get_latent_vectors(model, c, batch_size) for c in db_clouds]
    QV = [harness.get_latent_vectors(model, c, batch_size) for c in q_clouds]
    recall = np.zeros(25)
    count = 0
    similarity, one_percent_recall = [], []
    for m in range(3):
        for n in range(3):
            if m == n:
                continue
            pr, ps, po = ro.get_recall_kdtree(m, n, DB, QV, qsets)
            recall += np.array(pr)
            count += 1
            one_percent_recall.append(po)
            similarity += list(ps)
    return np.mean(np.mean(recall / count)), np.mean(similarity), np.mean(one_percent_recall)


def test_evaluate_model_matches_the_reference_evaluation(cuda):
    from lpdnet_hip import harness
    model = _model(cuda, 256)
    model.train()
    db, qs, qsets = _cloud_runs()
    got = harness.evaluate_model(model, db, qs, qsets, batch_size=4)          # 26 = 6 x 4 + 2, ...: ragged tails
    assert model.training
    want = _reference_evaluation(model, db, qs, qsets, 4)
    assert 0 < want[0] <= 100 and 0 < want[2] <= 100
    assert abs(got[0] - want[0]) < 1e-9 and abs(got[2] - want[2]) < 1e-9
    assert abs(got[1] - want[1]) < 1e-6


def test_evaluate_model_from_sets_reads_the_reference_pickle_structure(cuda, tmp_path):
    from lpdnet_hip import harness, ingest
    model = _model(cuda, 256)
    db, qs, qsets = _cloud_runs()
    DATABASE_SETS, QUERY_SETS = [], []
    for r, clouds in enumerate(db):
        run = {}
        for i, c in enumerate(clouds):
            name = f"db{r}_{i}.bin"
            np.ascontiguousarray(c, np.float64).tofile(os.path.join(tmp_path, name))
            run[i] = {"query": name, "northing": float(i), "easting": 0.0}
        DATABASE_SETS.append(run)
    np.zeros(100, np.float64).tofile(os.path.join(tmp_path, "broken.bin"))     # wrong size: skipped like load_pc_files does
    DATABASE_SETS[1][len(DATABASE_SETS[1])] = {"query": "broken.bin", "northing": 0.0, "easting": 0.0}
    for n, clouds in enumerate(qs):
        run = {}
        for i, c in enumerate(clouds):
            name = f"q{n}_{i}.bin"
            np.ascontiguousarray(c, np.float64).tofile(os.path.join(tmp_path, name))
            run[i] = dict(qsets[n][i], query=name, northing=float(i), easting=0.0)
        QUERY_SETS.append(run)
    model.eval()
    got = ingest.evaluate_model_from_sets(model, DATABASE_SETS, QUERY_SETS, 4, dataset_folder=str(tmp_path), num_points=256)
    assert model.training
    want = harness.evaluate_model(model, db, qs, qsets, batch_size=4)
    assert abs(got[0] - want[0]) < 1e-9 and abs(got[2] - want[2]) < 1e-9 and abs(got[1] - want[1]) < 1e-6


def test_recall_pairs_medium_shape_against_the_oracle(cuda):
    """6 runs of ~2000 descriptors: several query tiles per pair and 60+ database tiles per workgroup"""
    from lpdnet_hip import harness
    sizes = (2000, 1900, 2100, 1800, 2050, 1950)
    vecs, _, qsets = ro.synthetic_runs(seed=3, runs=6, per_run=sizes)
    got = harness.evaluate_pairs(vecs, vecs, qsets)
    pairs = harness.all_pairs(6)
    for p, (m, n) in enumerate(pairs):
        want = harness.get_recall(m, n, vecs, vecs, qsets)
        assert np.array_equal(got[p][0], want[0]) and got[p][2] == want[2]
        assert np.allclose(got[p][1], want[1], atol=1e-6)
    for p in (0, 7, 13, 22, 29):                                  # the brute-force oracle on a spread of pairs (fp64, per query)
        m, n = pairs[p]
        want = ro.get_recall_bruteforce(m, n, vecs, vecs, qsets)
        assert np.allclose(got[p][0], want[0]) and got[p][2] == want[2]
        assert np.allclose(got[p][1], want[1], atol=1e-6)
