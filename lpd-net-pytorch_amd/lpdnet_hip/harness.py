"""Counterparts of the two callers that sit directly on the hot path.

The reference's train/eval scripts (`train_pointnetvlad.py`, `evaluate.py`) read argparse singletons, pickles and
the Oxford dataset at import time and never travel; these functions reproduce exactly what those scripts do
AROUND the model call, with plain arguments:

  run_model          train_pointnetvlad.py:202-217   cat(q, pos, neg, other) -> [B,1,N,3] -> model -> split
  train_step         train_pointnetvlad.py:121-134   zero_grad / run_model / loss / backward / optimizer.step
  get_latent_vectors evaluate.py:96-159              eval mode, batched forward with a ragged tail, numpy out,
                                                     model.train() afterwards
  run_model_feed /   the same two on a feed that lpdnet_hip.tuples.TupleBank sampled, gathered and augmented on the device
  train_step_from_bank                               (util/data.py:56-101, 190-271 and loading_pointclouds.py:50-85 on the host there)
and the two "next" rows of SURVEY.md section 8f that sit right behind them:
  get_recall         evaluate.py:162-206             Recall@N / top-1 similarity / one-percent recall of one (database run,
                                                     query run) pair; the KDTree per pair becomes one GPU top-k launch
  evaluate_model     evaluate.py:33-93               the whole evaluation: every run embedded into one resident table (embed_runs),
                                                     every (m, n) pair scored in ONE lpd_recall_pairs launch (evaluate_pairs), the
                                                     reference's aggregation on the host
  get_random_hard_negatives  util/data.py:103-115    the hard_neg_num nearest of the sampled negatives of a query (KDTree over 4000
                                                     latent vectors per item there; one GPU top-k launch here)
  save_checkpoint /  train_pointnetvlad.py:64-77,    the reference's .ckpt dict (epoch, iter, state_dict, optimizer, recall)
  load_pretrained    172-199                         and bare .t7 state_dicts, with or without the DataParallel `module.` prefix
"""
import numpy as np
import torch

import loss.pointnetvlad_loss as L


def run_model(model, queries, positives, negatives, other_neg, require_grad=True, output_dim=256):
    """queries [bq,1,N,3], positives [bq,P,N,3], negatives [bq,Ng,N,3], other_neg [bq,1,N,3] (any device/dtype)
    -> (q [bq,1,D], pos [bq,P,D], neg [bq,Ng,D], other [bq,1,D]); cloud order inside a tuple = q, pos, neg, other."""
    bq, P, Ng = queries.shape[0], positives.shape[1], negatives.shape[1]
    N = queries.shape[2]
    feed = torch.cat((queries, positives, negatives, other_neg), 1).reshape(-1, 1, N, 3)
    dev = next(model.parameters()).device
    feed = feed.to(dev, dtype=torch.float32, non_blocking=True)
    if require_grad:
        out = model(feed)
    else:
        with torch.no_grad():
            out = model(feed)
    out = out.view(bq, -1, output_dim)
    return torch.split(out, [1, P, Ng, 1], dim=1)


def train_step(model, optimizer, queries, positives, negatives, other_neg, *, margin_1=0.5, margin_2=0.2,
               loss_function="quadruplet", use_min=True, lazy=True, ignore_zero_loss=False):
    """One optimisation step with the reference's defaults (util/initPara.py:32-88: margins 0.5/0.2, quadruplet,
    lazy, best positive).  Returns the loss tensor (0-dim, on the device)."""
    model.train()
    optimizer.zero_grad()
    q, p, n, o = run_model(model, queries, positives, negatives, other_neg)
    fn = L.quadruplet_loss if loss_function == "quadruplet" else L.triplet_loss_wrapper
    loss = fn(q, p, n, o, margin_1, margin_2, use_min=use_min, lazy=lazy, ignore_zero_loss=ignore_zero_loss)
    loss.backward()
    optimizer.step()
    return loss


def run_model_feed(model, feed, bq, P, Ng, require_grad=True, output_dim=256):
    """run_model on a feed that is already assembled on the device (tuples.TupleBank.assemble): feed [bq * (2+P+Ng), 1, N, 3] fp32
    in the tuple order q, pos, neg, other -> (q [bq,1,D], pos [bq,P,D], neg [bq,Ng,D], other [bq,1,D])."""
    if feed.shape[0] != bq * (2 + P + Ng):
        raise ValueError(f"run_model_feed: feed holds {feed.shape[0]} clouds, bq * (2 + P + Ng) = {bq * (2 + P + Ng)}")
    if require_grad:
        out = model(feed)
    else:
        with torch.no_grad():
            out = model(feed)
    out = out.view(bq, -1, output_dim)
    return torch.split(out, [1, P, Ng, 1], dim=1)


def train_step_from_bank(model, optimizer, bank, query_items, P, Ng, seed, hard=None, rotate=False, jitter=False, *, margin_1=0.5,
                         margin_2=0.2, loss_function="quadruplet", use_min=True, lazy=True, ignore_zero_loss=False):
    """train_step fed from a resident tuples.TupleBank: query_items are host integers; the tuples are sampled (bank.sample), gathered
    and augmented (bank.assemble) on the device, then run_model_feed / loss / backward / optimizer.step as train_step does.  `seed`
    (e.g. the iteration number) drives the sampling, the rotation angles and the jitter.  Returns the loss tensor."""
    model.train()
    optimizer.zero_grad()
    items = bank.sample(query_items, P, Ng, seed, hard=hard)
    feed = bank.assemble(items, rotate=rotate, jitter=jitter, seed=seed)
    q, p, n, o = run_model_feed(model, feed, items.shape[0], P, Ng)
    fn = L.quadruplet_loss if loss_function == "quadruplet" else L.triplet_loss_wrapper
    loss = fn(q, p, n, o, margin_1, margin_2, use_min=use_min, lazy=lazy, ignore_zero_loss=ignore_zero_loss)
    loss.backward()
    optimizer.step()
    return loss


_RINGS = {}


def _stream_ring(device, n):
    """The n HIP streams of a pipeline, ONE ring per (device, n, host thread), kept for the life of the process.  A pipeline is created
    per call (PointNetVlad.forward makes one for every eval batch above 32 clouds): with fresh torch.cuda.Stream objects each time the
    caching allocator -- whose free blocks belong to the stream that allocated them -- met every forward with empty pools and went to
    hipMalloc inside it (128 clouds per step: 8.4 ms against 7.2 ms for the four slices one after the other)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), n, __import__("threading").get_ident())
    ring = _RINGS.get(key)
    if ring is None:
        ring = _RINGS[key] = [torch.cuda.Stream(device=dev) for _ in range(n)]
    return ring


class BatchPipeline:
    """Embeds a SEQUENCE of independent eval batches with `in_flight` of them on the GPU at once (round 6).

    The stages of one forward are bound by different units -- the two kNN searches by latency (a third of their wave time issuing),
    conv3 and the fused edge MLP by the matrix cores, the K-agg and the pooling product by HBM -- so the stages of TWO consecutive
    batches fill each other's gaps: batch i runs on HIP stream i % in_flight (each with its own second stream for the xyz search,
    engine._side_stream), nothing else changes -- the same launches with the same arguments, bit-identical descriptors.  Measured at
    32 clouds x 4096 points per batch: 1.76-1.80 -> 1.64 ms per batch with two in flight (three: the same).  Latency of one batch
    grows (it shares the chip); throughput is what the callers of this class are after (evaluate.py:96-159 embeds whole runs).

        pipe = BatchPipeline(model)              # the model in eval mode
        outs = [pipe.submit(x) for x in batches] # enqueues; an output is valid once its stream gets there
        pipe.join()                              # ... or for the caller's stream after this
    """

    def __init__(self, model, in_flight=2, device=None):
        if in_flight < 1:
            raise ValueError("BatchPipeline: in_flight >= 1")
        self.model = model
        self.device = device if device is not None else next(model.parameters()).device
        self.streams = _stream_ring(self.device, in_flight) if in_flight > 1 else []
        self.count = 0
        self._used = set()

    def submit(self, x):
        """model(x) under no_grad on the next stream of the ring; x may still be in production on the caller's current stream"""
        if not self.streams:
            with torch.no_grad():
                return self.model(x)
        cur = torch.cuda.current_stream(self.device)
        s = self.streams[self.count % len(self.streams)]
        self.count += 1
        s.wait_stream(cur)                       # x (and the weights) as the caller's stream leaves them
        if isinstance(x, torch.Tensor) and x.is_cuda:
            x.record_stream(s)
        from . import engine
        was = engine._TLS.PIPELINED
        engine._TLS.PIPELINED = True             # (the forward then keeps its own second stream for small batches only)
        try:
            with torch.cuda.stream(s), torch.no_grad():
                out = self.model(x)
        finally:
            engine._TLS.PIPELINED = was
        out.record_stream(cur)                   # the caller will read it on ITS stream after join()
        self._used.add(s)
        return out

    def join(self):
        """the caller's current stream waits for every batch submitted so far"""
        cur = torch.cuda.current_stream(self.device)
        for s in self._used:
            cur.wait_stream(s)
        self._used.clear()


PIPELINE_IN_FLIGHT = 2      # batches in flight inside get_latent_vectors / update_vectors / large eval batches (1: one after the other)


def get_latent_vectors(model, clouds, batch_size):
    """clouds: [n, N, 3] array-like (float64 like the benchmark's .bin submaps, or float32) -> [n, D] float32 numpy.

    Mirrors evaluate.get_latent_vectors: full batches of `batch_size` clouds, then the ragged remainder in one
    call, eval mode inside, train mode restored afterwards (evaluate.py:97,156).  The batches are independent: two of them are in
    flight at a time (BatchPipeline)."""
    was_training = model.training
    model.eval()
    dev = next(model.parameters()).device
    clouds = np.asarray(clouds)
    n = clouds.shape[0]
    outs = []
    try:
        pipe = BatchPipeline(model, PIPELINE_IN_FLIGHT if dev.type == "cuda" else 1, dev)
        for s in range(0, n, batch_size):
            chunk = torch.from_numpy(np.ascontiguousarray(clouds[s:s + batch_size])).float().unsqueeze(1).to(dev)
            outs.append(pipe.submit(chunk))
        pipe.join()
        outs = [o.detach().cpu().numpy() for o in outs]
    finally:
        model.train(was_training)
    if not outs:
        return np.zeros((0, 0), dtype=np.float32)
    return np.concatenate(outs, axis=0)


RECALL_NUM = 25   # evaluate.py:19


def get_recall(m, n, DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num=RECALL_NUM, device=None):
    """evaluate.py:162-206 with the per-pair KDTree replaced by one launch of lpd_retrieval_topk.
    DATABASE_VECTORS[m] [n_db, D], QUERY_VECTORS[n] [n_q, D] (numpy, as get_latent_vectors returns them);
    QUERY_SETS[n][i][m] = indices of the true neighbours of query i of run n in run m.
    -> (recall [recall_num] cumulative percent, top-1 similarity scores, one-percent recall)."""
    from . import ops
    database_output, queries_output = DATABASE_VECTORS[m], QUERY_VECTORS[n]
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    D = torch.as_tensor(np.ascontiguousarray(database_output), dtype=torch.float32, device=dev)
    Q = torch.as_tensor(np.ascontiguousarray(queries_output), dtype=torch.float32, device=dev)
    k = min(recall_num, len(database_output))
    idx, _ = ops.retrieval_topk(Q, D, k)                                    # [n_q, k] int32 on the device, nearest first
    n_q = len(queries_output)
    # the true-neighbour lists as one padded [n_q, max_len] table (-1 = padding): the rank walk below is then three tensor
    # expressions instead of a Python loop with a set per query (at Oxford scale ~3 k queries x 23 x 22 run pairs)
    sets = [QUERY_SETS[n][i][m] for i in range(n_q)]
    lens = np.fromiter((len(t) for t in sets), dtype=np.int64, count=n_q)
    num_evaluated = int((lens > 0).sum())
    recall = np.zeros(recall_num, dtype=np.int64)
    top1_similarity_score = []
    one_percent_retrieved = 0
    threshold = max(int(round(len(database_output) / 100.0)), 1)
    if num_evaluated:
        width = int(lens.max())
        truth = np.full((n_q, width), -1, dtype=np.int64)
        truth[np.arange(width)[None, :] < lens[:, None]] = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in sets])
        truth_d = torch.from_numpy(truth).to(dev)
        hit = torch.zeros((n_q, k), dtype=torch.bool, device=dev)
        rows = max(1, (1 << 24) // max(1, k * width))                        # bounded [rows, k, width] comparison blocks
        for s0 in range(0, n_q, rows):
            hit[s0:s0 + rows] = (idx[s0:s0 + rows].long().unsqueeze(2) == truth_d[s0:s0 + rows].unsqueeze(1)).any(dim=2)
        found = hit.any(dim=1)                                               # queries without true neighbours never hit (-1)
        first = torch.where(found, hit.to(torch.uint8).argmax(dim=1), torch.full((n_q,), k, device=dev))
        recall[:k] = torch.bincount(first, minlength=k + 1)[:k].cpu().numpy()
        one_percent_retrieved = int(hit[:, :min(threshold, k)].any(dim=1).sum().item())
        at0 = torch.nonzero(first == 0).flatten().cpu().numpy()              # rank-0 hits, in query order (evaluate.py:188-190)
        if at0.size:
            best = idx[:, 0].cpu().numpy()[at0]
            qn, dn = np.asarray(queries_output), np.asarray(database_output)
            top1_similarity_score = [float(v) for v in np.einsum("ij,ij->i", qn[at0], dn[best])]
    one_percent_recall = (one_percent_retrieved / float(num_evaluated)) * 100
    recall = (np.cumsum(recall) / float(num_evaluated)) * 100
    return recall, top1_similarity_score, one_percent_recall


def _cuda_device_or_raise(what, device=None):
    if not torch.cuda.is_available():
        from ._lib import LpdHipError
        raise LpdHipError(f"{what}: no GPU visible; the recall evaluation runs on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _embed_batches(model, batches, dev):
    """model(batch) for every batch of the iterable in eval mode, PIPELINE_IN_FLIGHT batches on the GPU at once; -> list of outputs
    (valid on the caller's stream).  The caller restores the train/eval mode."""
    model.eval()
    pipe = BatchPipeline(model, PIPELINE_IN_FLIGHT if torch.device(dev).type == "cuda" else 1, dev)
    outs = [pipe.submit(b) for b in batches]
    pipe.join()
    return outs


def embed_runs(model, runs, batch_size):
    """Descriptors of several runs as ONE resident table: runs = list of [n_r, N, 3] array-likes (float64 like the .bin submaps, or
    float32), each embedded as get_latent_vectors does (batches of `batch_size`, ragged tail, eval mode, BatchPipeline) but nothing
    comes back to the host.  -> (table CUDA fp32 [sum n_r, D], offsets numpy int64 [len(runs) + 1]); run r = rows offsets[r] ..
    offsets[r + 1].  The model's train/eval mode is restored.  An empty run raises ValueError."""
    dev = next(model.parameters()).device
    runs = [np.asarray(r) for r in runs]
    for i, r in enumerate(runs):
        if r.ndim != 3 or r.shape[0] == 0 or r.shape[2] != 3:
            raise ValueError(f"embed_runs: run {i} must be a non-empty [n, N, 3] array, got shape {r.shape}")
    counts = np.array([r.shape[0] for r in runs], dtype=np.int64)

    def batches():
        for r in runs:
            for s in range(0, r.shape[0], batch_size):
                yield torch.from_numpy(np.ascontiguousarray(r[s:s + batch_size])).float().unsqueeze(1).to(dev)
    was_training = model.training
    try:
        outs = _embed_batches(model, batches(), dev)
    finally:
        model.train(was_training)
    offsets = np.zeros(len(runs) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return torch.cat([o.reshape(o.shape[0], -1) for o in outs], 0).float(), offsets


def all_pairs(runs):
    """evaluate.py:57-60: every (database run m, query run n) with m != n, m outer -> int32 [runs * (runs - 1), 2]"""
    m, n = np.meshgrid(np.arange(runs), np.arange(runs), indexing="ij")
    keep = m != n
    return np.stack([m[keep], n[keep]], 1).astype(np.int32)


def build_truth_csr(QUERY_SETS, q_counts, n_db_runs, pairs):
    """The truth lists of an evaluation as ONE CSR table (what lpd_recall_pairs reads): the list QUERY_SETS[n][i][m] of global query
    row g = sum(q_counts[:n]) + i is truth_idx[truth_off[g * n_db_runs + m] : truth_off[g * n_db_runs + m + 1]].  Only the (n, m) run
    combinations that appear in `pairs` ([P, 2] rows (m, n)) are read; the others stay empty.  Lists may be Python lists or numpy
    arrays (empty ones: the query is not evaluated in that run).  -> (truth_off int32 [sum(q_counts) * n_db_runs + 1], truth_idx int32)."""
    import itertools
    q_counts = [int(c) for c in q_counts]
    need = np.zeros((len(q_counts), n_db_runs), dtype=bool)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    need[pairs[:, 1], pairs[:, 0]] = True
    empty = ()

    def lists():
        for n, cnt in enumerate(q_counts):
            want = need[n]
            if not want.any():                           # a query run no pair reads: its entries are never touched
                yield from itertools.repeat(empty, cnt * n_db_runs)
                continue
            run = QUERY_SETS[n]
            for i in range(cnt):
                entry = run[i]
                for m in range(n_db_runs):
                    yield entry[m] if want[m] else empty
    total = sum(q_counts) * n_db_runs
    seqs = list(lists())                                   # one walk over the nested structure
    lens = np.fromiter(map(len, seqs), dtype=np.int64, count=total)
    truth_off = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(lens, out=truth_off[1:])
    if truth_off[-1] >= 2 ** 31:
        raise ValueError("build_truth_csr: more than 2^31 truth entries")
    idx = np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int64, count=int(truth_off[-1]))
    return truth_off.astype(np.int32), idx.astype(np.int32)


def recall_curves(hist, n_eval, n_onepct, recall_num=RECALL_NUM):
    """Per-pair results of get_recall (evaluate.py:162-206) from the integer counts of lpd_recall_pairs, in float64 with the
    reference's expressions: hist [P, >= recall_num] (queries whose first true neighbour is at rank r; the columns past the pair's
    k are zero or the not-found count and are not read), n_eval [P], n_onepct [P].
    -> (recall [P, recall_num] cumulative percent, one_percent_recall [P]).  A pair without an evaluated query raises
    ZeroDivisionError, as the reference's `/ float(num_evaluated)` does."""
    hist = np.asarray(hist, dtype=np.int64)
    n_eval = np.asarray(n_eval, dtype=np.int64).reshape(-1)
    if (n_eval == 0).any():
        raise ZeroDivisionError(f"float division by zero (pair {int(np.argmax(n_eval == 0))} has no query with true neighbours)")
    ev = n_eval.astype(np.float64)
    recall = (np.cumsum(hist[:, :recall_num], axis=1) / ev[:, None]) * 100
    one = (np.asarray(n_onepct, dtype=np.int64).reshape(-1) / ev) * 100
    return recall, one


def aggregate_evaluation(recall, one_percent_recall, similarities):
    """evaluate.py:62-90 from the per-pair results: ave_recall = mean over the recall_num ranks of (sum of the pair curves, added in
    pair order) / pair count -- a scalar, as the reference computes it; average_similarity_score = mean of every rank-0 similarity;
    ave_one_percent_recall = mean of the per-pair one-percent recalls."""
    recall = np.asarray(recall, dtype=np.float64)
    count = recall.shape[0]
    total = np.cumsum(recall, axis=0)[-1]                  # recall += pair_recall, one pair after the other
    ave_recall = np.mean(np.mean(total / count))
    average_similarity_score = np.mean(np.asarray(similarities, dtype=np.float64))
    ave_one_percent_recall = np.mean(np.asarray(one_percent_recall, dtype=np.float64))
    return ave_recall, average_similarity_score, ave_one_percent_recall


def _resident(vectors, dev, name):
    """a list of per-run descriptor arrays / tensors, or (CUDA table, offsets) -> (CUDA fp32 table, offsets numpy int64)"""
    if (isinstance(vectors, tuple) and len(vectors) == 2 and isinstance(vectors[0], torch.Tensor) and vectors[0].dim() == 2
            and np.asarray(vectors[1]).ndim == 1):
        table, off = vectors
        off = np.asarray(off, dtype=np.int64)
        return table.to(dev, torch.float32), off
    runs = [v.detach().float().to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
            for v in vectors]
    for i, r in enumerate(runs):
        if r.dim() != 2:
            raise ValueError(f"{name}[{i}]: expected [n, D] descriptors, got shape {tuple(r.shape)}")
    off = np.zeros(len(runs) + 1, dtype=np.int64)
    np.cumsum([r.shape[0] for r in runs], out=off[1:])
    return torch.cat(runs, 0), off


def _evaluate_counts(DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num, pairs, device=None):
    from . import ops
    dev = _cuda_device_or_raise("evaluate", device)
    if not 1 <= recall_num <= ops.RECALL_KMAX:
        raise ValueError(f"evaluate: recall_num={recall_num} (1..{ops.RECALL_KMAX} on the fused kernel; get_recall takes any)")
    D, d_off = _resident(DATABASE_VECTORS, dev, "DATABASE_VECTORS")
    Q, q_off = _resident(QUERY_VECTORS, dev, "QUERY_VECTORS")
    pairs = all_pairs(len(QUERY_SETS)) if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    for what, off, col in (("database", d_off, 0), ("query", q_off, 1)):
        runs = off.size - 1
        if pairs.size and (pairs[:, col].min() < 0 or pairs[:, col].max() >= runs):
            raise ValueError(f"evaluate: a pair names {what} run outside the {runs} given")
        empty = np.nonzero(np.diff(off)[pairs[:, col]] == 0)[0]
        if empty.size:
            raise ValueError(f"evaluate: {what} run {int(pairs[empty[0], col])} is empty")
    from .places import TruthTable
    resident = isinstance(QUERY_SETS, TruthTable)      # the truth lists are on the device already (places.evaluation_truth)
    if resident:
        if QUERY_SETS.q_counts != np.diff(q_off).tolist() or QUERY_SETS.n_db_runs != d_off.size - 1:
            raise ValueError(f"evaluate: the TruthTable was made for query runs of {QUERY_SETS.q_counts} rows and {QUERY_SETS.n_db_runs} "
                             f"database runs; the descriptors have {np.diff(q_off).tolist()} and {d_off.size - 1}")
        truth_off, truth_idx = QUERY_SETS.truth_off.to(dev), QUERY_SETS.truth_idx.to(dev)
    else:
        truth_off, truth_idx = build_truth_csr(QUERY_SETS, np.diff(q_off), d_off.size - 1, pairs)
    r = ops.recall_pairs(Q, D, q_off.astype(np.int32), d_off.astype(np.int32), pairs, truth_off, truth_idx, recall_num,
                         truth_on_device=resident)
    first, sim = r.first.cpu().numpy(), r.top1_sim.cpu().numpy()
    return (r.hist.cpu().numpy(), r.n_eval.cpu().numpy(), r.n_onepct.cpu().numpy(), first, sim, r.out_off)


def evaluate_pairs(DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num=RECALL_NUM, pairs=None, device=None):
    """get_recall (evaluate.py:162-206) for many (database run m, query run n) pairs in ONE launch (lpd_recall_pairs): no score
    matrix, no per-pair uploads, the truth lists turned into one CSR table once.

    DATABASE_VECTORS / QUERY_VECTORS: lists of per-run [n, D] descriptors (numpy, as get_latent_vectors returns them, or tensors), or
    a resident (CUDA table, run offsets) tuple as embed_runs returns it.  QUERY_SETS[n][i][m] = true neighbours of query i of run n in
    run m -- or a places.TruthTable (places.evaluation_truth: the same lists made on the device from the positions), whose arrays
    are used where they are instead of the walk over the nested structure.  pairs: rows (m, n); default every m != n over range(len(QUERY_SETS)), m outer (the reference's loop order).
    -> list, one entry per pair: (recall [recall_num] cumulative percent, top-1 similarity list, one-percent recall), identical to
    get_recall(m, n, ...).

    Edge cases: a pair whose queries have no true neighbours at all raises ZeroDivisionError (as the reference and get_recall do);
    a database run shorter than recall_num is ranked to its length (k = n_db) and its curve still has recall_num entries; an empty run
    raises ValueError; recall_num is at most 64; without a GPU the call raises (there is no CPU path, as for get_recall)."""
    hist, n_eval, n_one, first, sim, out_off = _evaluate_counts(DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num, pairs, device)
    recall, one = recall_curves(hist, n_eval, n_one, recall_num)
    top = first == 0
    return [(recall[p], [float(v) for v in sim[out_off[p]:out_off[p + 1]][top[out_off[p]:out_off[p + 1]]]], float(one[p]))
            for p in range(recall.shape[0])]


def evaluate_from_descriptors(DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num=RECALL_NUM, pairs=None, device=None):
    """evaluate.py:33-93 after the embedding: -> (ave_recall, average_similarity_score, ave_one_percent_recall), aggregated on the
    host in float64 from the integer counts of one lpd_recall_pairs launch (inputs and edge cases as evaluate_pairs)."""
    hist, n_eval, n_one, first, sim, _ = _evaluate_counts(DATABASE_VECTORS, QUERY_VECTORS, QUERY_SETS, recall_num, pairs, device)
    recall, one = recall_curves(hist, n_eval, n_one, recall_num)
    return aggregate_evaluation(recall, one, sim[first == 0])


def evaluate_model(model, database_sets, query_sets, QUERY_SETS, batch_size):
    """evaluate.evaluate_model (evaluate.py:33-93) on clouds: database_sets / query_sets = lists of runs, each [n, N, 3] (float64 like
    the .bin submaps, or float32); QUERY_SETS[n][i][m] the truth.  Every run is embedded into one resident table (embed_runs), every
    (m, n) pair with m != n over range(len(QUERY_SETS)) scored in one launch (evaluate_pairs), and the results aggregated as the
    reference does.  -> (ave_recall, average_similarity_score, ave_one_percent_recall); ave_recall is the mean of the summed recall
    curve over all recall_num ranks (evaluate.py:73), not Recall@1.  The model is left in train mode (evaluate.py:156).
    Edge cases as evaluate_pairs: ZeroDivisionError for a pair without evaluated queries, ValueError for an empty run, an error
    without a GPU."""
    _cuda_device_or_raise("evaluate_model")
    try:
        db = embed_runs(model, database_sets, batch_size)
        qv = embed_runs(model, query_sets, batch_size)
    finally:
        model.train()
    return evaluate_from_descriptors(db, qv, QUERY_SETS)


def _unwrap(model):
    return model.module if hasattr(model, "module") and isinstance(model.module, torch.nn.Module) else model


def _strip_module_prefix(state_dict):
    """checkpoints written from an nn.DataParallel wrapper carry `module.` in front of every key (script.py:62-81)"""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        return {k[len("module."):]: v for k, v in state_dict.items()}
    return state_dict


def save_checkpoint(path, model, optimizer, epoch, total_iterations, recall):
    """train_pointnetvlad.py:172-199: the reference's .ckpt dictionary (weights of the unwrapped model)."""
    torch.save({"epoch": epoch, "iter": total_iterations, "state_dict": _unwrap(model).state_dict(),
                "optimizer": optimizer.state_dict(), "recall": float(recall)}, path)


def load_pretrained(model, path, optimizer=None, map_location="cpu", trust_checkpoint=True):
    """train_pointnetvlad.py:64-77: a path ending in '7' (.t7) holds a bare state_dict (loaded with strict=False), anything
    else the .ckpt dictionary (strict=True, optimizer state restored).  -> (starting_epoch, total_iterations).

    The file is first read with torch's weights-only unpickler (tensors, containers and the numpy scalar types the reference's
    checkpoints hold: `recall` is a numpy.float64, train_pointnetvlad.py:172-199).  Only if that refuses the file AND
    trust_checkpoint is set (the default: the reference's own torch.load executes whatever the pickle says) it is read with the
    full unpickler; pass trust_checkpoint=False for files of unknown origin."""
    target = _unwrap(model)
    try:
        allow = [np.dtype, np.float64, np.float32, np.int64]
        for name in ("scalar", "_reconstruct"):
            for mod in (getattr(np, "_core", None), getattr(np, "core", None)):
                fn = getattr(getattr(mod, "multiarray", None), name, None) if mod is not None else None
                if fn is not None:
                    allow.append(fn)
                    break
        allow += [type(np.dtype(t)) for t in ("float64", "float32", "int64")]
        with torch.serialization.safe_globals(allow):
            blob = torch.load(path, map_location=map_location, weights_only=True)
    except Exception:      # noqa: BLE001 -- anything the restricted unpickler does not accept
        if not trust_checkpoint:
            raise
        blob = torch.load(path, map_location=map_location, weights_only=False)
    if str(path)[-1] == "7":
        target.load_state_dict(_strip_module_prefix(blob), strict=False)
        return 0, 0
    target.load_state_dict(_strip_module_prefix(blob["state_dict"]), strict=True)
    if optimizer is not None:
        optimizer.load_state_dict(blob["optimizer"])
    return blob["epoch"] + 1, blob["iter"]


def update_vectors(model, clouds, batch_num, device=None):
    """util/data.py:277-354: re-embed the WHOLE training set with the current weights (eval mode, no grad) into the
    latent-vector table the hard-negative mining searches; train mode afterwards.  clouds [n, N, 3] (array-like, float64 or
    float32; the reference's TRAINING_POINT_CLOUD); batch_num = eval_batch_size * (1 + positives + negatives) clouds per
    forward (:291).  The reference runs the tail (n % batch_num clouds) one cloud per forward; eval-mode descriptors do not
    depend on the batch composition, so the tail is one forward here.  Returns the table as a CUDA tensor [n, D]: it stays on
    the device for get_hard_negatives_batched (the reference keeps a numpy array and rebuilds a KDTree per item)."""
    was_training = model.training
    model.eval()
    dev = next(model.parameters()).device if device is None else device
    clouds = np.asarray(clouds)
    outs = []
    try:
        pipe = BatchPipeline(model, PIPELINE_IN_FLIGHT if torch.device(dev).type == "cuda" else 1, torch.device(dev))
        for s in range(0, clouds.shape[0], batch_num):
            chunk = torch.from_numpy(np.ascontiguousarray(clouds[s:s + batch_num])).to(dev)
            outs.append(pipe.submit(chunk.float().unsqueeze(1)))
        pipe.join()
    finally:
        model.train()          # the reference leaves the model in train mode (:345)
    if not was_training:
        model.eval()
    return torch.cat(outs, dim=0) if outs else torch.zeros((0, 0), device=dev)


def get_hard_negatives_batched(query_vecs, random_negs, hard_neg_num, latent_vectors):
    """The selection step of util/data.py:103-115 for a whole batch of queries in ONE launch: query b (descriptor
    query_vecs[b]) has its own list random_negs[b] of sampled negatives (item numbers into the latent-vector table, all lists
    of one length, 4000 in the reference); returns for every query the hard_neg_num items nearest to it, nearest first, as a
    list of lists of item numbers.  latent_vectors: the table from update_vectors (CUDA tensor) or a numpy array."""
    from . import ops
    if isinstance(latent_vectors, torch.Tensor) and latent_vectors.is_cuda:
        table = latent_vectors
    else:
        table = torch.as_tensor(np.ascontiguousarray(latent_vectors), dtype=torch.float32,
                                device=torch.device("cuda", torch.cuda.current_device()))
    cand_np = np.asarray(random_negs, dtype=np.int32)
    if cand_np.ndim != 2:
        raise ValueError("get_hard_negatives_batched: random_negs must be [bq, n_sampled] (equal-length lists)")
    cand = torch.from_numpy(cand_np).to(table.device)
    q = torch.as_tensor(np.asarray(query_vecs.detach().cpu() if isinstance(query_vecs, torch.Tensor) else query_vecs, dtype=np.float32),
                        device=table.device).reshape(cand_np.shape[0], -1)
    pos, _ = ops.hard_negatives(table.float().contiguous(), q.contiguous(), cand, int(hard_neg_num))
    pos = pos.cpu().numpy()
    return [[int(cand_np[b, j]) for j in pos[b]] for b in range(cand_np.shape[0])]


def get_random_hard_negatives(query_vec, random_negs, hard_neg_num, latent_vectors):
    """util/data.py:103-115: among the training items `random_negs` (indices into the latent-vector table), the
    `hard_neg_num` whose descriptors are nearest to `query_vec`, nearest first, as a list of item indices.
    latent_vectors: the table of all training descriptors (the reference's global TRAINING_LATENT_VECTORS), a numpy array
    or -- to keep it resident between calls -- a CUDA tensor [n_items, D]."""
    from . import ops
    if isinstance(latent_vectors, torch.Tensor) and latent_vectors.is_cuda:
        table = latent_vectors
    else:
        table = torch.as_tensor(np.ascontiguousarray(latent_vectors), dtype=torch.float32,
                                device=torch.device("cuda", torch.cuda.current_device()))
    cand = torch.as_tensor(np.asarray(random_negs, dtype=np.int64), device=table.device)
    D = table.index_select(0, cand).contiguous()
    q = torch.as_tensor(np.asarray(query_vec, dtype=np.float32), device=table.device).reshape(1, -1)
    idx, _ = ops.retrieval_topk(q, D, int(hard_neg_num))
    return [int(random_negs[j]) for j in idx[0].cpu().tolist()]
