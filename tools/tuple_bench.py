"""Timing of the device-resident training tuples (csrc/lpd_tuples.hip, lpdnet_hip/tuples.py) at the Oxford run size: T = 21711 items
of N = 4096 points, bq = 2 queries per step, P = 2, Ng = 18 (44 clouds), n_sampled = 4000 mining candidates.

  (a) the two launches by HIP events: lpd_sample_items at the shapes TupleBank uses (negatives, other, 4000 candidates) and
      lpd_gather_tuples for the 44 clouds (plain copy, rotation + jitter); then the whole bank.sample / bank.assemble calls;
  (b) the host recipe they replace, as the reference's Dataset.__getitem__ does it (util/data.py:56-101), written here in numpy /
      Python: shuffle of the ~21 k-entry negatives list, the set difference over all keys for `other`, float64 fancy index of the
      22 clouds, cast, cat, host-to-device copy.  Wall time per step (bq queries);
  (c) harness.train_step fed by (b) against harness.train_step_from_bank: wall time per step, median over the steps after warm-up.

    python tools/tuple_bench.py [--items 21711] [--num-points 4096] [--steps 20] [--warmup 5] [--out profiles/tuple_bench.txt]

Synthetic bank: items on a line 1 m apart, positives within 10 m, near = within 300 m (about 21.1 k negatives per query), random
clouds.  (a) is device time between two HIP events around `iters` back-to-back calls divided by `iters` (launch gaps included);
(b) and (c) are host wall time with a device synchronisation at the end of every step.  Needs a GPU.
"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _events(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def _wall(fn, steps, warmup):
    """median and minimum wall time of fn(step) over `steps` steps after `warmup`, synchronised after every step"""
    t = []
    for s in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(s)
        torch.cuda.synchronize()
        if s >= warmup:
            t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t))


def host_tuple(q, entry, positives_of, keys, clouds, P, Ng):
    """the reference's get_query_tuple_fast (util/data.py:56-101) with other_neg=True and no hard negatives"""
    query = clouds[q]
    random.shuffle(entry["positives"])
    pos = clouds[entry["positives"][:P]]
    random.shuffle(entry["negatives"])
    neg_indices = entry["negatives"][:Ng]
    neg = clouds[neg_indices]
    neighbors = list(entry["positives"])
    for n in neg_indices:
        neighbors.extend(positives_of[n])
    possible = list(keys - set(neighbors))
    random.shuffle(possible)
    other = clouds[possible[0]]
    f = lambda a: torch.from_numpy(np.asarray(a)).float()      # noqa: E731
    return f(query)[None], f(pos), f(neg), f(other)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=21711)
    ap.add_argument("--num-points", type=int, default=4096)
    ap.add_argument("--bq", type=int, default=2)
    ap.add_argument("--positives", type=int, default=2)
    ap.add_argument("--negatives", type=int, default=18)
    ap.add_argument("--n-sampled", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tuple_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import harness, ops, tuples
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad

    dev = torch.device("cuda:0")
    T, N, bq, P, Ng = a.items, a.num_points, a.bq, a.positives, a.negatives
    B = bq * (2 + P + Ng)
    lines = [f"tuple_bench: T={T} N={N} bq={bq} P={P} Ng={Ng} n_sampled={a.n_sampled} on {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    clouds = rng.random((T, N, 3)) * 2.0 - 1.0      # float64, as TRAINING_POINT_CLOUD
    positives = [[int(j) for j in range(max(0, i - 10), min(T, i + 11)) if j != i] for i in range(T)]
    near = [np.arange(max(0, i - 300), min(T, i + 301)) for i in range(T)]
    t0 = time.perf_counter()
    bank = tuples.TupleBank(clouds, positives, near, device=dev)
    torch.cuda.synchronize()
    say(f"bank: {T} clouds uploaded and narrowed in {time.perf_counter() - t0:.2f} s; table {bank.table.numel() * 4 / 1e9:.2f} GB, "
        f"max|positives| {bank.max_pos}, max|near| {bank.max_near}")
    queries = [int(v) for v in rng.integers(0, T, size=64)]
    step_queries = lambda s: [queries[(s * bq + b) % len(queries)] for b in range(bq)]      # noqa: E731

    # ---- (a) the launches
    q_dev = torch.tensor(step_queries(0), dtype=torch.int32, device=dev).view(-1, 1)
    items = bank.sample(step_queries(0), P, Ng, seed=0)
    members = torch.cat((items[:, :1], items[:, 1 + P:1 + P + Ng]), 1).contiguous()      # the query and its negatives: the lists of `other`
    flat = items.reshape(-1).contiguous()
    out = torch.empty((B, 1, N, 3), device=dev)
    rot = torch.from_numpy(tuples.TupleBank.rotations(B, 0)).to(dev)
    t = _events(lambda: ops.sample_items(bank.near_off, bank.near_idx, T, q_dev, None, Ng, 1, 1), a.iters)
    say(f"(a) lpd_sample_items  negatives   R={bq} m={Ng} L=1 invert=1          {t * 1e6:8.1f} us")
    t = _events(lambda: ops.sample_items(bank.pos_off, bank.pos_idx, T, members, None, 1, 1, 2), a.iters)
    say(f"(a) lpd_sample_items  other       R={bq} m=1 L={1 + Ng} invert=1          {t * 1e6:8.1f} us")
    t = _events(lambda: ops.sample_items(bank.near_off, bank.near_idx, T, q_dev, None, a.n_sampled, 1, 3), a.iters)
    say(f"(a) lpd_sample_items  candidates  R={bq} m={a.n_sampled} L=1 invert=1        {t * 1e6:8.1f} us")
    t_copy = _events(lambda: ops.gather_tuples(bank.table, flat, out=out), a.iters)
    mb = B * N * 12 / 1e6
    say(f"(a) lpd_gather_tuples copy        B={B}                              {t_copy * 1e6:8.1f} us   ({mb:.2f} MB in, {mb:.2f} MB out: "
        f"{2 * mb / 1e3 / t_copy / 1e3:.2f} TB/s)")
    t_aug = _events(lambda: ops.gather_tuples(bank.table, flat, rot, 0.005, 0.05, 7, out=out), a.iters)
    say(f"(a) lpd_gather_tuples rotation + jitter                             {t_aug * 1e6:8.1f} us")
    ts, _ = _wall(lambda s: bank.sample(step_queries(s), P, Ng, seed=s), a.iters, 10)
    ta, _ = _wall(lambda s: bank.assemble(items, rotate=True, jitter=True, seed=s), a.iters, 10)
    say(f"(a) bank.sample (three draws) wall, synchronised                    {ts * 1e6:8.1f} us;  bank.assemble (rotate, jitter) {ta * 1e6:.1f} us")

    # ---- (b) the host recipe
    keys = set(range(T))
    entries = {q: {"positives": list(positives[q]), "negatives": [int(j) for j in range(T) if abs(j - q) > 300]} for q in set(queries)}
    random.seed(3)
    host = {}

    def host_step(s):
        parts = [host_tuple(q, entries[q], positives, keys, clouds, P, Ng) for q in step_queries(s)]
        batch = [torch.stack([p[i] for p in parts], 0) for i in range(4)]      # the DataLoader's collate
        host["batch"] = batch
        feed = torch.cat(batch, 1).reshape(-1, 1, N, 3)
        host["feed"] = feed.to(dev)

    tb, tb_min = _wall(host_step, a.steps, a.warmup)
    say(f"(b) host recipe (shuffles, set difference, float64 index, cast, cat, H2D), {bq} queries: median {tb * 1e3:7.2f} ms  min {tb_min * 1e3:.2f} ms")

    # ---- (c) train steps
    def fresh():
        torch.manual_seed(0)
        m = PointNetVlad(num_points=N, featnet="lpdnet")
        m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
        m = m.to(dev)
        return m, torch.optim.Adam(m.parameters(), lr=1e-5)

    m, opt = fresh()

    def step_host(s):
        host_step(s)
        harness.train_step(m, opt, *host["batch"])

    th, th_min = _wall(step_host, a.steps, a.warmup)
    m, opt = fresh()

    def step_resident(s):
        harness.train_step(m, opt, *[t_.to(dev) for t_ in host["batch"]])

    host_step(0)
    tr, tr_min = _wall(step_resident, a.steps, a.warmup)
    m, opt = fresh()
    tk, tk_min = _wall(lambda s: harness.train_step_from_bank(m, opt, bank, step_queries(s), P, Ng, seed=s), a.steps, a.warmup)
    m, opt = fresh()
    tg, tg_min = _wall(lambda s: harness.train_step_from_bank(m, opt, bank, step_queries(s), P, Ng, seed=s, rotate=True, jitter=True),
                       a.steps, a.warmup)
    say(f"(c) train_step fed by (b)                          median {th * 1e3:7.2f} ms  min {th_min * 1e3:.2f} ms   ({a.steps} steps after {a.warmup})")
    say(f"(c) train_step on one prepared host batch (no recipe) median {tr * 1e3:7.2f} ms  min {tr_min * 1e3:.2f} ms")
    say(f"(c) train_step_from_bank                           median {tk * 1e3:7.2f} ms  min {tk_min * 1e3:.2f} ms   ({th / tk:.2f} x)")
    say(f"(c) train_step_from_bank, rotate + jitter          median {tg * 1e3:7.2f} ms  min {tg_min * 1e3:.2f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
