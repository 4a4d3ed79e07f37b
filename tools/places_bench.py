"""Timing of the place lists from positions (csrc/lpd_places.hip, lpdnet_hip/places.py) at the Oxford training-set size, T = 21711
synthetic route positions, against the host recipe they replace.

  (a) the two launches by HIP events: lpd_radius_count / lpd_radius_fill over all T x T pairs at r = 10 m and r = 50 m;
  (b) places.training_lists (both radii: four launches, two scans, the read-backs) -- wall time;
  (c) TupleBank.from_positions against TupleBank.from_queries_dict fed by the reference's recipe on the same positions
      (generate_training_tuples_baseline.py:52-67: sklearn KDTree, two query_radius searches, np.setdiff1d per item; then the bank's
      near_from_negatives and build_csr) -- wall time, the recipe's parts listed.  The recipe's `negatives` are kept as int32 numpy
      arrays here (about 1.9 GB at T = 21711); the reference turns them into Python lists and pickles them, which is not timed;
  (d) harness.evaluate_pairs with a places.TruthTable against the nested QUERY_SETS, at tools/recall_bench.py's run sizes (23 runs of
      2000 descriptors; every item of a run is a query, as there).  The nested structure is the TruthTable's own to_query_sets(), so
      both calls score the same lists; their results are compared before anything is printed.

    python tools/places_bench.py [--items 21711] [--iters 20] [--runs 23] [--per-run 2000] [--reps 5] [--out profiles/places_bench.txt]

Synthetic positions: a road driven in steps of `--step` +- 40 % metres with a slowly turning heading and driven back with 3 m of
lateral noise, at a UTM magnitude (northing 5.7e6).  (a) is device time between two HIP events around `iters` back-to-back launches
divided by `iters`; (b), (c), (d) are host wall time ending in a device synchronisation.  Needs a GPU.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ORIGIN = np.array([5.7e6, 6.2e5])


def road(n, seed, step):
    g = np.random.default_rng(seed)
    heading = np.cumsum(g.normal(0.0, 0.08, n))
    s = g.uniform(0.6 * step, 1.4 * step, n)
    return np.cumsum(np.stack((s * np.cos(heading), s * np.sin(heading)), 1), 0)


def route(T, seed, step):
    """a road of T / 2 steps and the way back with 3 m of noise: every place is visited twice"""
    half = (T + 1) // 2
    xy = road(half, seed, step)
    back = xy[::-1][:T - half] + np.random.default_rng(seed + 1).normal(0.0, 3.0, (T - half, 2))
    return np.concatenate((xy, back)) + ORIGIN


def _events(fn, iters, warmup=3):
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


def _wall(fn, reps, warmup=1):
    out, t = None, []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return out, float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=21711)
    ap.add_argument("--step", type=float, default=2.0, help="mean distance between consecutive training positions, metres")
    ap.add_argument("--num-points", type=int, default=64, help="points per cloud of the banks in (c): the table upload is common to both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=23)
    ap.add_argument("--per-run", type=int, default=2000)
    ap.add_argument("--run-step", type=float, default=20.0, help="mean distance between consecutive items of an evaluation run, metres")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--skip-recipe", action="store_true", help="leave the host recipe of (c) out (it holds about 2 GB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("places_bench: needs a GPU (no CPU timing)")
    import ctypes
    from lpdnet_hip import _lib, harness, ops, places, tuples

    dev = torch.device("cuda:0")
    T = a.items
    lines = [f"places_bench: T={T} route positions (step {a.step:g} m) on {torch.cuda.get_device_name(0)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pos = route(T, 1, a.step)
    dpos = torch.from_numpy(pos).to(dev)

    # ---- (a) the launches
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    seg = torch.tensor([0, T], dtype=torch.int32, device=dev)
    for r in (10.0, 50.0):
        off, idx, counts = ops.radius_lists(dpos, dpos, r)
        head = (p(dpos), T, p(dpos), T, p(seg), 1, r, None, None)
        tc = _events(lambda: lib.lpd_radius_count(*head, p(counts), ops._stream()), a.iters)
        tf = _events(lambda: lib.lpd_radius_fill(*head, p(off), p(idx), idx.numel(), ops._stream()), a.iters)
        say(f"(a) r = {r:4.0f} m  {idx.numel():9d} entries, longest row {int(counts.max()):4d}   lpd_radius_count {tc * 1e6:8.1f} us   "
            f"lpd_radius_fill {tf * 1e6:8.1f} us   ({T * T / tc / 1e9:.0f} G pairs/s in the count)")

    # ---- (b) the lists of a training set
    lists, tb, tb_min = _wall(lambda: places.training_lists(dpos), a.reps)
    say(f"(b) places.training_lists (r = 10 / 50 m), positions on the device    median {tb * 1e3:8.2f} ms  min {tb_min * 1e3:.2f} ms")
    _, tb, tb_min = _wall(lambda: places.training_lists(pos, device=dev), a.reps)
    say(f"(b) places.training_lists, positions on the host (one upload)         median {tb * 1e3:8.2f} ms  min {tb_min * 1e3:.2f} ms")

    # ---- (c) the bank
    clouds = np.random.default_rng(2).random((T, a.num_points, 3)).astype(np.float32)
    bank, tp, tp_min = _wall(lambda: tuples.TupleBank.from_positions(clouds, pos, device=dev), a.reps)
    say(f"(c) TupleBank.from_positions (N = {a.num_points}: lists + table upload)          median {tp * 1e3:8.2f} ms  min {tp_min * 1e3:.2f} ms")
    if a.skip_recipe:
        say("(c) host recipe: skipped (--skip-recipe)")
    else:
        from sklearn.neighbors import KDTree
        t0 = time.perf_counter()
        tree = KDTree(pos)
        ind_nn = tree.query_radius(pos, r=10)
        ind_r = tree.query_radius(pos, r=50)
        t1 = time.perf_counter()
        everyone = np.arange(T)
        queries = {}
        for i in range(T):
            queries[i] = {"query": i, "positives": np.setdiff1d(ind_nn[i], [i]), "negatives": np.setdiff1d(everyone, ind_r[i]).astype(np.int32)}
        t2 = time.perf_counter()
        old = tuples.TupleBank.from_queries_dict(queries, clouds, device=dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        same = all(torch.equal(getattr(bank, n), getattr(old, n)) for n in ("pos_off", "pos_idx", "near_off", "near_idx"))
        say(f"(c) host recipe: KDTree + two query_radius {t1 - t0:7.2f} s, setdiff1d x {2 * T} {t2 - t1:7.2f} s, TupleBank.from_queries_dict "
            f"(near_from_negatives, build_csr, uploads) {t3 - t2:7.2f} s: total {t3 - t0:7.2f} s   ({(t3 - t0) / tp:.0f} x from_positions)")
        say(f"(c) the two banks hold the same four CSR tensors: {same}")
        if not same:
            raise SystemExit("MISMATCH: from_positions and the host recipe disagree")
        del queries, old, ind_nn, ind_r, tree

    # ---- (d) the evaluation
    base = road(a.per_run, 7, a.run_step)
    runs = [base + np.random.default_rng(100 + m).normal(0.0, 3.0, base.shape) + ORIGIN for m in range(a.runs)]
    table, tt, tt_min = _wall(lambda: places.evaluation_truth(runs, runs, device=dev), a.reps)
    say(f"(d) places.evaluation_truth, {a.runs} runs x {a.per_run} items, r = 25 m: {table.truth_idx.numel()} entries      "
        f"median {tt * 1e3:8.2f} ms  min {tt_min * 1e3:.2f} ms")
    t0 = time.perf_counter()
    nested = table.to_query_sets()
    say(f"(d) TruthTable.to_query_sets (the nested layout, built once for this comparison)  {time.perf_counter() - t0:8.2f} s")
    g = torch.Generator(device=dev).manual_seed(3)
    vec = torch.nn.functional.normalize(torch.randn((a.runs * a.per_run, a.dim), device=dev, generator=g), dim=1)
    off = np.arange(a.runs + 1, dtype=np.int64) * a.per_run
    resident = (vec, off)
    got, tn, tn_min = _wall(lambda: harness.evaluate_pairs(resident, resident, table), a.reps)
    want, to, to_min = _wall(lambda: harness.evaluate_pairs(resident, resident, nested), a.reps)
    for k, ((gr, gs, go), (wr, ws, wo)) in enumerate(zip(got, want)):
        if not (np.array_equal(gr, wr) and gs == ws and go == wo):
            raise SystemExit(f"MISMATCH at pair {k}: TruthTable and nested QUERY_SETS give different results")
    say(f"(d) evaluate_pairs, nested QUERY_SETS ({len(want)} pairs)                     median {to * 1e3:8.2f} ms  min {to_min * 1e3:.2f} ms")
    say(f"(d) evaluate_pairs, TruthTable (identical results)                     median {tn * 1e3:8.2f} ms  min {tn_min * 1e3:.2f} ms   "
        f"({to / tn:.2f} x)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
