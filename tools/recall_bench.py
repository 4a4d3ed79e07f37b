"""Timing of the recall evaluation (evaluate.py:33-93) on synthetic descriptor runs: the per-pair get_recall loop the reference's
evaluate_model runs (one KDTree -> one retrieval_topk launch per (database run, query run) pair) against harness.evaluate_pairs
on resident tables (ONE lpd_recall_pairs launch for all pairs).

    python tools/recall_bench.py [--runs 23] [--per-run 2000] [--reps 5]
    python tools/recall_bench.py --kernel-only            # what a `rocprofv3 --kernel-trace --stats` run profiles
    python tools/recall_bench.py --kernel-stats <dir or kernel_stats.csv of that run>   # adds the kernel's FLOP/s and share of peak

Defaults: 23 runs as in the reference's Oxford evaluation split; 2000 descriptors per run (database and query runs are the same
descriptors, as synthetic_runs builds them) is an ASSUMPTION about the run sizes, not a measured property of the dataset.  Both
paths are timed with a host clock around work that ends in torch.cuda.synchronize(), after warm-up calls; their results are compared
(curves, one-percent recall exactly, similarities to 1e-6) before anything is printed.
"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F32_MFMA_PEAK = 157.3e12      # MI355X peak FP32 matrix rate (v_mfma_f32_32x32x2_f32), MI355X_MICROARCH.md


def _timed(fn, reps):
    torch.cuda.synchronize()
    best, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    return out, best


def _kernel_stats(path):
    files = [path] if path.endswith(".csv") else glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {path}")
    for r in csv.DictReader(open(files[0])):
        if "recall_pairs_kernel" in r["Name"]:
            return int(r["Calls"]), float(r["AverageNs"]) * 1e-9, float(r["MinNs"]) * 1e-9
    raise SystemExit(f"recall_pairs_kernel not in {files[0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=23)
    ap.add_argument("--per-run", type=int, default=2000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recall_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import harness
    from oracle import retrieval_oracle as ro

    t0 = time.perf_counter()
    vecs, _, qsets = ro.synthetic_runs(seed=a.seed, runs=a.runs, per_run=(a.per_run,) * a.runs, dim=a.dim)
    print(f"synthetic runs: {a.runs} x {a.per_run} descriptors of {a.dim} (built in {time.perf_counter() - t0:.1f} s)", flush=True)
    dev = torch.device("cuda:0")
    off = np.zeros(a.runs + 1, np.int64)
    np.cumsum([len(v) for v in vecs], out=off[1:])
    resident = (torch.from_numpy(np.concatenate(vecs)).to(dev), off)
    pairs = harness.all_pairs(a.runs)
    flops = 2.0 * a.dim * sum(len(vecs[n]) * len(vecs[m]) for m, n in pairs)

    fused = lambda: harness.evaluate_pairs(resident, resident, qsets)                                        # noqa: E731
    loop = lambda: [harness.get_recall(int(m), int(n), vecs, vecs, qsets) for m, n in pairs]                  # noqa: E731
    if a.kernel_only:
        _timed(fused, 1 + a.reps)
        print(f"kernel-only: {1 + a.reps} evaluate_pairs calls, {len(pairs)} pairs each, {flops / 1e12:.3f} TFLOP each")
        return

    _timed(fused, 2)                      # warm-up: code objects, allocator
    _timed(loop, 1)
    got, t_fused = _timed(fused, a.reps)
    want, t_loop = _timed(loop, a.loop_reps)
    for p, ((gr, gs, go), (wr, ws, wo)) in enumerate(zip(got, want)):
        if not (np.array_equal(gr, wr) and go == wo and len(gs) == len(ws) and np.allclose(gs, ws, atol=1e-6)):
            raise SystemExit(f"MISMATCH at pair {p} {tuple(pairs[p])}: fused and per-pair results differ")
    print(f"agreement: {len(pairs)} pairs, recall curves and one-percent recall identical, top-1 similarities within 1e-6")
    print(f"(a) per-pair get_recall loop : {len(pairs)} pairs  min {min(t_loop) * 1e3:9.1f} ms  median {np.median(t_loop) * 1e3:9.1f} ms"
          f"  ({a.loop_reps} reps)")
    print(f"(b) evaluate_pairs, resident : one launch   min {min(t_fused) * 1e3:9.1f} ms  median {np.median(t_fused) * 1e3:9.1f} ms"
          f"  ({a.reps} reps)")
    print(f"speed-up (medians): {np.median(t_loop) / np.median(t_fused):.1f}x")
    print(f"work: 2 * dim * sum Nq * Ndb = {flops / 1e12:.3f} TFLOP per evaluation")
    if a.kernel_stats:
        calls, avg, mn = _kernel_stats(a.kernel_stats)
        print(f"recall_pairs_kernel (rocprofv3 --kernel-trace --stats, {calls} calls): avg {avg * 1e3:.3f} ms, min {mn * 1e3:.3f} ms")
        print(f"achieved: {flops / avg / 1e12:.1f} TFLOP/s at the average = {flops / avg / F32_MFMA_PEAK * 100:.1f} % of the "
              f"{F32_MFMA_PEAK / 1e12:.1f} TFLOP/s f32 MFMA peak (compute-bound: the tables are {resident[0].numel() * 4 / 1e6:.0f} MB)")


if __name__ == "__main__":
    main()
