"""Timing of the sequence scoring of retrieved candidates (csrc/lpd_seqmatch.hip, lpdnet_hip/sequence.py) at the sizes a user runs: K =
25 candidates a query, the default sequence.SeqSearch (six velocities, five shifts, eleven terms), dim 256.

  (a) ops.seq_match at nq = nd = 400 (two 2 km drives cut every 5 m) and at nq = nd = 21711 (the Oxford table size, 45 runs), with the
      candidates of ops.retrieval_topk: the time of a call (two norm launches and the kernel), the time a candidate, the bytes of
      descriptor rows it stages a second, and the MFMA issue time of its 128 (dim 256) v_mfma_f32_32x32x2_f32 a candidate on the
      chip's 1024 SIMDs at 64 cycles each and 2.4 GHz -- an estimate, printed beside the measurement;
  (b) one plain-torch rung at n = 400: gather the bands, bmm, quantise, index sums, argmin; its winning rows must agree with the
      kernel's for 99 % of the valid candidates before anything is printed (cuBLAS-style products round differently: a near tie can
      fall the other way).  At n = 21711 the gathered bands alone are 17 GB: no rung there;
  (c) verify.align_pairs of 32 queries x 25 candidates (tools/align_bench.py's clouds) in the same run: the stage this one filters for;
  (d) the 32-cloud eval forward of LPD-Net, the yardstick.

    python tools/seq_bench.py [--iters 30] [--out profiles/seq_bench.txt]

Every step runs in a child process of its own with a time limit, one at a time; the tool stops at the first step that fails.  Needs a GPU.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = (("seq:400", 300), ("seq:21711", 420), ("align", 420), ("forward", 300))
K, DIM, QUERIES = 25, 256, 32
SIMDS, CLOCK, MFMA_CYCLES = 1024, 2.4e9, 64


def drive_tables(n, seed=0, noise=2.5):
    """Q, D [n, 256] fp32: two drives past the same n places (neighbouring places share three quarters of their latent), unit rows"""
    import numpy as np
    g = np.random.default_rng(seed)
    base = g.standard_normal((n + 3, DIM)).astype(np.float32)
    place = (base[:-3] + base[1:-2] + base[2:-1] + base[3:]) / 2.0

    def unit(x):
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return unit(place + noise * g.standard_normal((n, DIM)).astype(np.float32)), unit(place + noise * g.standard_normal((n, DIM)).astype(np.float32))


def torch_rung(q, d, cand, steps, S, min_terms):
    """the stage for ONE run a table in plain torch -> row [nq, K] of the best hypothesis, or -1"""
    import torch
    nq, nd, Kc = q.shape[0], d.shape[0], cand.shape[1]
    V, L = steps.shape
    h = (L - 1) // 2
    W = 2 * S + 1
    dev = q.device
    t = torch.arange(-h, h + 1, device=dev)
    ra = torch.arange(nq, device=dev)[:, None] + t[None, :]                                   # [nq, L]
    j = cand.long()
    rb = j[:, :, None] - 15 + torch.arange(31, device=dev)[None, None, :]                     # [nq, K, 31]
    oka, okb = (ra >= 0) & (ra < nq), (rb >= 0) & (rb < nd) & ((j >= 0) & (j < nd))[:, :, None]
    qb, db = q[ra.clamp(0, nq - 1)], d[rb.clamp(0, nd - 1)]                                  # [nq, L, dim], [nq, K, 31, dim]
    dots = torch.matmul(qb[:, None], db.transpose(2, 3))                                      # [nq, K, L, 31]
    d2 = ((qb * qb).sum(-1)[:, None, :, None] + (db * db).sum(-1)[:, :, None, :] - 2.0 * dots).clamp(min=0.0)
    dq = torch.round(d2.clamp(max=16.0) * 16384.0).to(torch.int64)
    ok = oka[:, None, :, None] & okb[:, :, None, :]
    e = torch.arange(V * W, device=dev)
    s = e % W - S
    bp = 15 + s[:, None] + steps.long()[e // W]                                               # [E, L]
    sel = dq[:, :, torch.arange(L, device=dev)[None, :], bp]                                  # [nq, K, E, L]
    cnt = ok[:, :, torch.arange(L, device=dev)[None, :], bp]
    total, n = (sel * cnt).sum(-1), cnt.sum(-1)
    c0 = j[:, :, None] + s[None, None, :]
    valid = (c0 >= 0) & (c0 < nd) & ((j >= 0) & (j < nd))[:, :, None] & (n >= min_terms)
    mean = torch.where(valid, total.double() / n.clamp(min=1).double(), torch.full((), float("inf"), dtype=torch.float64, device=dev))
    we = mean.argmin(-1)
    return torch.where(torch.gather(valid, 2, we[..., None])[..., 0], j + s[we], torch.full_like(j, -1))


def step_seq(n, iters):
    import numpy as np
    import torch
    from align_bench import _median_events
    from lpdnet_hip import ops, sequence
    dev = torch.device("cuda:0")
    Q, D = drive_tables(n)
    q, d = torch.from_numpy(Q).to(dev), torch.from_numpy(D).to(dev)
    s = sequence.SeqSearch()
    steps = s.steps_table()
    off = None if n <= 400 else np.append(np.arange(0, n, 483), n).astype(np.int32)
    cand, _ = ops.retrieval_topk(q, d, K)
    top1 = float((torch.abs(cand[:, 0].long() - torch.arange(n, device=dev)) <= 2).double().mean())
    m = sequence.match_sequences(q, d, cand, off, off, search=s)
    first = torch.gather(m.row, 1, m.order[:, :1])[:, 0].long()
    seq1 = float((torch.abs(first - torch.arange(n, device=dev)) <= 2).double().mean())
    t, t_min = _median_events(lambda: ops.seq_match(q, d, cand, steps, s.shifts, s.min_terms, q_off=off, d_off=off), iters)
    tw, tw_min = _median_events(lambda: sequence.match_sequences(q, d, cand, off, off, search=s), iters)
    tr, tr_min = _median_events(lambda: ops.retrieval_topk(q, d, K), max(3, iters // 3))
    C = n * K
    mfma = C * (DIM // 2) * MFMA_CYCLES / (SIMDS * CLOCK)
    staged = C * 31 * DIM * 4 + n * 4 * 31 * DIM * 4      # a candidate's band, and the query band once a wave
    runs = 1 if off is None else len(off) - 1
    print(f"n = {n:6d} ({runs} run{'s' if runs > 1 else ''}), {C} candidates: seq_match median {t * 1e6:9.1f} us (min {t_min * 1e6:.1f}) = {t / C * 1e9:7.1f} ns a "
          f"candidate, {staged / t / 1e9:7.1f} GB/s of descriptor rows staged; MFMA issue alone (estimate) {mfma * 1e6:.1f} us = {mfma / t:.2f} of it   "
          f"match_sequences {tw * 1e6:9.1f} us (min {tw_min * 1e6:.1f})   retrieval_topk {tr * 1e6:9.1f} us (min {tr_min * 1e6:.1f})")
    print(f"n = {n:6d}  rows within 2 of the truth: single-frame top-1 {top1:.3f}, first sequence candidate after its shift {seq1:.3f}")
    print(f"KV seq{n} {t}")
    if n <= 400:
        st = torch.from_numpy(steps).to(dev)
        got = torch_rung(q, d, cand, st, s.shifts, s.min_terms)
        valid = m.valid
        agree = float((got == m.row)[valid].double().mean())
        if not agree >= 0.99:
            raise SystemExit(f"MISMATCH: the torch rung's rows agree with the kernel's for {agree:.4f} of the valid candidates")
        tt, tt_min = _median_events(lambda: torch_rung(q, d, cand, st, s.shifts, s.min_terms), max(3, iters // 3), warmup=1)
        print(f"n = {n:6d}  plain torch (gather the bands, matmul, quantise, index sums, argmin; rows agree for {agree:.4f} of the valid candidates) median "
              f"{tt * 1e6:9.1f} us (min {tt_min * 1e6:.1f}) = {tt / t:.1f} x seq_match")


def step_align(iters):
    import torch
    from align_bench import CANDIDATES, _median_events, tables
    from lpdnet_hip import verify
    dev = torch.device("cuda:0")
    A, B, pairs = tables()
    a, b, pr = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(pairs).to(dev)
    P = pr.shape[0]
    assert CANDIDATES == K
    t, t_min = _median_events(lambda: verify.align_pairs(a, b, pr), iters)
    print(f"align_pairs of {QUERIES} queries x {K} candidates, 4096 points a cloud: median {t * 1e6:9.1f} us (min {t_min * 1e6:.1f}) = {t / P * 1e6:.2f} us a pair")
    print(f"KV align {t / P}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("seq_bench: needs a GPU (no CPU timing)")
        if a.step == "forward":
            from align_bench import step_forward
            step_forward(a.iters)
        elif a.step == "align":
            step_align(a.iters)
        else:
            step_seq(int(a.step.split(":")[1]), a.iters)
        return
    lines = [f"seq_bench: K = {K} candidates a query, dim {DIM}, default SeqSearch (6 velocities x 5 shifts, 11 terms); HIP-event medians of {a.iters} calls; "
             "one child process a step"]
    kv = {}
    print(lines[0], flush=True)
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"seq_bench: step {step} exceeded its {limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"seq_bench: step {step} failed (rc={r.returncode}); stopping\n{r.stdout}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("KV "):
                kv[line.split()[1]] = float(line.split()[2])
            elif line.strip():
                print(line, flush=True)
                lines.append(line)
    per_cloud = kv["forward"] / QUERIES
    c400, c21711 = kv["seq400"] / (400 * K), kv["seq21711"] / (21711 * K)
    tail = (f"a candidate: sequence scoring {c400 * 1e9:.1f} ns (n = 400) / {c21711 * 1e9:.1f} ns (n = 21711), align_pairs {kv['align'] * 1e6:.2f} us = "
            f"{kv['align'] / c400:.0f} x / {kv['align'] / c21711:.0f} x; one query: its forward {per_cloud * 1e6:.1f} us (1/{QUERIES} of the batch's), the scoring of its "
            f"{K} candidates {c21711 * K * 1e6:.2f} us = {c21711 * K / per_cloud:.3f} x that, their alignments {kv['align'] * K * 1e6:.1f} us = "
            f"{kv['align'] * K / per_cloud:.2f} x")
    print(tail, flush=True)
    lines.append(tail)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
