"""Timing of the geometric verification (csrc/lpd_align.hip, lpdnet_hip/verify.py) at the sizes a user runs: N = 4096 points a cloud,
the default verify.AlignSearch (coarse: 120 yaws x 17 x 17 shifts of 0.5 m cells; fine: 17 yaws x 9 x 9 shifts of 0.25 m cells, four
height layers), P = 1 pair, 25 (one query's candidates) and 800 (32 queries x 25).

  (a) the coarse launch and the fine launch of lpd_align_pairs, and verify.align_pairs end to end (both launches and the torch
      operations between them): the median of `--iters` HIP-event intervals, one around every call, after a warm-up;
  (b) one plain-torch rung on the same inputs: the clouds rasterised into dense [layers, 128, 128] occupancy images per yaw
      (torch.floor + index_put_) and the (2S+1)^2 scores of every yaw as ONE conv2d of the zero-padded image of B with the images of A
      as the filters; its scores must equal the kernel's (the same winner) before anything is printed.  P = 1 and 25 only;
  (c) the 32-cloud eval forward of LPD-Net in the same run, the yardstick: what share of it a query's 25 verifications cost.

    python tools/align_bench.py [--iters 30] [--out profiles/align_bench.txt]

Every step runs in a child process of its own with a time limit, one at a time; the tool stops at the first step that fails.  The
clouds are the labelled street scenes of tests/align_ref.py (fixed seeds).  Needs a GPU.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = (("pairs:1", 300), ("pairs:25", 300), ("pairs:800", 420), ("forward", 300))
N, QUERIES, CANDIDATES, DATABASE = 4096, 32, 25, 64


def _median_events(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e-3 for a, b in ev)
    return t[len(t) // 2], t[0]


def tables():
    """32 query clouds, 64 database clouds (the first 32 are revisits of the queries' places, the others are other places), and the
    pairs: query i against its revisit and 24 other database rows"""
    import numpy as np
    import align_ref as R
    g = np.random.default_rng(7)
    A, B = [], []
    for i in range(QUERIES):
        a, b, _, _ = R.true_pair(100 + i)
        A.append(a), B.append(b)
    for i in range(DATABASE - QUERIES):
        B.append(R.false_pair(200 + i)[0])
    pairs = []
    for i in range(QUERIES):
        others = [int(v) for v in g.permutation(DATABASE) if v != i][:CANDIDATES - 1]
        pairs += [(i, c) for c in [i] + others]
    return np.stack(A), np.stack(B), np.array(pairs, dtype=np.int32)


def torch_rung(a, b, rot, inv_cell, S, z0, inv_zcell, layers):
    """scores [H, 2S+1, 2S+1] of ONE pair by dense images and conv2d; a, b [N, 3] on the device"""
    import torch
    import torch.nn.functional as F

    def image(p, cs):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        if cs is not None:
            c, s = cs[:, 0:1], cs[:, 1:2]
            x, y = x[None] * c - y[None] * s, x[None] * s + y[None] * c      # [H, N]
            z = z[None].expand_as(x)
        else:
            x, y, z = x[None], y[None], z[None]
        fx, fy, fz = torch.floor(x * inv_cell) + 64.0, torch.floor(y * inv_cell) + 64.0, torch.floor((z - z0) * inv_zcell)
        ok = (fx >= 0) & (fx < 128) & (fy >= 0) & (fy < 128) & (fz >= 0) & (fz < layers)
        img = torch.zeros((x.shape[0], layers, 128, 128), dtype=torch.float32, device=p.device)
        h = torch.arange(x.shape[0], device=p.device)[:, None].expand_as(x)
        img[h[ok], fz[ok].long(), fy[ok].long(), fx[ok].long()] = 1.0
        return img
    ia, ib = image(a, rot), image(b, None)
    return F.conv2d(F.pad(ib, (S, S, S, S)), ia)[0]      # [H, 2S+1 (dy), 2S+1 (dx)]


def step_pairs(P, iters):
    import numpy as np
    import torch
    from lpdnet_hip import ops, verify
    dev = torch.device("cuda:0")
    A, B, pairs = tables()
    a, b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    pr = torch.from_numpy(pairs[:P]).to(dev)
    s = verify.AlignSearch()
    H, R, Hf = s.yaw_steps, s.dense_steps, 2 * s.fine_div + 1
    rc, rd = s.coarse_table(dev), s.dense_table(dev)

    def coarse():
        return ops.align_pairs(a, b, pr, rc, H, 1.0 / s.cell, s.shifts, s.z_lo, 1.0 / s.z_cell, s.layers)
    best, _ = coarse()
    # the fine launch's arguments as verify.align_pairs makes them, restated here so that the launch can be timed alone; the
    # torch.equal check below holds the restatement to the chain itself
    first = torch.remainder(best[:, 0].long() * s.fine_div - s.fine_div, R).to(torch.int32)
    t0 = torch.stack((best[:, 2].float() * s.cell, best[:, 1].float() * s.cell), dim=1)

    def fine():
        return ops.align_pairs(a, b, pr, rd, Hf, 2.0 / s.cell, s.fine_shifts, s.z_lo, 1.0 / s.z_cell, s.layers, first=first, t0=t0,
                               want_yaw_scores=False)
    al = verify.align_pairs(a, b, pr, s)
    if not torch.equal(al.coarse, best) or not torch.equal(al.fine, fine()[0]):
        raise SystemExit("MISMATCH: verify.align_pairs and the two launches disagree")
    tc, tc_min = _median_events(coarse, iters)
    tf, tf_min = _median_events(fine, iters)
    te, te_min = _median_events(lambda: verify.align_pairs(a, b, pr, s), iters)
    ov = al.overlap.cpu().numpy()
    is_true = pairs[:P, 0] == pairs[:P, 1]
    print(f"P = {P:4d}  coarse launch (H = {H}, S = {s.shifts}) median {tc * 1e6:9.1f} us (min {tc_min * 1e6:.1f})   fine launch (H = {Hf}, S = "
          f"{s.fine_shifts}) {tf * 1e6:8.1f} us (min {tf_min * 1e6:.1f})   verify.align_pairs {te * 1e6:9.1f} us (min {te_min * 1e6:.1f})   "
          f"= {te / P * 1e6:.1f} us a pair")
    print(f"P = {P:4d}  overlap of the {int(is_true.sum())} revisits >= {ov[is_true].min():.3f}" +
          (f", of the {int((~is_true).sum())} other places <= {ov[~is_true].max():.3f}" if (~is_true).any() else ""))
    print(f"KV align{P} {te}")
    if P <= CANDIDATES:
        def rung():
            return [torch_rung(a[i], b[j], rc, 1.0 / s.cell, s.shifts, s.z_lo, 1.0 / s.z_cell, s.layers) for i, j in pairs[:P].tolist()]
        sc = torch.stack(rung()).cpu().numpy()      # [P, H, 17, 17]
        bh = best.cpu().numpy()
        for p in range(P):
            h, dy, dx, score = (int(v) for v in bh[p, :4])
            if int(np.rint(sc[p].max())) != score or int(np.rint(sc[p, h, dy + s.shifts, dx + s.shifts])) != score:
                raise SystemExit(f"MISMATCH at pair {p}: the torch rung's best score {sc[p].max()} / the kernel's {score}")
        tr, tr_min = _median_events(rung, max(3, iters // 5), warmup=1)
        print(f"P = {P:4d}  plain torch, coarse pass only (dense images + conv2d, the same scores)  median {tr * 1e6:9.1f} us (min {tr_min * 1e6:.1f})   "
              f"= {tr / tc:.1f} x the coarse launch")


def step_forward(iters):
    import torch
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad
    dev = torch.device("cuda:0")
    m = PointNetVlad(num_points=N, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
    m = m.to(dev).eval()
    x = torch.rand((QUERIES, 1, N, 3), generator=torch.Generator().manual_seed(1)).to(dev) * 2.0 - 1.0
    with torch.no_grad():
        t, t_min = _median_events(lambda: m(x), iters, warmup=5)
    print(f"eval forward of {QUERIES} clouds x {N} points (LPD-Net)                 median {t * 1e6:9.1f} us (min {t_min * 1e6:.1f})   "
          f"= {t / QUERIES * 1e6:.1f} us a cloud")
    print(f"KV forward {t}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("align_bench: needs a GPU (no CPU timing)")
        if a.step == "forward":
            step_forward(a.iters)
        else:
            step_pairs(int(a.step.split(":")[1]), a.iters)
        return
    lines = [f"align_bench: N = {N}, default AlignSearch; HIP-event medians of {a.iters} calls; one child process a step"]
    kv = {}
    print(lines[0], flush=True)
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"align_bench: step {step} exceeded its {limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"align_bench: step {step} failed (rc={r.returncode}); stopping\n{r.stdout}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("KV "):
                kv[line.split()[1]] = float(line.split()[2])
            elif line.strip():
                print(line, flush=True)
                lines.append(line)
    per_cloud = kv["forward"] / QUERIES
    tail = (f"one query: its forward {per_cloud * 1e6:.1f} us (1/{QUERIES} of the batch's), its {CANDIDATES} verifications {kv['align25'] * 1e6:.1f} us alone "
            f"= {kv['align25'] / per_cloud:.2f} x that; in a batch of {QUERIES} queries {kv['align800'] / QUERIES * 1e6:.1f} us a query = "
            f"{kv['align800'] / kv['forward']:.2f} x the {QUERIES}-cloud forward")
    print(tail, flush=True)
    lines.append(tail)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
