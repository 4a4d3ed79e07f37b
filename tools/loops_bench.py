"""Timing of the consistent-loop selection (csrc/lpd_loops.hip, lpdnet_hip/consistency.py) at the sizes a user runs.

  (a) one drive with P = 256, 1024 and 4096 loops (tests/loops_ref.drive_loops, three loops in ten grossly wrong): lpd_loop_consistency
      and lpd_loop_select (both of its launches) through their wrappers; beside them the numpy restatement on the host, whose result the
      device's must equal in every bit before anything is printed; a plain-torch rung on the device (batched float64 4 x 4 products over
      [P, P], then bit packing); and lpd_pgo_solve of the same graph with every loop under huber = 3;
  (b) 45 drives of 200 loops in one launch of each kernel.

    python tools/loops_bench.py [--iters 20] [--out profiles/loops_bench.txt]

Every step runs in a child process of its own with a time limit, one at a time; the tool stops at the first step that fails.
HIP-event medians after a warm-up.  Needs a GPU.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = (("p256", 240), ("p1024", 300), ("p4096", 540), ("batch", 300))
SIZES = {"p256": (200, 256), "p1024": (800, 1024), "p4096": (3200, 4096)}      # nodes, loops
BATCH, BATCH_NODES, BATCH_LOOPS = 45, 200, 200
SOLVER = dict(outer=20, cg_iters=500, cg_tol=1e-6, lambda0=1e-4, huber=3.0)


def _up(dev, arrays):
    import numpy as np
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _torch_rung(pose, edge, meas, weight, w_or, w_ot, gate):
    """The same decision in plain torch on the device, not bit-exact: E = (Z_a X_ja^-1) (X_jb Z_b^-1 X_ib^-1) X_ia as batched 4 x 4 float64
    products over [P, P]; |r_rot|^2 = 4 (1 - q_w^2) = 3 - trace; the variances by broadcasting; 64 columns packed into a word by shifts."""
    import torch
    P = edge.shape[0]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=pose.device)

    def m4(x):
        return torch.cat((x.reshape(-1, 3, 4), bottom.expand(x.shape[0], 1, 4)), dim=1)
    i, j = edge[:, 0].long(), edge[:, 1].long()
    Xi, Xj, Z = m4(pose[i]), m4(pose[j]), m4(meas)
    A = Z @ torch.linalg.inv(Xj)
    B = Xj @ torch.linalg.inv(Z) @ torch.linalg.inv(Xi)
    E = (A[:, None] @ B[None]) @ Xi[:, None]
    rr = 3.0 - (E[..., 0, 0] + E[..., 1, 1] + E[..., 2, 2])
    tt = (E[..., :3, 3] ** 2).sum(-1)
    ni, nj = (i[:, None] - i[None]).abs().double(), (j[:, None] - j[None]).abs().double()
    ci2 = ((pose[i][:, None, 3::4] - pose[i][None, :, 3::4]) ** 2).sum(-1)
    cj2 = ((pose[j][:, None, 3::4] - pose[j][None, :, 3::4]) ** 2).sum(-1)
    var_r = 1.0 / weight[:, None, 0] + 1.0 / weight[None, :, 0] + (ni + nj) / w_or
    var_t = 1.0 / weight[:, None, 1] + 1.0 / weight[None, :, 1] + (ni + nj) / w_ot + (ni * ci2 + nj * cj2) / w_or
    M = torch.triu(rr / var_r + tt / var_t <= gate, 1)      # the decision of (a, b) is that of (min, max): the upper triangle, mirrored
    M = M | M.T
    nw = (P + 63) // 64
    bits = torch.zeros((P, nw * 64), dtype=torch.int64, device=pose.device)
    bits[:, :P] = M
    return (bits.reshape(P, nw, 64) << torch.arange(64, device=pose.device)).sum(-1), M


def step_size(name, iters):
    import numpy as np
    import torch
    import loops_ref as L
    import pgo_ref  # noqa: F401
    from align_bench import _median_events
    from lpdnet_hip import ops, posegraph
    dev = torch.device("cuda:0")
    V, P = SIZES[name]
    start, edge, meas, weight, (w_or, w_ot) = L.drive_loops(P, V, P)
    args = _up(dev, (start, edge, meas, weight))
    t0 = time.perf_counter()
    ref = L.consistency(start, edge, meas, weight, w_or, w_ot, L.GATE)
    t_cons = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref += L.select(ref[0], ref[1], seeds=L.SEEDS, min_size=L.MIN_SIZE)
    t_sel = time.perf_counter() - t0
    adj, degree = ops.loop_consistency(*args, w_or, w_ot, L.GATE)
    accepted, info = ops.loop_select(adj, degree, seeds=L.SEEDS, min_size=L.MIN_SIZE)
    got = (adj.cpu().numpy().view(np.uint64), degree.cpu().numpy(), accepted.cpu().numpy(), info.cpu().numpy())
    if not all(a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, ref)):
        raise SystemExit("MISMATCH: the device's selection differs from the restatement's")
    tc, tc_min = _median_events(lambda: ops.loop_consistency(*args, w_or, w_ot, L.GATE), iters)
    ts, ts_min = _median_events(lambda: ops.loop_select(adj, degree, seeds=L.SEEDS, min_size=L.MIN_SIZE), iters)
    ts64, _ = _median_events(lambda: ops.loop_select(adj, degree, seeds=64, min_size=L.MIN_SIZE), iters)
    words, M = _torch_rung(*args, w_or, w_ot, L.GATE)
    agree = float((M == torch.from_numpy(L.unpack(got[0], P)).to(dev)).double().mean())
    tt, tt_min = _median_events(lambda: _torch_rung(*args, w_or, w_ot, L.GATE), max(3, iters // 4), warmup=1)
    od = posegraph.odometry_edges(args[0], None, w_or, w_ot)
    e, m, w = (torch.cat((a, b)) for a, b in zip(od, args[1:]))
    tp, _ = _median_events(lambda: ops.pgo_solve(args[0], e, m, w, **SOLVER), max(3, iters // 4), warmup=1)
    i = got[3][0]
    pairs = P * (P - 1) // 2
    print(f"P = {P} loops on {V} nodes: {i[1]} valid, {i[5]} of {pairs} pairs consistent, {i[2]} chosen from {i[3]} seeds (status {i[0]}), bits equal to the "
          f"restatement")
    print(f"P = {P}: lpd_loop_consistency median {tc * 1e6:9.1f} us (min {tc_min * 1e6:.1f}) = {tc / (P * P) * 1e9:.2f} ns a pair statistic of the P^2 evaluated; "
          f"lpd_loop_select (8 seeds, both launches) {ts * 1e6:9.1f} us (min {ts_min * 1e6:.1f}), with 64 seeds {ts64 * 1e6:9.1f} us; on the host: restated "
          f"consistency {t_cons:.2f} s = {t_cons / tc:.0f} x, restated selection {t_sel:.3f} s = {t_sel / ts:.0f} x; plain torch on the device {tt * 1e6:9.1f} us "
          f"(min {tt_min * 1e6:.1f}) = {tt / tc:.1f} x the kernel, {agree * 100:.4f} % of its bits the kernel's; lpd_pgo_solve of the same graph, every loop, "
          f"huber = 3: {tp * 1e6:9.1f} us = {tp / (tc + ts):.1f} x the selection")
    print(f"KV {name} {tc} {ts}")


def step_batch(iters):
    import numpy as np
    import torch
    import loops_ref as L
    from align_bench import _median_events
    from lpdnet_hip import ops
    dev = torch.device("cuda:0")
    gs = [L.drive_loops(100 + b, BATCH_NODES, BATCH_LOOPS) for b in range(BATCH)]
    cat = [np.concatenate([g[k] for g in gs]) for k in range(4)]
    args = _up(dev, cat)
    w_or, w_ot = gs[0][4]
    node_off, loop_off = [b * BATCH_NODES for b in range(BATCH + 1)], [b * BATCH_LOOPS for b in range(BATCH + 1)]
    ref = L.consistency(*cat, w_or, w_ot, L.GATE, node_off=node_off, loop_off=loop_off)
    ref += L.select(ref[0], ref[1], loop_off=loop_off, seeds=L.SEEDS, min_size=L.MIN_SIZE)
    noff, loff = torch.tensor(node_off, dtype=torch.int32, device=dev), torch.tensor(loop_off, dtype=torch.int32, device=dev)
    ldw = (BATCH_LOOPS + 63) // 64
    adj, degree = ops.loop_consistency(*args, w_or, w_ot, L.GATE, node_off=noff, loop_off=loff, ldw=ldw)
    accepted, info = ops.loop_select(adj, degree, loop_off=loff, seeds=L.SEEDS, min_size=L.MIN_SIZE)
    got = (adj.cpu().numpy().view(np.uint64), degree.cpu().numpy(), accepted.cpu().numpy(), info.cpu().numpy())
    if not all(a.tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(got, ref)):
        raise SystemExit("MISMATCH: the device's selection differs from the restatement's")
    tc, tc_min = _median_events(lambda: ops.loop_consistency(*args, w_or, w_ot, L.GATE, node_off=noff, loop_off=loff, ldw=ldw), iters)
    ts, ts_min = _median_events(lambda: ops.loop_select(adj, degree, loop_off=loff, seeds=L.SEEDS, min_size=L.MIN_SIZE), iters)
    print(f"{BATCH} drives of {BATCH_LOOPS} loops in one launch: lpd_loop_consistency median {tc * 1e6:9.1f} us (min {tc_min * 1e6:.1f}), lpd_loop_select "
          f"({BATCH} x 8 workgroups, then {BATCH}) {ts * 1e6:9.1f} us (min {ts_min * 1e6:.1f}) = {(tc + ts) / BATCH * 1e6:.1f} us a drive; chosen "
          f"{int(got[3][:, 2].min())} .. {int(got[3][:, 2].max())} loops, statuses {sorted(set(got[3][:, 0].tolist()))}, bits equal to the restatement")
    print(f"KV batch {tc} {ts}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("loops_bench: needs a GPU (no CPU timing)")
        step_batch(a.iters) if a.step == "batch" else step_size(a.step, a.iters)
        return
    lines = [f"loops_bench: drives with three gross loops in ten (tests/loops_ref.drive_loops), gate {16.81}, 8 seeds; HIP-event medians of {a.iters} calls; one "
             "child process a step"]
    print(lines[0], flush=True)
    kv = {}
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"loops_bench: step {step} exceeded its {limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"loops_bench: step {step} failed (rc={r.returncode}); stopping\n{r.stdout}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("KV "):
                kv[line.split()[1]] = (float(line.split()[2]), float(line.split()[3]))
            elif line.strip():
                print(line, flush=True)
                lines.append(line)
    one = sum(kv["p256"])
    tail = (f"a drive of 256 loops alone {one * 1e6:.1f} us; 45 drives of 200 in one launch {sum(kv['batch']) / BATCH * 1e6:.1f} us each; 4096 loops "
            f"{sum(kv['p4096']) * 1e3:.2f} ms")
    print(tail, flush=True)
    lines.append(tail)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
