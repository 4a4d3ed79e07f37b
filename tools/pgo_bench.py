"""Timing of the pose-graph optimisation (csrc/lpd_pgo.hip, lpdnet_hip/posegraph.py) at the sizes a user runs.

  (a) one drive: 200 nodes (the windows of a 2 km drive, 20 m every 10 m), two laps with a loop every fourth node -- ops.pgo_solve
      with the CSR made inside, and the kernel alone; the same graph on the host by scipy.optimize.least_squares and by the numpy
      restatement (tests/pgo_ref.py), whose result the device's must equal bit for bit before anything is printed;
  (b) 45 such drives in one launch (one workgroup each);
  (c) 21711 nodes, an Oxford-sized training set as ONE graph: one workgroup on one CU of 256, which the design accepts;
  (d) the verify.refine_pairs call that makes a small drive's loop edges, beside the solve that uses them.

    python tools/pgo_bench.py [--iters 20] [--out profiles/pgo_bench.txt]

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

STEPS = (("drive", 420), ("batch", 300), ("large", 420), ("refine", 300))
SOLVER = dict(outer=20, cg_iters=500, cg_tol=1e-6, lambda0=1e-4)
LARGE_SOLVER = dict(outer=6, cg_iters=40, cg_tol=1e-6, lambda0=1e-4)
DRIVE_NODES, BATCH, LARGE_NODES = 200, 45, 21711


def _up(dev, g):
    import numpy as np
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("start", "edge", "meas", "weight"))


def _kernel_alone(args, V, E, G, node_off, edge_off, solver):
    """-> a function that launches lpd_pgo_solve only: the CSR, the outputs and the workspace are made once"""
    import torch
    from lpdnet_hip import ops
    lib, ptr = ops._lib.load(), ops._ptr
    pose0, edge, meas, weight = args
    dev = pose0.device
    cp, ci = ops.pgo_csr(edge, node_off, edge_off, V)
    pose = pose0.clone()
    fixed = torch.zeros(V, dtype=torch.uint8, device=dev)
    cost = torch.empty((G, solver["outer"] + 1), dtype=torch.float64, device=dev)
    chi2 = torch.empty(E, dtype=torch.float64, device=dev)
    info = torch.empty((G, 8), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.lpd_pgo_workspace_bytes(V, E, G)), dtype=torch.uint8, device=dev)

    def run():
        pose.copy_(pose0)
        ops._call("pgo_solve", lib.lpd_pgo_solve, ptr(pose), ptr(fixed), ptr(node_off), V, ptr(edge), ptr(meas), ptr(weight), ptr(edge_off), E, G,
                  ptr(cp), ptr(ci), solver["outer"], solver["cg_iters"], solver["cg_tol"], solver["lambda0"], 0.0, ptr(cost), ptr(chi2), ptr(info),
                  ptr(ws), ops._stream())
    return run, info


def step_drive(iters):
    import numpy as np
    import torch
    import pgo_ref as R
    from align_bench import _median_events
    from lpdnet_hip import ops
    dev = torch.device("cuda:0")
    g = R.two_laps(11, DRIVE_NODES)
    args = _up(dev, g)
    V, E = DRIVE_NODES, len(g["edge"])
    t0 = time.perf_counter()
    ref = R.solve(g["start"], g["edge"], g["meas"], g["weight"], **SOLVER)
    t_ref = time.perf_counter() - t0
    got = [t.cpu().numpy() for t in ops.pgo_solve(*args, **SOLVER)]
    if not all(a.tobytes() == np.ascontiguousarray(b).astype(a.dtype).tobytes() for a, b in zip(got, ref)):
        raise SystemExit("MISMATCH: the device's solve differs from the restatement's")
    t0 = time.perf_counter()
    sp = R.scipy_solve(g["start"], g["edge"], g["meas"], g["weight"])
    t_sp = time.perf_counter() - t0
    tw, tw_min = _median_events(lambda: ops.pgo_solve(*args, **SOLVER), iters)
    off = torch.tensor([0, V], dtype=torch.int32, device=dev), torch.tensor([0, E], dtype=torch.int32, device=dev)
    run, info = _kernel_alone(args, V, E, 1, off[0], off[1], SOLVER)
    tk, tk_min = _median_events(run, iters)
    i = got[3][0]
    print(f"one drive: {V} nodes, {E} edges, outer <= {SOLVER['outer']}, cg <= {SOLVER['cg_iters']}: status {i[0]}, {i[1]} trials accepted, {i[2]} refused, "
          f"{i[3]} CG iterations; cost {got[1][0, 0]:.1f} -> {got[1][0, -1]:.6f} (scipy {sp[1]:.6f}, ratio - 1 = {got[1][0, -1] / sp[1] - 1:.2e}); ATE "
          f"{R.ate(g['start'], g['gt']):.3f} -> {R.ate(got[0], g['gt']):.3f} m (scipy {R.ate(sp[0], g['gt']):.3f} m)")
    print(f"one drive: ops.pgo_solve (CSR sort + launch) median {tw * 1e6:9.1f} us (min {tw_min * 1e6:.1f}); the kernel alone {tk * 1e6:9.1f} us (min "
          f"{tk_min * 1e6:.1f}) = {tk / max(int(i[3]), 1) * 1e6:.2f} us a CG iteration; on the host: restatement {t_ref:.2f} s = {t_ref / tk:.0f} x, scipy "
          f"least_squares {t_sp:.2f} s = {t_sp / tk:.0f} x (bits equal to the restatement)")
    print(f"KV drive {tk}")


def step_batch(iters):
    import numpy as np
    import torch
    import pgo_ref as R
    from align_bench import _median_events
    dev = torch.device("cuda:0")
    gs = [R.two_laps(100 + b, DRIVE_NODES) for b in range(BATCH)]
    cat = {k: np.concatenate([g[k] for g in gs]) for k in ("start", "edge", "meas", "weight")}
    args = _up(dev, cat)
    node_off = torch.tensor(np.arange(BATCH + 1) * DRIVE_NODES, dtype=torch.int32, device=dev)
    edge_off = torch.tensor(np.concatenate(([0], np.cumsum([len(g["edge"]) for g in gs]))), dtype=torch.int32, device=dev)
    run, info = _kernel_alone(args, BATCH * DRIVE_NODES, len(cat["edge"]), BATCH, node_off, edge_off, SOLVER)
    t, t_min = _median_events(run, iters)
    i = info.cpu().numpy()
    print(f"{BATCH} drives in one launch ({BATCH} workgroups): the kernel median {t * 1e6:9.1f} us (min {t_min * 1e6:.1f}) = {t / BATCH * 1e6:.1f} us a drive; "
          f"statuses {sorted(set(i[:, 0].tolist()))}, CG iterations {int(i[:, 3].min())} .. {int(i[:, 3].max())}")
    print(f"KV batch {t}")


def step_large(iters):
    import numpy as np
    import torch
    import pgo_ref as R
    from align_bench import _median_events
    dev = torch.device("cuda:0")
    g = R.two_laps(12, LARGE_NODES, radius=LARGE_NODES * 10.0 / (4.0 * np.pi))      # 10 m between nodes, as the windows of a drive
    args = _up(dev, g)
    V, E = LARGE_NODES, len(g["edge"])
    off = torch.tensor([0, V], dtype=torch.int32, device=dev), torch.tensor([0, E], dtype=torch.int32, device=dev)
    run, info = _kernel_alone(args, V, E, 1, off[0], off[1], LARGE_SOLVER)
    t, t_min = _median_events(run, max(3, iters // 4), warmup=1)
    i = info.cpu().numpy()[0]
    t0 = time.perf_counter()
    ref = R.solve(g["start"], g["edge"], g["meas"], g["weight"], **LARGE_SOLVER)
    t_ref = time.perf_counter() - t0
    print(f"one graph of {V} nodes, {E} edges on ONE workgroup (one CU of 256), outer <= {LARGE_SOLVER['outer']}, cg <= {LARGE_SOLVER['cg_iters']}: the kernel "
          f"median {t * 1e3:9.2f} ms (min {t_min * 1e3:.2f}) = {t / max(int(i[3]), 1) * 1e6:.1f} us a CG iteration ({i[3]} iterations, {i[1]} trials accepted, "
          f"status {i[0]}); the restatement on the host {t_ref:.1f} s = {t_ref / t:.0f} x, info equal: {bool((ref[3][0] == i).all())}; scipy is not run at "
          f"this size (minutes)")
    print(f"KV large {t}")


def step_refine(iters):
    import numpy as np
    import torch
    import align_ref as AR
    import pgo_ref as R
    from align_bench import _median_events
    from lpdnet_hip import drive, posegraph, verify
    dev = torch.device("cuda:0")
    sc = AR.scene(3, extent=40.0)
    g = np.random.default_rng(21)
    S, radius, n = 81, 80.0 / (2.0 * np.pi), 1024
    th = np.arange(S) * (2.0 / radius)
    true = np.array([R.pose12(R.yaw_rot(t + np.pi / 2), [radius * np.cos(t), radius * np.sin(t), 0.0]) for t in th])
    pts = np.concatenate([AR.submap(sc, true[s].reshape(3, 4)[:2, 3], th[s] + np.pi / 2, 100 + s, n=n) for s in range(S)])
    drifted = [true[0]]
    for s in range(S - 1):
        step = R.mul12(R.inv12(true[s]), true[s + 1])
        drifted.append(R.mul12(drifted[-1], R.mul12(step, R.pose12(R.yaw_rot(g.normal(0.002, 0.002)), [g.normal(0, 0.01), g.normal(0.01, 0.01), 0.0]))))
    drifted = np.array(drifted)
    sub, _ = drive.submaps_from_drive(torch.from_numpy(pts), [n] * S, drifted, 20.0, 10.0, num_points=2048, device=dev)
    W = len(sub.plan)
    pairs = torch.tensor([[w, w - 8] for w in range(8, W)], dtype=torch.int32, device=dev)
    al = verify.align_pairs(sub, sub, pairs)
    rf = verify.refine_pairs(sub, sub, pairs, init=al)
    ta, _ = _median_events(lambda: verify.align_pairs(sub, sub, pairs), iters)
    tr, _ = _median_events(lambda: verify.refine_pairs(sub, sub, pairs, init=al), iters)
    tc, _ = _median_events(lambda: posegraph.close_loops(sub, drifted, rf, pairs), iters)
    res = posegraph.close_loops(sub, drifted, rf, pairs)
    ref = sub.plan.ref.cpu().numpy()
    print(f"a drive of {S} scans, {W} windows of 2048 points, {len(pairs)} loops: align_pairs median {ta * 1e6:9.1f} us, refine_pairs (normals made inside) "
          f"{tr * 1e6:9.1f} us, close_loops (host poses uploaded, edges made, CSR, solve) {tc * 1e6:9.1f} us = {tc / tr:.2f} x the refinement; ATE of the "
          f"windows {R.ate(drifted[ref], true[ref]):.3f} -> {R.ate(res.poses.reshape(-1, 12).cpu().numpy(), true[ref]):.3f} m; info {res.info.cpu().tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pgo_bench: needs a GPU (no CPU timing)")
        {"drive": step_drive, "batch": step_batch, "large": step_large, "refine": step_refine}[a.step](a.iters)
        return
    lines = [f"pgo_bench: two-lap graphs (tests/pgo_ref.two_laps), a loop every fourth node; HIP-event medians of {a.iters} calls; one child process a step"]
    print(lines[0], flush=True)
    kv = {}
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"pgo_bench: step {step} exceeded its {limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"pgo_bench: step {step} failed (rc={r.returncode}); stopping\n{r.stdout}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("KV "):
                kv[line.split()[1]] = float(line.split()[2])
            elif line.strip():
                print(line, flush=True)
                lines.append(line)
    tail = (f"a drive alone {kv['drive'] * 1e6:.1f} us; in a batch of {BATCH} {kv['batch'] / BATCH * 1e6:.1f} us = {kv['drive'] * BATCH / kv['batch']:.1f} x "
            f"the throughput of one after the other; the {LARGE_NODES}-node graph {kv['large'] * 1e3:.2f} ms on one CU")
    print(tail, flush=True)
    lines.append(tail)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
