"""Timing of the 6-DoF refinement (csrc/lpd_icp.hip, lpdnet_hip/verify.py) at the sizes a user runs: N = 4096 points a cloud, the
default verify.RefineSearch (normals from 16 neighbours, eight steps at dmax = 1 m, nine passes), P = 1 pair, 25 (one query's
candidates) and 800 (32 queries x 25), started from verify.align_pairs' alignment.

  (a) point_normals of 32 clouds against the xyz kNN that feeds it;
  (b) one correspondence pass (ops.icp_pairs with no step: one memset, the init, one pass and one step launch) and the lane-operations
      per second of the pass -- N * N candidates x 11 VALU operations (three differences, three products, two sums, one compare, two
      selects) over its time -- against the chip's plain fp32 VALU rate, 256 CUs x 4 SIMDs x 32 lanes a cycle x 2.4 GHz = 78.6e12
      lane-operations/s (the 157.3 TFLOP/s fp32 vector peak counts an FMA as two);
      the whole verify.refine_pairs with the normals given and with the normals made inside; verify.align_pairs beside it;
  (c) one plain-torch rung for 25 pairs: torch.cdist + argmin + torch.linalg.solve, the same nine passes in float64 steps; its poses
      must agree with the kernel's to 0.05 degrees and 2 cm before anything is printed (cdist expands the squares, so a tie or a
      candidate at the edge of dmax can fall the other way);
  (d) the 32-cloud eval forward of LPD-Net in the same run, the yardstick: what share of it a query's 25 refinements cost.

    python tools/icp_bench.py [--iters 30] [--out profiles/icp_bench.txt]

Every step runs in a child process of its own with a time limit, one at a time; the tool stops at the first step that fails.  The
clouds are the labelled street scenes of tests/align_ref.py (fixed seeds).  Needs a GPU.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = (("normals", 300), ("pairs:1", 300), ("pairs:25", 420), ("pairs:800", 420), ("forward", 300))
N, QUERIES, CANDIDATES = 4096, 32, 25
LANE_OPS_PER_CANDIDATE = 11
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def step_normals(iters):
    import torch
    from align_bench import _median_events, tables
    from lpdnet_hip import ops
    dev = torch.device("cuda:0")
    _, B, _ = tables()
    x = torch.from_numpy(B[:QUERIES]).to(dev)
    rows = x.reshape(QUERIES * N, 3)
    idx = ops.knn_pm(rows, QUERIES, N, 16)
    tk, tk_min = _median_events(lambda: ops.knn_pm(rows, QUERIES, N, 16), iters)
    tn, tn_min = _median_events(lambda: ops.point_normals(rows, idx, QUERIES, N), iters)
    zero = int((ops.point_normals(rows, idx, QUERIES, N) == 0).all(dim=1).sum())
    print(f"normals of {QUERIES} clouds x {N} points, 16 neighbours: xyz kNN median {tk * 1e6:8.1f} us (min {tk_min * 1e6:.1f})   point_normals "
          f"{tn * 1e6:8.1f} us (min {tn_min * 1e6:.1f}) = {tn / tk:.2f} x the kNN, {tn / QUERIES * 1e6:.2f} us a cloud; {zero} zero normals")


def torch_rung(a, b, nb, pose, schedule, min_inliers):
    """the same nine passes for P pairs in plain torch: a, b, nb [P, N, 3] on the device, pose [P, 3, 4] float64 -> pose [P, 3, 4]"""
    import torch
    pose = pose.clone()
    for s, dmax in enumerate(schedule[:-1]):
        M = pose.to(torch.float32)
        p = a @ M[:, :, :3].transpose(1, 2) + M[:, None, :, 3]
        d = torch.cdist(p, b)
        dist, j = d.min(dim=2)
        q = torch.gather(b, 1, j[..., None].expand(-1, -1, 3))
        n = torch.gather(nb, 1, j[..., None].expand(-1, -1, 3))
        w = ((dist <= dmax) & (n != 0).any(dim=2)).to(torch.float64)[..., None]
        J = torch.cat((torch.cross(p, n, dim=2), n), dim=2).to(torch.float64) * w
        r = ((q - p) * n).sum(dim=2, keepdim=True).to(torch.float64) * w
        x = torch.linalg.solve(J.transpose(1, 2) @ J, (J.transpose(1, 2) @ r)[..., 0])      # raises on a singular system: no refusal here
        h = x[:, :3] * 0.5
        qt = torch.cat((torch.ones_like(h[:, :1]), h), dim=1)
        qw, qx, qy, qz = (qt / qt.norm(dim=1, keepdim=True)).unbind(dim=1)
        dR = torch.stack((1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                          2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                          2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)), dim=1).reshape(-1, 3, 3)
        pose = dR @ pose
        pose[:, :, 3] += x[:, 3:]
    return pose


def step_pairs(P, iters):
    import numpy as np
    import torch
    from align_bench import _median_events, tables
    from lpdnet_hip import ops, verify
    dev = torch.device("cuda:0")
    A, B, pairs = tables()
    a, b = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    pr = torch.from_numpy(pairs[:P]).to(dev)
    s = verify.RefineSearch()
    al = verify.align_pairs(a, b, pr)
    nb = verify.point_normals(b, s.k)
    rf = verify.refine_pairs(a, b, pr, init=al, search=s, normals_b=nb)
    start = verify._init_pose(al, P, dev)[0]

    def one_pass():
        return ops.icp_pairs(a, b, nb, pr, start, [s.dmax[0]], s.min_inliers)
    tp, tp_min = _median_events(one_pass, iters)
    tr, tr_min = _median_events(lambda: verify.refine_pairs(a, b, pr, init=al, search=s, normals_b=nb), iters)
    tw, tw_min = _median_events(lambda: verify.refine_pairs(a, b, pr, init=al, search=s), iters)
    ta, ta_min = _median_events(lambda: verify.align_pairs(a, b, pr), iters)
    rate = P * float(N) * N * LANE_OPS_PER_CANDIDATE / tp
    is_true = pairs[:P, 0] == pairs[:P, 1]
    share, rms = rf.inlier_share.cpu().numpy(), rf.rms.cpu().numpy()
    print(f"P = {P:4d}  one pass (memset + init + pass + step launches) median {tp * 1e6:9.1f} us (min {tp_min * 1e6:.1f}) = {rate / 1e12:6.2f}e12 "
          f"lane-operations/s = {rate / VALU_LANE_OPS_PER_S:.3f} of the VALU rate   refine_pairs, normals given {tr * 1e6:9.1f} us (min "
          f"{tr_min * 1e6:.1f}) = {tr / P * 1e6:.1f} us a pair; normals made inside {tw * 1e6:9.1f} us (min {tw_min * 1e6:.1f})   "
          f"align_pairs {ta * 1e6:9.1f} us (min {ta_min * 1e6:.1f}): the refinement is {tr / ta:.2f} x it")
    print(f"P = {P:4d}  inlier share of the {int(is_true.sum())} revisits >= {share[is_true].min():.3f}, rms <= {rms[is_true].max():.3f} m" +
          (f"; of the {int((~is_true).sum())} other places share <= {share[~is_true].max():.3f}, rms >= {rms[~is_true].min():.3f} m" if (~is_true).any() else ""))
    print(f"KV refine{P} {tr}")
    print(f"KV align{P} {ta}")
    if P == CANDIDATES:
        ai, bi = pr[:, 0].long(), pr[:, 1].long()
        ga, gb, gn = a[ai], b[bi], nb[bi]

        def rung():
            return torch_rung(ga, gb, gn, start.reshape(P, 3, 4), s.schedule, s.min_inliers)
        got, want = rung().cpu().numpy(), rf.pose.cpu().numpy()
        t = np.where(is_true)[0]
        dR = got[t, :, :3] @ want[t, :, :3].transpose(0, 2, 1)
        ang = np.degrees(np.arccos(np.clip((np.trace(dR, axis1=1, axis2=2) - 1) / 2, -1, 1))).max()
        dt = np.linalg.norm(got[t, :, 3] - want[t, :, 3], axis=1).max()
        if not (ang <= 0.05 and dt <= 0.02):
            raise SystemExit(f"MISMATCH: the torch rung's poses of the revisits differ from the kernel's by {ang:.4f} deg, {dt:.4f} m")
        tt, tt_min = _median_events(rung, max(3, iters // 5), warmup=1)
        print(f"P = {P:4d}  plain torch (cdist + argmin + linalg.solve, eight steps; poses of the revisits within {ang:.4f} deg, {dt * 1e3:.2f} mm of the kernel's)"
              f"  median {tt * 1e6:9.1f} us (min {tt_min * 1e6:.1f}) = {tt / tr:.1f} x refine_pairs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("icp_bench: needs a GPU (no CPU timing)")
        if a.step == "forward":
            from align_bench import step_forward
            step_forward(a.iters)
        elif a.step == "normals":
            step_normals(a.iters)
        else:
            step_pairs(int(a.step.split(":")[1]), a.iters)
        return
    lines = [f"icp_bench: N = {N}, default RefineSearch (k = 16, eight steps at dmax = 1 m) from align_pairs' alignment; HIP-event medians of "
             f"{a.iters} calls; one child process a step"]
    kv = {}
    print(lines[0], flush=True)
    for step, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(a.iters)], capture_output=True, text=True,
                               timeout=limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"icp_bench: step {step} exceeded its {limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"icp_bench: step {step} failed (rc={r.returncode}); stopping\n{r.stdout}{r.stderr[-2000:]}")
        for line in r.stdout.splitlines():
            if line.startswith("KV "):
                kv[line.split()[1]] = float(line.split()[2])
            elif line.strip():
                print(line, flush=True)
                lines.append(line)
    per_cloud = kv["forward"] / QUERIES
    tail = (f"one query: its forward {per_cloud * 1e6:.1f} us (1/{QUERIES} of the batch's), its {CANDIDATES} refinements {kv['refine25'] * 1e6:.1f} us alone "
            f"= {kv['refine25'] / per_cloud:.2f} x that ({kv['refine25'] / kv['align25']:.2f} x its {CANDIDATES} alignments); in a batch of {QUERIES} queries "
            f"{kv['refine800'] / QUERIES * 1e6:.1f} us a query = {kv['refine800'] / kv['forward']:.2f} x the {QUERIES}-cloud forward "
            f"({kv['refine800'] / kv['align800']:.2f} x the alignments)")
    print(tail, flush=True)
    lines.append(tail)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
