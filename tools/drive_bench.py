"""Timing of the drive step in front of the cleaning and the submaps (csrc/lpd_drive.hip, lpdnet_hip/drive.py) on two 2 km drives:
a pushbroom drive of 20000 scans x 541 rows and a sweep drive of 400 scans x 65536 rows, 20 m windows every 10 m.

  (a) the launches: lpd_drive_steps, the torch.cumsum behind it, lpd_drive_plan, lpd_drive_rows in both frames; the rows kernel's rate
      on its 24 bytes per point against 8 TB/s and against the copy rate of lpd_gather_tuples (24 bytes per point as well) in this run;
  (b) drive.accumulate with a plan (no wait for the device) and drive.plan_windows (the two waits);
  (c) what they replace, on the same input: the numpy recipe on the host (float64, one matrix product per scan and window), and a
      plain-torch rung on the device: searchsorted + repeat_interleave + batched matmul in float64, narrowed at the end;
  (d) drive.submaps_from_drive with and without clean=, and submap.make_submaps(clean=) on the accumulated rows, which it feeds.

    python tools/drive_bench.py [--iters 20] [--length 20] [--stride 10] [--num-points 4096] [--out profiles/drive_bench.txt]

Device figures are device time between two HIP events around `iters` back-to-back calls on one stream after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time): call time in a full stream, launch gaps included.  Functions that wait for
the device are timed the same way, so their waits are in the figure.  The numpy recipe is host wall time, once.  Needs a GPU.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from submap_bench import _time  # noqa: E402

HBM = 8.0e12      # bytes / s


def make_poses(S, metres, seed):
    """S poses along a slowly turning road of `metres`, at UTM magnitude, with a little roll and pitch -> [S, 12] float64"""
    g = np.random.default_rng(seed)
    yaw = np.cumsum(g.normal(0.0, 0.3 / np.sqrt(S), S))
    roll, pitch = g.normal(0.0, 0.005, S), g.normal(0.0, 0.005, S)
    step = metres / (S - 1)
    t = np.zeros((S, 3))
    t[0] = (5.7e6, 6.2e5, 80.0)
    t[1:] = t[0] + np.cumsum(step * np.stack((np.cos(yaw[1:]), np.sin(yaw[1:]), np.zeros(S - 1)), 1), 0)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.zeros((S, 3, 3)); Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = cy, -sy, sy, cy, 1
    Ry = np.zeros((S, 3, 3)); Ry[:, 0, 0], Ry[:, 0, 2], Ry[:, 2, 0], Ry[:, 2, 2], Ry[:, 1, 1] = cp, sp, -sp, cp, 1
    Rx = np.zeros((S, 3, 3)); Rx[:, 1, 1], Rx[:, 1, 2], Rx[:, 2, 1], Rx[:, 2, 2], Rx[:, 0, 0] = cr, -sr, sr, cr, 1
    return np.concatenate((Rz @ Ry @ Rx, t[:, :, None]), 2).reshape(S, 12)


def make_points(rows, dev, seed):
    """sensor-frame rows made on the device: half of them a road at z = -1.7 m, the rest clutter above it, within 50 m"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    p = torch.rand((rows, 3), generator=g, device=dev)
    p[:, :2] = p[:, :2] * 100.0 - 50.0
    road = torch.rand((rows,), generator=g, device=dev) < 0.5
    p[:, 2] = torch.where(road, -1.7 + 0.03 * (p[:, 2] - 0.5), -1.5 + 7.0 * p[:, 2])
    return p


def numpy_recipe(points, offsets, poses, table):
    """the host recipe, float64: every scan of every window through R_ref^T (R_i x + t_i - t_ref), narrowed at the end"""
    P = poses.reshape(-1, 3, 4)
    out = np.empty((int(table[:, 3].sum()), 3), dtype=np.float32)
    at = 0
    for first, end, ref, n in table:
        if ref < 0:
            continue
        Rr, tr = P[ref, :, :3], P[ref, :, 3]
        for i in range(first, end):
            a, b = offsets[i], offsets[i + 1]
            M, u = Rr.T @ P[i, :, :3], Rr.T @ (P[i, :, 3] - tr)
            out[at:at + b - a] = points[a:b].astype(np.float64) @ M.T + u
            at += b - a
    return out


def torch_rung(points, offsets, poses, D, L, T, W, windows_at_a_time=16):
    """plain torch on the device: searchsorted for the three bounds and for the scan of a row, repeat_interleave for the rows' windows,
    one batched float64 matmul per row, narrowed at the end; `windows_at_a_time` windows per pass bound the [rows, 3, 3] float64 gather"""
    dev = points.device
    w = torch.arange(W, device=dev, dtype=torch.int64)
    first, end = torch.searchsorted(D, w * T), torch.searchsorted(D, w * T + L)
    ref = torch.minimum(torch.searchsorted(D, w * T + L // 2), end - 1)
    R, t = poses.view(-1, 3, 4)[:, :, :3], poses.view(-1, 3, 4)[:, :, 3]
    off = offsets.to(torch.int64)
    rows = off[end] - off[first]
    outs = []
    for a in range(0, W, windows_at_a_time):
        b = min(W, a + windows_at_a_time)
        n = rows[a:b]
        win = torch.repeat_interleave(torch.arange(a, b, device=dev), n)      # waits for the total
        start = torch.cumsum(n, 0) - n
        src = off[first[win]] + torch.arange(win.numel(), device=dev) - start[win - a]
        scan = torch.searchsorted(off, src, right=True) - 1
        Rr = R[ref[win]].transpose(1, 2)
        x = torch.matmul(R[scan], points[src].double().unsqueeze(2)).squeeze(2) + (t[scan] - t[ref[win]])
        outs.append(torch.matmul(Rr, x.unsqueeze(2)).squeeze(2).float())
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--length", type=float, default=20.0)
    ap.add_argument("--stride", type=float, default=10.0)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--num-points", type=int, default=4096)
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drive_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, ops, submap

    dev = torch.device("cuda:0")
    lines = [f"drive_bench: {a.metres:g} m drives, {a.length:g} m windows every {a.stride:g} m on {torch.cuda.get_device_name(0)}; "
             f"device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # the copy rate of lpd_gather_tuples in this run: 12 bytes in and 12 bytes out per point, as the rows kernel
    Tn, N = 4096, 4096
    table = torch.rand((Tn, N, 3), device=dev)
    items = torch.randperm(Tn, device=dev).to(torch.int32)
    buf = torch.empty((Tn, N, 3), device=dev)
    t_g = _time(lambda: ops.gather_tuples(table, items, out=buf), a.iters)
    gather_rate = 24.0 * Tn * N / t_g
    say(f"(a) lpd_gather_tuples, {Tn} clouds x {N} points, plain copy          {t_g * 1e6:9.1f} us   {gather_rate / 1e12:.2f} TB/s "
        f"({gather_rate / HBM:.2f} of 8 TB/s)")
    del table, buf

    lib, p = ops._lib.load(), ops._ptr
    scale = 10 if a.small else 1
    for name, S, n in (("pushbroom", 20000 // scale, 541), ("sweep", 400 // scale, 65536)):
        poses_h = make_poses(S, a.metres / scale, 7)
        lengths = np.full(S, n, dtype=np.int64)
        points = make_points(S * n, dev, 11)
        poses = torch.from_numpy(poses_h).to(dev)
        plan = drive.plan_windows(poses, a.length, a.stride, lengths=lengths)
        W, L, T = len(plan), plan.length_units, plan.stride_units
        total, longest = int(plan.row_counts.sum()), int(plan.row_counts.max())
        say(f"--- {name}: {S} scans x {n} rows = {S * n} rows; {W} windows, {total} output rows, longest window {longest}")
        off = plan.scan_offsets
        q = torch.empty((S,), dtype=torch.int64, device=dev)
        t_s = _time(lambda: lib.lpd_drive_steps(p(poses), S, p(q), ops._stream()), a.iters)
        D = torch.cumsum(q, 0)
        t_c = _time(lambda: torch.cumsum(q, 0), a.iters)
        tab = torch.empty((W, 4), dtype=torch.int32, device=dev)
        pos = torch.empty((W, 3), dtype=torch.float64, device=dev)
        t_p = _time(lambda: lib.lpd_drive_plan(p(D), S, p(off), p(poses), L, T, 0, W, p(tab), p(pos), ops._stream()), a.iters)
        say(f"(a) lpd_drive_steps / torch.cumsum / lpd_drive_plan               {t_s * 1e6:9.1f} / {t_c * 1e6:.1f} / {t_p * 1e6:.1f} us")
        out = torch.empty((total, 3), device=dev)
        t_r = {}
        for frame in (1, 0):
            t_r[frame] = _time(lambda: lib.lpd_drive_rows(p(points), 3, S * n, p(off), p(poses), S, p(tab), W, p(plan.offsets), frame, longest,
                                                          p(out), ops._stream()), a.iters)
            rate = 24.0 * total / t_r[frame]
            say(f"(a) lpd_drive_rows, frame = {frame}                                    {t_r[frame] * 1e6:9.1f} us   {rate / 1e12:.2f} TB/s on 24 B "
                f"per point = {rate / HBM:.2f} of 8 TB/s, {rate / gather_rate:.2f} of the gather's copy rate")
        t_acc = _time(lambda: drive.accumulate(points, lengths, plan=plan), a.iters)
        t_plan = _time(lambda: drive.plan_windows(poses, a.length, a.stride, lengths=lengths), a.iters)
        say(f"(b) drive.accumulate with a plan / drive.plan_windows (two waits) {t_acc * 1e6:9.1f} / {t_plan * 1e6:.1f} us")

        # (c) what they replace
        table_h, points_h, off_h = tab.cpu().numpy(), points.cpu().numpy(), off.cpu().numpy().astype(np.int64)
        t0 = time.perf_counter()
        ref = numpy_recipe(points_h, off_h, poses_h, table_h)
        t_np = time.perf_counter() - t0
        got = drive.accumulate(points, lengths, plan=plan).points
        err = float((got.cpu() - torch.from_numpy(ref)).abs().max())
        say(f"(c) the numpy recipe on the host (float64), once                  {t_np * 1e6:9.1f} us   = {t_np / (t_s + t_c + t_p + t_r[1]):.0f} x the "
            f"launches; max |difference| to the kernel's rows {err:.2e} m")
        t_t = _time(lambda: torch_rung(points, off, poses, D, L, T, W), max(a.iters // 10, 2), warmup=1)
        diff = float((torch_rung(points, off, poses, D, L, T, W) - got).abs().max())
        say(f"(c) plain torch: searchsorted + repeat_interleave + f64 matmul    {t_t * 1e6:9.1f} us   = {t_t / t_r[1]:.1f} x lpd_drive_rows; "
            f"max |difference| {diff:.2e} m")
        del ref, points_h

        # (d) the whole step and what it feeds
        clean = submap.RoadRemoval(r_max=50.0)
        it = max(a.iters // 4, 3)
        t_sub = _time(lambda: drive.submaps_from_drive(points, lengths, poses, a.length, a.stride, a.num_points), it, warmup=2)
        t_subc = _time(lambda: drive.submaps_from_drive(points, lengths, poses, a.length, a.stride, a.num_points, clean=clean), it, warmup=2)
        counts = plan.row_counts.tolist()
        t_ms = _time(lambda: submap.make_submaps(got, counts, a.num_points, clean=clean), it, warmup=2)
        say(f"(d) submaps_from_drive, no clean / clean=RoadRemoval(r_max=50)    {t_sub * 1e6:9.1f} / {t_subc * 1e6:.1f} us")
        say(f"(d) make_submaps(clean=) on the accumulated rows, which it feeds  {t_ms * 1e6:9.1f} us   (the drive step = plan_windows + accumulate = "
            f"{(t_plan + t_acc) / t_ms:.3f} x it)")
        del points, out, got
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
