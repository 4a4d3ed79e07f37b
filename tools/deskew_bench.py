"""Timing of the motion compensation of LiDAR sweeps (csrc/lpd_deskew.hip, lpdnet_hip/odometry.py) on the two 2 km drives of
tools/drive_bench.py: the pushbroom drive (20000 scans of 541 rows) and the sweep drive (400 scans of 65536 rows).

  (a) lpd_scan_deskew over the whole scan table, out of place and in place, beside lpd_drive_rows of the same drive and
      lpd_gather_tuples in the same run: the kernel's rate on its 28 bytes a row (12 in, 4 of the time, 12 out) against 8 TB/s and
      against the gather's copy rate.  lpd_drive_motions of the drive's poses beside it.
  (b) a plain-torch rung of the same transform: searchsorted for the scan of a row, the blend and the product in float64, narrowed at
      the end, in passes of 4 M rows.
  (c) the whole chain, odometry.estimate_poses over the first --scans scans of the sweep drive's scan lines (tools/odom_bench.py's
      drive) with times against without, alternating in the same run; the chain without times is the chain as it was.

    python tools/deskew_bench.py [--iters 10] [--scans 40] [--out profiles/deskew_bench.txt]

Device figures are device time between two HIP events around `iters` back-to-back calls on one stream after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time); the chain is a host clock around estimate_poses, which ends in its one wait.
Needs a GPU.
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

from drive_bench import HBM, make_points, make_poses  # noqa: E402
from map_bench import scan_line_points  # noqa: E402
from submap_bench import _time  # noqa: E402


def torch_rung(points, offsets, times, motion, ref, rows_at_a_time=1 << 22):
    """plain torch on the device, float64: the quaternion of every motion by the trace branch (the motions of a drive turn by a few
    degrees), the normalised blend with the identity's, the rotation's quadratic form and the product, narrowed at the end"""
    m = motion.view(-1, 3, 4)
    R, t = m[:, :, :3], m[:, :, 3]
    s = torch.sqrt(1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]) * 2.0
    qb = torch.stack((0.25 * s, (R[:, 2, 1] - R[:, 1, 2]) / s, (R[:, 0, 2] - R[:, 2, 0]) / s, (R[:, 1, 0] - R[:, 0, 1]) / s), 1)
    qa = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=points.device)
    off = offsets.to(torch.int64)
    outs = []
    for lo in range(0, points.shape[0], rows_at_a_time):
        hi = min(points.shape[0], lo + rows_at_a_time)
        scan = torch.searchsorted(off, torch.arange(lo, hi, device=points.device), right=True) - 1
        a = (times[lo:hi].double() - ref)[:, None]
        q = qa + a * (qb[scan] - qa)
        q = q / q.norm(dim=1, keepdim=True)
        w, x, y, z = q.unbind(1)
        Ra = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                          2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), 1).view(-1, 3, 3)
        outs.append((torch.matmul(Ra, points[lo:hi, :3].double().unsqueeze(2)).squeeze(2) + a * t[scan]).float())
    return torch.cat(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--length", type=float, default=20.0)
    ap.add_argument("--stride", type=float, default=10.0)
    ap.add_argument("--scans", type=int, default=40, help="scans of the sweep drive that the whole chain runs over")
    ap.add_argument("--repeats", type=int, default=3, help="alternating runs of the chain with and without times")
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deskew_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, odometry, ops

    dev = torch.device("cuda:0")
    lines = [f"deskew_bench: {a.metres:g} m drives on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

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
        rows = S * n
        points = make_points(rows, dev, 11)
        g = torch.Generator(device=dev)
        g.manual_seed(13)
        times = torch.rand((rows,), generator=g, device=dev)
        poses = torch.from_numpy(poses_h).to(dev)
        off = drive._scan_offsets(lengths, dev)
        say(f"--- {name}: {S} scans x {n} rows = {rows} rows")
        plan = drive.plan_windows(poses, a.length, a.stride, lengths=lengths)
        W, total, longest = len(plan), int(plan.row_counts.sum()), int(plan.row_counts.max())
        tab = torch.empty((W, 4), dtype=torch.int32, device=dev)
        pos = torch.empty((W, 3), dtype=torch.float64, device=dev)
        q = torch.empty((S,), dtype=torch.int64, device=dev)
        lib.lpd_drive_steps(p(poses), S, p(q), ops._stream())
        lib.lpd_drive_plan(p(torch.cumsum(q, 0)), S, p(off), p(poses), plan.length_units, plan.stride_units, 0, W, p(tab), p(pos), ops._stream())
        wout = torch.empty((total, 3), device=dev)
        t_r = _time(lambda: lib.lpd_drive_rows(p(points), 3, rows, p(off), p(poses), S, p(tab), W, p(plan.offsets), 1, longest, p(wout), ops._stream()),
                    a.iters)
        rate_r = 24.0 * total / t_r
        say(f"(a) lpd_drive_rows, frame = 1, {total} output rows                 {t_r * 1e6:9.1f} us   {rate_r / 1e12:.2f} TB/s on 24 B a row = "
            f"{rate_r / HBM:.2f} of 8 TB/s, {rate_r / gather_rate:.2f} of the gather's copy rate")
        del wout
        t_m = _time(lambda: ops.drive_motions(poses), a.iters)
        motion = ops.drive_motions(poses)
        out = torch.empty((rows, 3), device=dev)
        info = torch.zeros((2,), dtype=torch.int64, device=dev)
        t_d = _time(lambda: ops.scan_deskew(points, off, times, motion, 0.5, out, info), a.iters)
        same = points.clone()
        t_i = _time(lambda: ops.scan_deskew(same, off, times, motion, 0.5, same, info), a.iters)
        for what, t in (("out of place", t_d), ("in place", t_i)):
            rate = 28.0 * rows / t
            say(f"(a) lpd_scan_deskew, {what:12s}                               {t * 1e6:9.1f} us   {rate / 1e12:.2f} TB/s on 28 B a row = "
                f"{rate / HBM:.2f} of 8 TB/s, {rate / gather_rate:.2f} of the gather's copy rate; {t / rows * 1e12:.1f} ps a row")
        say(f"(a) lpd_drive_motions of {S} poses                                  {t_m * 1e6:9.1f} us")
        info.zero_()
        ops.scan_deskew(points, off, times, motion, 0.5, out, info)
        t_t = _time(lambda: torch_rung(points, off, times, motion, 0.5), max(2, a.iters // 5))
        worst = float((torch_rung(points, off, times, motion, 0.5) - out).abs().max())
        say(f"(b) plain torch: searchsorted + float64 blend and product         {t_t * 1e6:9.1f} us   = {t_t / t_d:.1f} x lpd_scan_deskew; rows "
            f"transformed / passed {info.tolist()}, largest difference {worst:.2e} m")
        del points, times, out, same
        torch.cuda.empty_cache()

    # (c) the chain with and without times
    S, n = 400 // scale, 65536
    Sc = min(a.scans, S)
    poses_h = make_poses(S, a.metres / scale, 7)
    lengths = np.full(Sc, n, dtype=np.int64)
    points = scan_line_points(S, n, dev, 11)[:Sc * n].contiguous()
    times = odometry.azimuth_fractions(points, lengths)
    first = np.linalg.inv(np.vstack((poses_h[0].reshape(3, 4), [0, 0, 0, 1]))) @ np.vstack((poses_h[1].reshape(3, 4), [0, 0, 0, 1]))
    say(f"--- sweep, scan lines: the chain over the first {Sc} scans x {n} rows, times from the azimuth")
    for cell in (0.2, 1.0):
        per, last = {}, {}
        search = odometry.OdometrySearch(cell=cell, keep=60.0, refresh=10, first_motion=np.ascontiguousarray(first[:3]))
        for rep in range(a.repeats + 1):      # the first round is the warm-up
            for with_times in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                odo = odometry.estimate_poses(points, lengths, poses_h[0], search, times=times if with_times else None)
                torch.cuda.synchronize()
                if rep:
                    per.setdefault(with_times, []).append((time.perf_counter() - t0) / Sc)
                last[with_times] = odo
        for with_times in (False, True):
            odo = last[with_times]
            say(f"(c) cell {cell:g} m, chain {'with   ' if with_times else 'without'} times: {Sc - odo.lost} of {Sc} scans accepted, {odo.passed} rows passed "
                f"through; per scan " + " / ".join(f"{t * 1e6:.0f}" for t in per[with_times]) + f" us (best {min(per[with_times]) * 1e6:.0f})")
        say(f"(c) cell {cell:g} m, chain per scan, with / without times = {min(per[True]) / min(per[False]):.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
