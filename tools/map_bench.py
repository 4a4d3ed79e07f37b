"""Timing of the drive map (csrc/lpd_map.hip, lpdnet_hip/mapping.py) on the two 2 km drives of tools/drive_bench.py -- a pushbroom drive
of 20000 scans x 541 rows and a sweep drive of 400 scans x 65536 rows -- at a cell of 0.2 m and of 1 m.  Each shape twice: with
drive_bench's rows (uniform clutter in no order: consecutive rows share no cell, the worst case of the per-workgroup sums) and with
rows on surfaces in the order a scanner emits them (scan_line_points: consecutive rows fall into the same few cells).

  (a) lpd_map_insert into a CLEARED table (every cell is created: compare-and-swap + adds) and into the table it has just filled (every
      key matches: adds only), in both forms: rows summed per workgroup in LDS first (the default), and LPD_DEBUG=map-direct (every row
      straight to the table).  Rows per second, global 64-bit atomics per row in each form (the aggregated form's from the distinct
      (chunk, key) pairs of the input, counted in torch), and the 64-bit integer atomic rate this implies.
  (b) lpd_drive_rows over the same rows in the same run (frame = 0, windows that hold every row once): the copy-rate yardstick -- the
      insert reads the same 12 bytes a row.
  (c) what the kernel replaces, on the same rows: plain torch, unique(return_inverse=True) + index_add_ on int64 keys.  The rung is
      handed the WORLD rows (it does not pay for the transform) and makes the same keys, sums and counts.
  (d) the extraction (mapping.extract_cells) and lpd_drive_correct at S = 20000.

    python tools/map_bench.py [--iters 10] [--out profiles/map_bench.txt]

Device figures are device time between two HIP events around `iters` back-to-back calls on one stream after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time).  A cleared-table figure includes the three fills that clear it; they are
timed alone as well.  Needs a GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from drive_bench import make_points, make_poses  # noqa: E402
from submap_bench import _time  # noqa: E402

CHUNK = 1024


def torch_rung(world, inv_cell):
    """world rows [n, 3] fp32 -> (keys, sums [M, 3] int64, counts [M]) in plain torch"""
    f = torch.floor(world * inv_cell)
    ok = ((f >= -1048576.0) & (f < 1048576.0)).all(dim=1)
    q = f[ok].to(torch.int64) + 1048576
    key = q[:, 0] | (q[:, 1] << 21) | (q[:, 2] << 42)
    U = torch.round(world[ok].double() * 65536.0).to(torch.int64)
    keys, inv = torch.unique(key, return_inverse=True)
    sums = torch.zeros((keys.shape[0], 3), dtype=torch.int64, device=world.device).index_add_(0, inv, U)
    counts = torch.zeros((keys.shape[0],), dtype=torch.int64, device=world.device).index_add_(0, inv, torch.ones_like(inv))
    return keys, sums, counts


def world_rows(points, lengths, poses, origin):
    """the world rows of lpd_map_insert in plain torch, operation for operation (eager elementwise fp32 operations are not fused)"""
    dev = points.device
    scan = torch.repeat_interleave(torch.arange(len(lengths), device=dev), torch.from_numpy(lengths).to(dev))
    P = poses.view(-1, 3, 4)
    M, u = P[:, :, :3].float()[scan], (P[:, :, 3] - origin).float()[scan]
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    return torch.stack([(((M[:, c, 0] * x) + (M[:, c, 1] * y)) + (M[:, c, 2] * z)) + u[:, c] for c in range(3)], dim=1)


def chunk_keys(world, inv_cell):
    """the distinct (chunk, key) pairs of the rows: what the aggregated form sends to the table when no workgroup's table spills"""
    f = torch.floor(world * inv_cell).to(torch.int64) + 1048576
    key = f[:, 0] | (f[:, 1] << 21) | (f[:, 2] << 42)
    pad = (-key.shape[0]) % CHUNK
    if pad:
        key = torch.cat((key, key[-1:].expand(pad)))
    ks = key.view(-1, CHUNK).sort(dim=1).values
    return int(ks.shape[0] + (ks[:, 1:] != ks[:, :-1]).sum())


def scan_line_points(S, n, dev, seed):
    """Sensor-frame rows in the order a scanner emits them, on surfaces: a street of ground at z = -1.7 m between walls.  n < 4096: a
    2-D line scanner across the road (n beams over 270 degrees in the y-z plane); else a 64-beam sweep (n / 64 azimuth steps, the 64
    beams of a step consecutive, elevations -24 .. +2 degrees) in a yard of 20 m x 60 m.  2 cm of range noise; at most 50 m."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    j = torch.arange(n, device=dev, dtype=torch.float32)
    if n < 4096:
        a = torch.deg2rad(-135.0 + 270.0 * j / (n - 1)) - 3.14159265 / 2      # 0 = straight down
        dy, dz = torch.cos(a + 3.14159265 / 2) * 0 + torch.sin(a + 3.14159265 / 2), -torch.cos(a + 3.14159265 / 2)
        r = torch.minimum(torch.where(dz < -1e-3, 1.7 / (-dz).clamp(min=1e-3), torch.full_like(dz, 50.0)), 8.0 / dy.abs().clamp(min=1e-3)).clamp(max=50.0)
        d = torch.stack((torch.zeros_like(dy), dy, dz), 1)
    else:
        az = 2.0 * 3.14159265 * torch.div(j, 64, rounding_mode="floor") / (n // 64)
        el = torch.deg2rad(-24.0 + 26.0 * (j % 64) / 63.0)
        wall = torch.minimum(10.0 / torch.sin(az).abs().clamp(min=1e-3), 30.0 / torch.cos(az).abs().clamp(min=1e-3)) / torch.cos(el)
        ground = torch.where(el < -1e-3, 1.7 / (-torch.sin(el)).clamp(min=1e-3), torch.full_like(el, 50.0))
        r = torch.minimum(wall, ground).clamp(max=50.0)
        d = torch.stack((torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)), 1)
    r = r[None, :] + 0.02 * torch.randn((S, n), generator=g, device=dev)
    return (r[:, :, None] * d[None, :, :]).reshape(S * n, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, mapping, ops

    dev = torch.device("cuda:0")
    lines = [f"map_bench: {a.metres:g} m drives on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def with_debug(token, fn):
        old = os.environ.get("LPD_DEBUG")
        if token:
            os.environ["LPD_DEBUG"] = (old + "," if old else "") + token
        try:
            return fn()
        finally:
            if token:
                if old is None:
                    del os.environ["LPD_DEBUG"]
                else:
                    os.environ["LPD_DEBUG"] = old

    scale = 10 if a.small else 1
    for name, S, n, lines_ in (("pushbroom", 20000 // scale, 541, False), ("sweep", 400 // scale, 65536, False),
                               ("pushbroom, scan lines", 20000 // scale, 541, True), ("sweep, scan lines", 400 // scale, 65536, True)):
        rows = S * n
        poses_h = make_poses(S, a.metres / scale, 7)
        lengths = np.full(S, n, dtype=np.int64)
        points = scan_line_points(S, n, dev, 11) if lines_ else make_points(rows, dev, 11)
        poses = torch.from_numpy(poses_h).to(dev)
        origin = poses[0][[3, 7, 11]].contiguous()
        off = drive._scan_offsets(lengths, dev)
        say(f"--- {name}: {S} scans x {n} rows = {rows} rows")

        # (b) the copy-rate yardstick: every row once through lpd_drive_rows, frame = 0
        plan = drive.plan_windows(poses, 20.0, 20.0, lengths=lengths)
        total = int(plan.row_counts.sum())
        t_rows = _time(lambda: drive.accumulate(points, lengths, plan=plan, frame="world"), a.iters)
        say(f"(b) lpd_drive_rows, frame = 0, {total} rows                       {t_rows * 1e6:9.1f} us   {total / t_rows / 1e9:6.2f} G rows/s   "
            f"{24.0 * total / t_rows / 1e12:.2f} TB/s on 24 B a row")

        for cell in (0.2, 1.0):
            inv = ops.map_inv_cell(cell)
            world = world_rows(points, lengths, poses, origin)
            keys_t, sums_t, counts_t = torch_rung(world, inv)
            cells = int(keys_t.shape[0])
            flushes = chunk_keys(world, inv)
            cap = 1 << 16
            while cap < 2 * cells:
                cap *= 2
            say(f"  cell {cell:g} m: {cells} occupied cells = {rows / cells:.1f} rows a cell; {flushes} distinct (chunk, key) pairs = "
                f"{flushes / rows:.3f} a row; table of {cap} slots ({40 * cap / 2 ** 20:.0f} MiB), load {cells / cap:.2f}")
            keys, acc, info = ops.map_table(cap, dev)

            def clear():
                keys.fill_(-1)
                acc.zero_()
                info.zero_()

            def insert():
                ops.map_insert(points, off, poses, origin, inv, keys, acc, info)

            def fresh():
                clear()
                insert()

            t_clear = _time(clear, a.iters)
            for form, token in (("LDS-aggregated", None), ("map-direct", "map-direct")):
                t_new = with_debug(token, lambda: _time(fresh, a.iters)) - t_clear
                with_debug(token, fresh)
                t_hit = with_debug(token, lambda: _time(insert, a.iters))
                atomics = 4.0 * (flushes if token is None else rows)      # the adds; a created cell costs one compare-and-swap more
                say(f"(a) lpd_map_insert, {form:14s} cleared table / filled table   {t_new * 1e6:9.1f} / {t_hit * 1e6:9.1f} us   "
                    f"{rows / t_new / 1e9:6.2f} / {rows / t_hit / 1e9:6.2f} G rows/s   {atomics / rows:.2f} global adds a row = "
                    f"{atomics / t_hit / 1e9:.2f} G 64-bit atomics/s ({8.0 * atomics / t_hit / 1e12:.2f} TB/s of added bytes); "
                    f"{t_new / t_rows:.2f} x lpd_drive_rows")
            with_debug(None, fresh)
            lost = int(info[2])
            got = mapping.extract_cells(keys, acc, origin, cell)
            same = bool(torch.equal(got.keys, keys_t) and torch.equal(got.sums, sums_t) and torch.equal(got.counts, counts_t))
            t_ex = _time(lambda: mapping.extract_cells(keys, acc, origin, cell), a.iters)
            t_t = _time(lambda: torch_rung(world, inv), max(a.iters // 2, 2), warmup=1)
            say(f"(c) plain torch on the world rows: unique(return_inverse) + index_add_   {t_t * 1e6:9.1f} us   {rows / t_t / 1e9:6.2f} G rows/s; "
                f"the same keys, sums and counts: {same}; rows lost {lost}")
            say(f"(d) extraction (mask, sort, gather, mean), clearing the table            {t_ex * 1e6:9.1f} / {t_clear * 1e6:.1f} us")
            del world, keys, acc, keys_t, sums_t, counts_t, got
            torch.cuda.empty_cache()

        if name == "pushbroom":
            _, D = ops.drive_distance(poses)
            node_scan = torch.arange(0, S, 20, dtype=torch.int32, device=dev)
            node_pose = poses[node_scan.to(torch.int64)].contiguous()
            t_c = _time(lambda: ops.drive_correct(poses, D, node_scan, node_pose), a.iters)
            say(f"(d) lpd_drive_correct, S = {S}, a node every 20 scans (with the zero-fill of its counters)   {t_c * 1e6:9.1f} us")
        del points
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
