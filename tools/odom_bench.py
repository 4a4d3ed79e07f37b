"""Timing of LiDAR odometry (csrc/lpd_odom.hip, lpdnet_hip/odometry.py) on the 2 km sweep drive of tools/localize_bench.py -- scans of
65536 rows on surfaces in scanner order -- at a cell of 0.2 m and of 1 m.

  (a) the whole chain, odometry.estimate_poses over the first --scans scans, with surface="touched" against surface="full" in the same
      run, alternating; time per scan, scans accepted, cells of the final local map.  The full route is the existing lpd_map_surface:
      the yardstick.  The sweep drive's scans are one yard seen again and again (it is a timing drive, not a consistent world), so the
      odometry's poses are not judged here -- tests/test_odometry_cpu.py does that.
  (b) on the table of the WHOLE drive mapped at its true poses: lpd_map_touch + lpd_map_surface_touched behind the insert of one scan,
      against lpd_map_surface of the same table; the share of the slots that the scan marks.
  (c) lpd_map_crop around the middle of the drive against lpd_map_rehash of the same table into a table of the same size.
  (d) the chain's time per scan against the bare eight-step lpd_map_localize of one scan on the whole-drive table.

    python tools/odom_bench.py [--iters 10] [--scans 60] [--out profiles/odom_bench.txt]

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

from drive_bench import make_poses  # noqa: E402
from map_bench import scan_line_points  # noqa: E402
from submap_bench import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--scans", type=int, default=60, help="scans of the drive that the whole chain runs over")
    ap.add_argument("--repeats", type=int, default=3, help="alternating runs of each route of the chain")
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odom_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, mapping, odometry, ops

    dev = torch.device("cuda:0")
    lines = [f"odom_bench: {a.metres:g} m sweep drive on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scale = 10 if a.small else 1
    S, n = 400 // scale, 65536
    lengths = np.full(S, n, dtype=np.int64)
    poses_h = make_poses(S, a.metres / scale, 7)
    points = scan_line_points(S, n, dev, 11)
    poses = torch.from_numpy(poses_h).to(dev)
    off = drive._scan_offsets(lengths, dev)
    say(f"--- sweep, scan lines: {S} scans x {n} rows; the chain runs over the first {min(a.scans, S)}")
    Sc = min(a.scans, S)
    first = np.linalg.inv(np.vstack((poses_h[0].reshape(3, 4), [0, 0, 0, 1]))) @ np.vstack((poses_h[1].reshape(3, 4), [0, 0, 0, 1]))

    for cell in (0.2, 1.0):
        say(f"  cell {cell:g} m")
        # (a) the whole chain
        per = {}
        for rep in range(a.repeats + 1):      # the first round is the warm-up
            for surface in odometry.SURFACES:
                search = odometry.OdometrySearch(cell=cell, keep=60.0, refresh=10, first_motion=np.ascontiguousarray(first[:3]), surface=surface)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                odo = odometry.estimate_poses(points[:Sc * n], lengths[:Sc], poses_h[0], search)
                torch.cuda.synchronize()
                if rep:
                    per.setdefault(surface, []).append((time.perf_counter() - t0) / Sc)
                if rep == a.repeats:
                    say(f"(a) chain, surface={surface:8s}: {Sc - odo.lost} of {Sc} scans accepted, {len(odo.cells())} cells in {odo.capacity} slots, "
                        f"{odo.left_behind} cells left behind by the crops; per scan "
                        + " / ".join(f"{t * 1e6:.0f}" for t in per[surface]) + f" us (best {min(per[surface]) * 1e6:.0f})")
        t_chain = {k: min(v) for k, v in per.items()}
        say(f"(a) chain per scan, touched / full = {t_chain['touched'] / t_chain['full']:.2f}")
        # (b) touch + refresh against the full surface, on the whole drive's table
        vm = mapping.build_map(points, lengths, poses, cell=cell)
        cap, cells = vm.capacity, vm.occupied
        say(f"    whole drive: {cells} occupied cells in {cap} slots (load {cells / cap:.2f})")
        surf, _ = ops.map_surface(vm.keys, vm.acc, 1, 5)
        dirty = torch.zeros((cap,), dtype=torch.uint8, device=dev)
        mid = S // 2
        ops.map_touch(points, off, poses, vm.origin, vm.inv_cell, vm.keys, dirty, 1, mid, mid + 1)
        marked = int(dirty.sum())

        def touched():
            ops.map_touch(points, off, poses, vm.origin, vm.inv_cell, vm.keys, dirty, 1, mid, mid + 1)
            ops.map_surface_touched(vm.keys, vm.acc, surf, dirty, 1, 5)

        t_t = _time(touched, a.iters)
        t_touch = _time(lambda: ops.map_touch(points, off, poses, vm.origin, vm.inv_cell, vm.keys, dirty, 1, mid, mid + 1), a.iters)
        t_s = _time(lambda: ops.map_surface(vm.keys, vm.acc, 1, 5), a.iters)
        full, _ = ops.map_surface(vm.keys, vm.acc, 1, 5)
        touched()
        same = torch.equal(surf.view(torch.int32), full.view(torch.int32))
        say(f"(b) one scan of {n} rows marks {marked} slots ({marked / cap:.4f} of the table); touch + refresh {t_t * 1e6:9.1f} us (touch alone "
            f"{t_touch * 1e6:.1f}) against lpd_map_surface {t_s * 1e6:9.1f} us = {t_t / t_s:.2f}; the same bits: {same}")
        # (c) crop against rehash
        k2, a2, _, i5 = ops.map_crop_table(cap, dev)

        def crop():
            k2.fill_(-1)
            a2.zero_()
            ops.map_crop(vm.keys, vm.acc, poses[mid], vm.origin, vm.inv_cell, int(np.ceil(60.0 / cell)), k2, a2, i5)

        def rehash():
            k2.fill_(-1)
            a2.zero_()
            ops.map_rehash(vm.keys, vm.acc, k2, a2, i5[:4])

        def clear():
            k2.fill_(-1)
            a2.zero_()

        t_c, t_r, t_0 = _time(crop, a.iters), _time(rehash, a.iters), _time(clear, a.iters)
        i5.zero_()
        crop()
        c = i5.tolist()
        say(f"(c) lpd_map_crop to 60 m ({c[3]} cells kept, {c[4]} left behind) {(t_c - t_0) * 1e6:9.1f} us against lpd_map_rehash {(t_r - t_0) * 1e6:9.1f} us "
            f"(both without the {t_0 * 1e6:.1f} us that clear the new table)")
        # (d) the chain against the bare localisation of one scan
        sched = mapping.LocalizeSearch().schedule(cell)
        o1, p1 = off[mid:mid + 2], poses[mid:mid + 1].contiguous()
        t_l = _time(lambda: ops.map_localize(points, o1, p1, vm.origin, vm.inv_cell, vm.keys, full, sched, 50, 0.3), a.iters)
        say(f"(d) eight-step lpd_map_localize of one scan {t_l * 1e6:9.1f} us; the chain per scan = {t_chain['touched'] / t_l:.2f} x (touched), "
            f"{t_chain['full'] / t_l:.2f} x (full)")
        del vm, surf, full, dirty, k2, a2
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
