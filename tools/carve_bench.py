"""Timing of the moving-object stage (csrc/lpd_carve.hip) on the 2 km sweep drive of tools/localize_bench.py -- 400 scans x 65536 rows on
surfaces in scanner order -- mapped at a cell of 0.2 m and of 1 m.

  (a) lpd_map_pierce of 1 scan and of 32 scans against the whole map at the defaults of mapping.Carve: rays, cells stepped into and
      lookups per second (the lookups are counted by the torch rung on the first scan and scaled by the cells stepped into).
  (b) beside it, in the same process: one pass of lpd_map_localize on the same rows (27 lookups a row; profiles/localize_bench.txt holds
      82 / 211 G lookups/s for it at 0.2 m / 1 m) and lpd_map_insert of the same rows.
  (c) lpd_map_carve over the whole table and lpd_scan_moving of the same rows.
  (d) a plain-torch rung of the pierce count on one scan: the same integer walk with all rays stepped together, searchsorted over sorted
      keys, gathers of the surf rows, the rule, index_add_.
  (e) mapping.remove_moving of the first 32 scans end to end (host time, with its read-backs) beside mapping.build_map of the same scans.

    python tools/carve_bench.py [--iters 10] [--out profiles/carve_bench.txt]

Device figures are device time between two HIP events around `iters` back-to-back calls on one stream after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time).  Needs a GPU.
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
from map_bench import scan_line_points, world_rows  # noqa: E402
from submap_bench import _time  # noqa: E402

QLIM = 1 << 20


def _key(q):
    q = q + QLIM
    return q[:, 0] | (q[:, 1] << 21) | (q[:, 2] << 42)


def torch_pierce(world, sensor, inv_cell, skeys, srows, carve, cell):
    """the pierce count of rays sensor -> world [n, 3] in plain torch -> (counts per sorted key, cells stepped into, lookups, found, pierces).
    The walk is the kernel's, in int64; the rule is evaluated in float64 without the kernel's rounding order (a timing yardstick)."""
    f, e = world * inv_cell, (sensor * inv_cell).expand_as(world)
    A = 2 * torch.floor(f.double() * 256.0).to(torch.int64) + 1
    B = 2 * torch.floor(e.double() * 256.0).to(torch.int64) + 1
    qa, q = A >> 9, B >> 9
    qb = q.clone()
    D = A - B
    s = torch.sign(D)
    N = (512 * (q + (s > 0)) - B).abs()
    D = D.abs()
    vis = ((qa - q).abs().sum(dim=1) - 1).clamp(0, carve.max_steps)
    at_e = torch.searchsorted(skeys, _key(qa)).clamp(max=skeys.shape[0] - 1)
    has_e = skeys[at_e] == _key(qa)
    erow = srows[at_e].double()
    e_rel = has_e & (erow[:, 3:6] != 0).any(dim=1) & (erow[:, 6] <= carve.max_flat)
    o, w = sensor.double().expand_as(world), world.double()
    clr, rad = carve.clearance * cell, carve.radius * cell
    counts = torch.zeros(skeys.shape[0], dtype=torch.int64, device=world.device)
    big = torch.iinfo(torch.int64).max
    steps = lookups = found = pierces = 0
    act = torch.nonzero(vis > 0)[:, 0]
    step = 0
    while act.numel():
        n_, d_ = N[act], D[act]
        t = torch.where(d_ != 0, n_, torch.full_like(n_, big))
        b = torch.zeros_like(act)
        for c in (1, 2):      # the smallest N_c / D_c by cross-multiplication, ties to the lowest axis
            nb, db = t.gather(1, b[:, None])[:, 0], d_.gather(1, b[:, None])[:, 0]
            take = (d_[:, c] != 0) & ((db == 0) | (n_[:, c] * db < nb * d_[:, c]))
            b = torch.where(take, torch.full_like(b, c), b)
        q[act, b] += s[act, b]
        N[act, b] += 512
        steps += int(act.numel())
        qq = q[act]
        see = ((qq - qa[act]).abs().amax(dim=1) >= carve.skip_end) & ((qq - qb[act]).abs().amax(dim=1) >= carve.skip_start)
        ray = act[see]
        k = _key(qq[see])
        lookups += int(k.numel())
        j = torch.searchsorted(skeys, k).clamp(max=skeys.shape[0] - 1)
        hit = skeys[j] == k
        ray, j = ray[hit], j[hit]
        found += int(j.numel())
        row = srows[j].double()
        c3, n3 = row[:, :3], row[:, 3:6]
        part1 = ~e_rel[ray] | (((erow[ray, 3:6] * (c3 - w[ray])).sum(dim=1)).abs() > clr)
        g, h = (n3 * (o[ray] - c3)).sum(dim=1), (n3 * (w[ray] - c3)).sum(dim=1)
        plane = ((g > clr) & (h < -clr)) | ((g < -clr) & (h > clr))
        v, a = w[ray] - o[ray], c3 - o[ray]
        aa, vv, av = (a * a).sum(dim=1), (v * v).sum(dim=1), (a * v).sum(dim=1)
        near = (aa * vv - av * av) < (rad * rad) * vv
        rel = (n3 != 0).any(dim=1) & (row[:, 6] <= carve.max_flat)
        ok = part1 & torch.where(rel, plane, near)
        counts.index_add_(0, j[ok], torch.ones_like(j[ok]))
        pierces += int(ok.sum())
        step += 1
        act = act[vis[act] > step]
    return counts, steps, lookups, found, pierces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carve_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, mapping, ops

    dev = torch.device("cuda:0")
    lines = [f"carve_bench: {a.metres:g} m sweep drive on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

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
    carve = mapping.Carve()
    say(f"--- sweep, scan lines: {S} scans x {n} rows = {S * n} rows; {carve!r}")
    for cell in (0.2, 1.0):
        vm = mapping.build_map(points, lengths, poses, cell=cell)
        cap, cells, inv = vm.capacity, vm.occupied, vm.inv_cell
        surf = vm.surface(carve.reach, carve.min_cells)
        say(f"  cell {cell:g} m: {cells} occupied cells in {cap} slots (load {cells / cap:.2f})")
        prm = (carve.clearance * cell, carve.radius * cell, carve.skip_end, carve.skip_start, carve.max_steps, carve.max_flat)
        looked_share = None
        for ns in (1, 32 // scale if scale > 1 else 32):
            rows = ns * n
            pts_n, off_n, poses_n = points[:rows], off[:ns + 1].contiguous(), poses[:ns].contiguous()
            pierce = torch.zeros((cap,), dtype=torch.int32, device=dev)
            info = torch.zeros((6,), dtype=torch.int64, device=dev)
            ops.map_pierce(pts_n, off_n, poses_n, vm.origin, inv, vm.keys, surf, *prm, pierce=pierce, info=info)
            rays, dropped, cut, steps, found, hits = info.tolist()
            scratch = torch.zeros_like(pierce)
            t_p = _time(lambda: ops.map_pierce(pts_n, off_n, poses_n, vm.origin, inv, vm.keys, surf, *prm, pierce=scratch), a.iters)
            if ns == 1:
                sc = vm.surface_cells(carve.reach, carve.min_cells)
                srows = torch.cat((sc.points, sc.normals, sc.flatness[:, None]), dim=1)
                world = world_rows(pts_n, lengths[:1], poses_n, vm.origin)
                sensor = (poses_n[0, [3, 7, 11]] - vm.origin).float()[None, :]
                t0 = time.perf_counter()
                tc, tsteps, tlook, tfound, thits = torch_pierce(world, sensor, inv, sc.keys, srows, carve, cell)
                torch.cuda.synchronize()
                t_t = time.perf_counter() - t0
                looked_share = tlook / max(tsteps, 1)
                say(f"(d) plain torch, 1 scan: the walk of all rays together, searchsorted, gathers, index_add_    {t_t * 1e6:11.1f} us   = "
                    f"{t_t / t_p:.0f} x the kernel ({tsteps} cells stepped into, {tlook} lookups, {tfound} found, {thits} pierces; the kernel: "
                    f"{steps} / {found} / {hits})")
                del world, srows, sc, tc
            lookups = steps * looked_share
            say(f"(a) lpd_map_pierce, {ns:2d} scans = {rows} rows: {rays} rays, {dropped} dropped, {cut} cut; {steps / max(rays, 1):.1f} cells a ray, "
                f"{found / max(steps, 1):.3f} found, {hits} pierces   {t_p * 1e6:9.1f} us   {rays / t_p / 1e9:6.3f} G rays/s   "
                f"{steps / t_p / 1e9:6.2f} G cells/s   {lookups / t_p / 1e9:6.2f} G lookups/s")
            sched = mapping.LocalizeSearch().schedule(cell)
            t_1 = _time(lambda: ops.map_localize(pts_n, off_n, poses_n, vm.origin, inv, vm.keys, surf, sched[:1], 50, 0.3), a.iters)
            say(f"(b) lpd_map_localize, one pass on the same rows (27 lookups a row)                    {t_1 * 1e6:9.1f} us   "
                f"{27 * rows / t_1 / 1e9:6.2f} G lookups/s   the pierce count = {t_p / t_1:.1f} x one pass")
            flags = torch.zeros((points.shape[0],), dtype=torch.uint8, device=dev)
            t_m = _time(lambda: ops.scan_moving(pts_n, off_n, poses_n, vm.origin, inv, vm.keys, vm.acc, pierce, carve.min_pierce, carve.ratio_q,
                                                flags=flags[:rows]), a.iters)
            say(f"(c) lpd_scan_moving of the same rows                                                  {t_m * 1e6:9.1f} us   "
                f"{rows / t_m / 1e9:6.2f} G rows/s   {int(flags[:rows].sum())} rows flagged")
            if ns > 1:
                keys2, acc2, _, info5 = ops.map_crop_table(cap, dev)

                def carve_call():
                    keys2.fill_(-1)
                    acc2.zero_()
                    ops.map_carve(vm.keys, vm.acc, pierce, carve.min_pierce, carve.ratio_q, keys2, acc2, info5)

                def clear_only():
                    keys2.fill_(-1)
                    acc2.zero_()

                t_c, t_0 = _time(carve_call, a.iters), _time(clear_only, a.iters)
                info5.zero_()
                carve_call()
                say(f"(c) lpd_map_carve over {cap} slots ({int(info5[4])} cells left behind of {cells}; without the two fills)   "
                    f"{(t_c - t_0) * 1e6:9.1f} us   {cap / max(t_c - t_0, 1e-9) / 1e9:6.2f} G slots/s")
                del keys2, acc2
            # last, and into a copy: the repeats add rows to the table they time, which would spoil the counts printed above
            keys_c, acc_c, info_c = vm.keys.clone(), vm.acc.clone(), vm.info.clone()
            t_i = _time(lambda: ops.map_insert(pts_n, off_n, poses_n, vm.origin, inv, keys_c, acc_c, info_c), a.iters)
            say(f"(b) lpd_map_insert of the same rows into a copy of the filled table                   {t_i * 1e6:9.1f} us")
            del keys_c, acc_c, info_c
        del vm, surf
        torch.cuda.empty_cache()
        ns = 32 // scale if scale > 1 else 32
        rows = ns * n
        for name, fn in (("build_map", lambda: mapping.build_map(points[:rows], lengths[:ns], poses[:ns], cell=cell)),
                         ("remove_moving", lambda: mapping.remove_moving(points[:rows], lengths[:ns], poses[:ns], cell=cell, carve=carve))):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            extra = f"; {out[2].rows_removed} rows and {out[2].cells_removed} cells removed" if name == "remove_moving" else ""
            say(f"(e) mapping.{name} of {ns} scans = {rows} rows, host time with its read-backs{extra}   {dt * 1e3:9.2f} ms")
            del out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
