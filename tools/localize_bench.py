"""Timing of localisation against the drive map (csrc/lpd_localize.hip) on the 2 km sweep drive of tools/map_bench.py -- 400 scans x 65536
rows on surfaces in scanner order -- mapped at a cell of 0.2 m and of 1 m.

  (a) lpd_map_surface over the whole table.
  (b) lpd_map_localize: one pass (iters = 0) and the eight-step call, for 1 scan and for 32 scans of 65536 rows started a little off
      their mapped poses; lookups (27 a row with a cell) and probes (slots read, counted in torch by walking the same chains) per second,
      and the share of the 27 cells that are present.
  (c) beside them, in the same process: lpd_map_insert of the same rows into the filled table (the same address stream, with atomics
      instead of loads); lpd_icp_pairs (one pass) on the same rows cut into clouds of 16384 points against themselves (the brute-force
      search the map replaces); and a plain-torch rung of one pass -- sorted keys, searchsorted over the 27 neighbour keys, gathers of
      the centroids, the minimum, the rows' terms, index_add_ per scan.

    python tools/localize_bench.py [--iters 10] [--out profiles/localize_bench.txt]

Device figures are device time between two HIP events around `iters` back-to-back calls on one stream after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time).  Needs a GPU.
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

from drive_bench import make_poses  # noqa: E402
from map_bench import scan_line_points, world_rows  # noqa: E402
from submap_bench import _time  # noqa: E402

QLIM = 1 << 20
M64 = (1 << 64) - 1


def _lsr(x, n):
    """logical right shift of int64 words"""
    return (x >> n) & ((1 << (64 - n)) - 1)


def _i64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def slot_of(key, capacity):
    """lpd_map_slot in torch: the finaliser of splitmix64 (int64 products wrap as the uint64 ones do)"""
    x = key ^ _lsr(key, 30)
    x = x * _i64(0xbf58476d1ce4e5b9)
    x = x ^ _lsr(x, 27)
    x = x * _i64(0x94d049bb133111eb)
    x = x ^ _lsr(x, 31)
    return x & (capacity - 1)


def neighbour_keys(world, inv_cell):
    """world rows [n, 3] -> (key [n', 27] int64, -1 for a cell beyond the index range; the rows that have a cell)"""
    f = torch.floor(world * inv_cell)
    ok = ((f >= -float(QLIM)) & (f < float(QLIM))).all(dim=1)
    q = f[ok].to(torch.int64)
    d = torch.tensor([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], dtype=torch.int64, device=world.device)
    nq = q[:, None, :] + d[None, :, :]
    inside = ((nq >= -QLIM) & (nq < QLIM)).all(dim=2)
    nq = nq + QLIM
    key = nq[:, :, 0] | (nq[:, :, 1] << 21) | (nq[:, :, 2] << 42)
    return torch.where(inside, key, torch.full_like(key, -1)), ok


def count_probes(keys, nk):
    """the slots that the lookups of nk (>= 0) read in the table `keys`, and how many are found"""
    cap = keys.shape[0]
    k = nk[nk >= 0]
    s = slot_of(k, cap)
    live = torch.ones_like(k, dtype=torch.bool)
    found = torch.zeros_like(live)
    probes = 0
    for _ in range(min(cap, 128)):
        cur = keys[s]
        probes += int(live.sum())
        hit = live & (cur == k)
        found |= hit
        live = live & ~hit & (cur != -1)
        if not bool(live.any()):
            break
        s = (s + 1) & (cap - 1)
    return probes, int(found.sum()), int(k.numel())


def torch_pass(world, scan, S, g32, skeys, spts, snrm, sflat, inv_cell, dmax, max_flat):
    """one pass in plain torch on the world rows -> sums [S, 29] float64 (the rung does not quantise: it is a timing yardstick)"""
    nk, ok = neighbour_keys(world, inv_cell)
    w, sc = world[ok], scan[ok]
    j = torch.searchsorted(skeys, nk.clamp(min=0)).clamp(max=skeys.shape[0] - 1)
    present = (skeys[j] == nk) & (nk >= 0)
    c = spts[j]
    d2 = ((c - w[:, None, :]) ** 2).sum(dim=2)
    d2 = torch.where(present, d2, torch.full_like(d2, float("inf")))
    best, e = d2.min(dim=1)
    at = j.gather(1, e[:, None])[:, 0]
    n = snrm[at]
    has = (best <= dmax * dmax) & (n != 0).any(dim=1) & (sflat[at] <= max_flat)
    p, q, n, sc = (w - g32[sc])[has], (spts[at] - g32[sc])[has], n[has], sc[has]
    J = torch.cat((torch.cross(p, n, dim=1), n), dim=1).double()
    r = ((q - p) * n).sum(dim=1).double()
    iu = torch.triu_indices(6, 6, device=world.device)
    terms = torch.cat((torch.ones_like(r)[:, None], J[:, iu[0]] * J[:, iu[1]], J * r[:, None], (r * r)[:, None]), dim=1)
    return torch.zeros((S, 29), dtype=torch.float64, device=world.device).index_add_(0, sc, terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--metres", type=float, default=2000.0)
    ap.add_argument("--small", action="store_true", help="a tenth of the scans: a quick look, not the recorded figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("localize_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import drive, mapping, ops

    dev = torch.device("cuda:0")
    lines = [f"localize_bench: {a.metres:g} m sweep drive on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

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
    say(f"--- sweep, scan lines: {S} scans x {n} rows = {S * n} rows")
    rng = np.random.default_rng(3)
    start_h = poses_h.copy()      # the starts: up to 0.1 m and 0.3 degrees off the mapped poses
    start_h[:, [3, 7, 11]] += rng.uniform(-0.1, 0.1, (S, 3))
    yaw = rng.uniform(-0.005, 0.005, S)
    R = poses_h.reshape(S, 3, 4)[:, :, :3]
    Rz = np.stack([np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]]) for y in yaw])
    start_h.reshape(S, 3, 4)[:, :, :3] = Rz @ R
    start = torch.from_numpy(start_h).to(dev)

    for cell in (0.2, 1.0):
        vm = mapping.build_map(points, lengths, poses, cell=cell)
        cap, cells = vm.capacity, vm.occupied
        inv = vm.inv_cell
        say(f"  cell {cell:g} m: {cells} occupied cells in {cap} slots (load {cells / cap:.2f}); keys {8 * cap / 2 ** 20:.0f} MiB, surf "
            f"{32 * cap / 2 ** 20:.0f} MiB, acc {32 * cap / 2 ** 20:.0f} MiB")
        t_s = _time(lambda: ops.map_surface(vm.keys, vm.acc, 1, 5), a.iters)
        surf, sinfo = ops.map_surface(vm.keys, vm.acc, 1, 5)
        sinfo = sinfo.tolist()
        say(f"(a) lpd_map_surface, reach 1: {sinfo[0]} cells with a normal, {sinfo[1]} without            {t_s * 1e6:9.1f} us   "
            f"{cap / t_s / 1e9:6.2f} G slots/s   {27 * cells / t_s / 1e9:6.2f} G lookups/s")
        sc = vm.surface_cells()
        sched = mapping.LocalizeSearch().schedule(cell)
        for ns in (1, 32 // scale if scale > 1 else 32):
            rows = ns * n
            world = world_rows(points[:rows], lengths[:ns], start[:ns], vm.origin)
            nk, ok = neighbour_keys(world, inv)
            probes, found, lookups = count_probes(vm.keys, nk)
            del nk

            pts_n, off_n, start_n = points[:rows], off[:ns + 1].contiguous(), start[:ns].contiguous()

            def one_pass():
                return ops.map_localize(pts_n, off_n, start_n, vm.origin, inv, vm.keys, surf, sched[:1], 50, 0.3)

            def chain():
                return ops.map_localize(pts_n, off_n, start_n, vm.origin, inv, vm.keys, surf, sched, 50, 0.3)

            t_1 = _time(one_pass, a.iters)
            t_8 = _time(chain, a.iters)
            _, info, sums, _ = chain()
            info = info.cpu().numpy()
            say(f"(b) lpd_map_localize, {ns:2d} scans = {rows} rows: one pass / eight steps (nine passes)   {t_1 * 1e6:9.1f} / {t_8 * 1e6:9.1f} us   "
                f"{rows / t_1 / 1e9:6.2f} G rows/s   {lookups / t_1 / 1e9:6.2f} G lookups/s   {probes / t_1 / 1e9:6.2f} G probes/s "
                f"({probes / lookups:.2f} probes a lookup)   {found / lookups:.3f} of the 27 cells present; steps {int(info[:, 1].min())} .. "
                f"{int(info[:, 1].max())}, inlier share of the last pass {info[:, 3].min() / n:.3f} .. {info[:, 3].max() / n:.3f}")

            def insert():
                ops.map_insert(pts_n, off_n, poses[:ns].contiguous(), vm.origin, inv, vm.keys, vm.acc, vm.info)

            t_i = _time(insert, a.iters)
            say(f"(c) lpd_map_insert of the same rows into the filled table                         {t_i * 1e6:9.1f} us   "
                f"one pass = {t_1 / t_i:.2f} x the insert")
            N = 16384
            T = rows // N
            clouds = points[:rows].view(T, N, 3)
            nrm = torch.nn.functional.normalize(torch.randn((T, N, 3), device=dev), dim=2)
            pairs = torch.arange(T, dtype=torch.int32, device=dev)[:, None].expand(T, 2).contiguous()
            ident = torch.tensor([1.0, 0, 0, 0.01, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float64, device=dev).expand(T, 12).contiguous()
            t_p = _time(lambda: ops.icp_pairs(clouds, clouds, nrm, pairs, ident, (1.0,), 50), max(a.iters // 2, 2), warmup=2)
            say(f"(c) lpd_icp_pairs, one pass, {T} pairs of {N} points (brute force, {N} candidates a row)   {t_p * 1e6:9.1f} us   "
                f"= {t_p / t_1:.1f} x one pass against the map")
            scan = torch.repeat_interleave(torch.arange(ns, device=dev), n)
            g32 = (start[:ns][:, [3, 7, 11]] - vm.origin).float()
            t_t = _time(lambda: torch_pass(world, scan, ns, g32, sc.keys, sc.points, sc.normals, sc.flatness, inv, sched[0], 0.3), max(a.iters // 2, 2),
                        warmup=1)
            say(f"(c) plain torch, one pass on the world rows: searchsorted x 27, gathers, index_add_    {t_t * 1e6:9.1f} us   "
                f"= {t_t / t_1:.1f} x one pass of the kernel")
            del world, clouds, nrm, scan
            torch.cuda.empty_cache()
        del vm, surf, sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
