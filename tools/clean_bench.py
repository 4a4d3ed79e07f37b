"""Timing of the road removal in front of the submaps (csrc/lpd_clean.hip, lpdnet_hip/submap.py): 32 scans x 65536 points.

  (a) the launches: lpd_road_planes at H = 0 (the row passes alone: hypotheses' table + live count), 64, 256, 1024, with and without the
      refinement round; lpd_clean_count, the torch.cumsum between them, lpd_clean_fill; ops.clean_scans (the three together);
  (b) the route it replaces: a z-threshold mask through submap.filter_scans (plain torch, one read-back) and then make_submaps;
  (c) submap.make_submaps with and without clean=, on the same device tensor with host lengths;
  (d) the eval forward of the 32 submaps that (c) produced, the consumer.

    python tools/clean_bench.py [--scans 32] [--points 65536] [--num-points 4096] [--iters 200] [--out profiles/clean_bench.txt]

Every figure is device time between two HIP events around `iters` back-to-back calls on one stream, after warm-up calls of the same
shape, divided by `iters` (tools/submap_bench.py's _time): call time in a full stream, launch gaps included, not a profiler's kernel
time.  The scans are tools/submap_bench.py's synthetic ones (half road).  Needs a GPU: there is no CPU timing.
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

from submap_bench import _time, synthetic_scan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--num-points", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--model-iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clean_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import ops, submap
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad

    dev = torch.device("cuda:0")
    B, n, N = a.scans, a.points, a.num_points
    lines = [f"clean_bench: {B} scans x {n} points on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    points = torch.from_numpy(np.concatenate([synthetic_scan(n, 100 + b) for b in range(B)], 0)).to(dev)
    lengths = [n] * B
    off = torch.arange(B + 1, dtype=torch.int32, device=dev) * n
    evals = B * n

    # (a) the launches
    t0 = None
    for H in (0, 64, 256, 1024):
        for refine in ((0,) if H == 0 else (0, 1)):
            prm = submap.RoadRemoval(H=H, refine=refine).c_params()
            t = _time(lambda: ops.road_planes(points, off, B, n, prm), a.iters)
            if H == 0:
                t0 = t
                say(f"(a) lpd_road_planes  H =    0 (row passes alone)            {t * 1e6:9.1f} us")
            else:
                say(f"(a) lpd_road_planes  H = {H:4d} refine = {refine}                    {t * 1e6:9.1f} us   "
                    f"({evals * H / max(t - t0, 1e-9) / 1e12:.2f} T evaluations/s over the H = 0 time)")
    clean = submap.RoadRemoval()
    prm = clean.c_params()
    plane, info = ops.road_planes(points, off, B, n, prm)
    inf = info.cpu()
    chunks = (n + ops.CLEAN_CHUNK - 1) // ops.CLEAN_CHUNK
    counts = torch.empty((B * chunks,), dtype=torch.int32, device=dev)
    boff = torch.zeros((B * chunks + 1,), dtype=torch.int32, device=dev)
    out = torch.empty((B * n, 3), device=dev)
    ooff = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    lib = ops._lib.load()
    p = ops._ptr
    import ctypes
    head = (p(points), 3, B * n, p(off), B, n, ctypes.byref(prm), p(plane), p(info))
    t_c = _time(lambda: lib.lpd_clean_count(*head, p(counts), ops._stream()), a.iters)
    t_s = _time(lambda: torch.cumsum(counts, 0, dtype=torch.int32, out=boff[1:]), a.iters)
    t_f = _time(lambda: lib.lpd_clean_fill(*head, p(boff), p(out), p(ooff), None, ops._stream()), a.iters)
    kept = int(ooff[-1])
    say(f"(a) lpd_clean_count / torch.cumsum / lpd_clean_fill           {t_c * 1e6:9.1f} / {t_s * 1e6:.1f} / {t_f * 1e6:.1f} us   "
        f"({kept} of {B * n} rows kept; inliers {int(inf[:, 3].min())}..{int(inf[:, 3].max())} per scan)")
    t_cs = _time(lambda: ops.clean_scans(points, off, B, n, prm, plane, info), a.iters)
    t_all = _time(lambda: submap.clean_scans(points, lengths, clean), a.iters)
    say(f"(a) ops.clean_scans (count + cumsum + fill, allocations)      {t_cs * 1e6:9.1f} us")
    say(f"(a) submap.clean_scans (planes + compaction), defaults        {t_all * 1e6:9.1f} us")

    # (b) the route it replaces
    def old_route():
        pts, lens = submap.filter_scans(points, lengths, points[:, 2] > -1.4)
        return submap.make_submaps(pts, lens, N)
    t_old_f = _time(lambda: submap.filter_scans(points, lengths, points[:, 2] > -1.4), max(a.iters // 4, 5))
    t_old = _time(old_route, max(a.iters // 4, 5))
    say(f"(b) filter_scans with a z-threshold mask (one read-back)      {t_old_f * 1e6:9.1f} us")
    say(f"(b) filter_scans + make_submaps (check_finite waits again)    {t_old * 1e6:9.1f} us")

    # (c) make_submaps with and without clean=
    t_plain = _time(lambda: submap.make_submaps(points, lengths, N, check_finite=False), a.iters)
    t_clean = _time(lambda: submap.make_submaps(points, lengths, N, clean=clean), a.iters)
    t_k = _time(lambda: ops._make_submaps(points, off, B, N, True, False, None), a.iters)
    say(f"(c) make_submaps, no clean (check_finite=False) / kernel      {t_plain * 1e6:9.1f} / {t_k * 1e6:.1f} us")
    say(f"(c) make_submaps(clean=RoadRemoval())                         {t_clean * 1e6:9.1f} us   "
        f"(cleaning = {t_all / t_k:.2f} x the submap kernel on the raw scans)")

    # (d) the consumer
    m = PointNetVlad(num_points=N, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
    m = m.to(dev).eval()
    x = submap.make_submaps(points, lengths, N, clean=clean).x
    with torch.no_grad():
        t_fw = _time(lambda: m(x), a.model_iters, warmup=5)
    say(f"(d) eval forward of the {B} cleaned submaps                    {t_fw * 1e6:9.1f} us   (cleaning = {t_all / t_fw:.3f} x the forward)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
