"""Timing of the raw-scan submaps (csrc/lpd_submap.hip, lpdnet_hip/submap.py): 32 scans x 65536 points -> 4096 points each, and 1 scan.

  (a) the kernel: ops._make_submaps on device tensors (one launch, one 1024-thread workgroup per scan);
  (b) the whole submap.make_submaps call on a concatenated device tensor with host lengths (offsets upload, finite check, launch),
      with and without check_finite;
  (c) yardstick 1: a plain-torch device formulation of ONE rung of the ladder -- keys, torch.unique(return_inverse=True),
      index_add_ of the coordinate sums and counts -- where the kernel walks seven or eight rungs and then averages;
  (d) yardstick 2: the eval forward of the batch of submaps that (a) produced, the consumer the kernel feeds.

    python tools/submap_bench.py [--scans 32] [--points 65536] [--num-points 4096] [--iters 200] [--out profiles/submap_bench.txt]

Every figure is device time between two HIP events around `iters` back-to-back calls on one stream, after warm-up calls of the same
shape, divided by `iters`: call time in a full stream, launch gaps included, not a profiler's kernel time.  Synthetic scans (ground
disc + wall + clutter to 50 m, seeded).  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters      # seconds per call


def synthetic_scan(n, seed):
    rng = np.random.default_rng(seed)
    ng, nw = n // 2, n // 4
    nc = n - ng - nw
    r, a = 50.0 * np.sqrt(rng.random(ng)), 2 * np.pi * rng.random(ng)
    ground = np.stack((r * np.cos(a), r * np.sin(a), -1.7 + 0.03 * rng.standard_normal(ng)), axis=1)
    wall = np.stack((-40 + 80 * rng.random(nw), 12.0 + 0.05 * rng.standard_normal(nw), -1.7 + 8 * rng.random(nw)), axis=1)
    centres = rng.uniform((-45, -45, -1.5), (45, 45, 2.0), size=(24, 3))
    clutter = centres[rng.integers(0, 24, nc)] + rng.standard_normal((nc, 3)) * (0.8, 0.8, 0.5)
    pts = np.concatenate((ground, wall, clutter), 0)
    return np.ascontiguousarray(pts[rng.permutation(n)], dtype=np.float32)


def torch_one_rung(points, B, n, cells):
    """One rung in plain torch for B scans of n points each: per-scan box, `cells` cells per extent, unique cells, their averages."""
    x = points.view(B, n, 3)
    mn = x.amin(dim=1, keepdim=True)
    E = (x.amax(dim=1, keepdim=True) - mn).amax(dim=2, keepdim=True)
    q = ((x - mn) * (cells / E)).clamp_(0, 1023).to(torch.int64)
    key = q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (torch.arange(B, device=x.device).view(B, 1) << 30)
    uniq, inv = torch.unique(key.view(-1), return_inverse=True)
    sums = torch.zeros((uniq.numel(), 3), device=x.device).index_add_(0, inv, points)
    cnt = torch.zeros((uniq.numel(),), device=x.device).index_add_(0, inv, torch.ones_like(points[:, 0]))
    return sums / cnt[:, None]


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
        raise SystemExit("submap_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import ops, submap
    from oracle import lpd_oracle as orc
    from util.PointNetVlad import PointNetVlad

    dev = torch.device("cuda:0")
    B, n, N = a.scans, a.points, a.num_points
    lines = [f"submap_bench: {B} scans x {n} points -> {N} on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    points = torch.from_numpy(np.concatenate([synthetic_scan(n, 100 + b) for b in range(B)], 0)).to(dev)
    results = {}
    for nb in (B, 1):
        pts = points[:nb * n]
        lengths = [n] * nb
        off = torch.arange(nb + 1, dtype=torch.int32, device=dev) * n
        out = torch.empty((nb, N, 3), device=dev)
        res = ops._make_submaps(pts, off, nb, N, True, False, out)
        info = res[1].cpu()
        t_k = _time(lambda: ops._make_submaps(pts, off, nb, N, True, False, out), a.iters)
        t_c = _time(lambda: submap.make_submaps(pts, lengths, N), a.iters)
        t_n = _time(lambda: submap.make_submaps(pts, lengths, N, check_finite=False), a.iters)
        mb = nb * n * 12 / 1e6
        say(f"(a) kernel, {nb:2d} scan(s)                                  {t_k * 1e6:9.1f} us   ({mb:.1f} MB of points, "
            f"levels {int(info[:, 0].min())}..{int(info[:, 0].max())}, cells {int(info[:, 1].min())}..{int(info[:, 1].max())})")
        say(f"(b) submap.make_submaps, {nb:2d} scan(s)                     {t_c * 1e6:9.1f} us   (check_finite=False: {t_n * 1e6:.1f} us)")
        results[nb] = t_k
        if nb == B:
            level = int(info[0, 0])
            cells = 1024.0 * 2.0 ** (-level / 16.0)
            t_t = _time(lambda: torch_one_rung(pts, nb, n, cells), max(a.iters // 10, 5), warmup=3)
            say(f"(c) plain torch, ONE rung (unique + index_add_), {nb} scans  {t_t * 1e6:9.1f} us   ({t_t / t_k:.2f} x the kernel)")
            m = PointNetVlad(num_points=N, featnet="lpdnet")
            m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N), strict=True)
            m = m.to(dev).eval()
            x = out.view(nb, 1, N, 3)
            with torch.no_grad():
                t_f = _time(lambda: m(x), a.model_iters, warmup=5)
            say(f"(d) eval forward of the {nb} submaps                        {t_f * 1e6:9.1f} us   (kernel = {t_k / t_f:.2f} x the forward)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
