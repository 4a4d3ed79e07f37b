"""Timing of the local point-distribution features (csrc/lpd_feat.hip, lpdnet_hip/features.py) at 32 clouds x 4096 points:

  (a) the xyz kNN that feeds the kernel, K = 20 and K = 32;
  (b) the feature kernel, fixed k = 20 and adaptive (candidates 8, 12, .., 32 on K = 32 lists), with the achieved bytes/s on its
      algorithmic bytes M (4 K + 12 + 4 columns): the index lists and the coordinates read once, the selected columns written once;
  (c) the eval forward of a use_mFea model fed a precomputed 8-column batch against the same model inside LocalFeatureInput
      (Z-order + kNN + features + forward);
  (d) for orientation, the plain xyz-only model.

    python tools/local_features_bench.py [--clouds 32] [--points 4096] [--iters 200] [--out profiles/local_features_bench.txt]

Every figure is device time between two HIP events around `iters` back-to-back calls on one stream, after warm-up calls of the same
shape, divided by `iters`: call time in a full stream, launch gaps included, not a profiler's kernel time.  Synthetic clouds
(oracle/synth.py), Z-ordered as the product orders them.  Needs a GPU: there is no CPU timing.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CANDIDATES = (8, 12, 16, 20, 24, 28, 32)


def _time(fn, iters, warmup=10):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--model-iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("local_features_bench: needs a GPU (no CPU timing)")
    from lpdnet_hip import engine, features, ops
    from oracle import lpd_oracle as orc
    from oracle import synth
    from util.PointNetVlad import PointNetVlad

    dev = torch.device("cuda:0")
    B, N = a.clouds, a.points
    M = B * N
    x = engine.reorder_points(torch.from_numpy(synth.cloud(11, B, N)).unsqueeze(1).to(dev))      # [B,1,N,3], Z-ordered
    rows = x.view(M, 3)
    lines = [f"local_features_bench: {B} clouds x {N} points on {torch.cuda.get_device_name(0)}; device events around {a.iters} calls"]

    def say(s):
        print(s)
        lines.append(s)

    t_knn = {}
    for K in (20, 32):
        t_knn[K] = _time(lambda: ops.knn_pm(rows, B, N, K), a.iters)
        say(f"(a) xyz kNN              K={K:2d}                 {t_knn[K] * 1e6:8.1f} us")
    idx = {K: ops.knn_pm(rows, B, N, K) for K in (20, 32)}
    for label, K, cand, cols, copy in (("fixed k=20, 10 columns", 20, None, range(10), False),
                                       ("fixed k=20, xyz + 5 cols", 20, None, features.DEFAULT_COLUMNS, True),
                                       ("adaptive 8..32, 10 columns", 32, CANDIDATES, range(10), False),
                                       ("adaptive 8..32, xyz + 5", 32, CANDIDATES, features.DEFAULT_COLUMNS, True)):
        ncol = len(list(cols)) + (3 if copy else 0)
        out = torch.empty((M, ncol), device=dev)
        t = _time(lambda: ops.local_features(rows, idx[K], B, N, candidates=cand, columns=cols, copy_xyz=copy, out=out), a.iters)
        nbytes = M * (4 * K + 12 + 4 * ncol)
        say(f"(b) features {label:27s} {t * 1e6:8.1f} us  {nbytes / 1e6:6.1f} MB algorithmic = {nbytes / t / 1e9:7.1f} GB/s"
            f"  ({t / t_knn[K]:.2f} x the K={K} kNN)")
    t = _time(lambda: features.append_local_features(x, zorder=True), a.iters)
    say(f"    append_local_features(zorder=True): Z-order + kNN(20) + kernel {t * 1e6:8.1f} us")

    def model(use_mfea):
        m = PointNetVlad(num_points=N, featnet="lpdnet")
        if use_mfea:
            features.convert_to_local_features(m)
        m.load_state_dict(orc.synthetic_state("lpdnet", num_points=N, use_mFea=use_mfea), strict=True)
        return m.to(dev).eval()

    with torch.no_grad():
        m8, m3 = model(True), model(False)
        w8 = features.LocalFeatureInput(m8).eval()
        x8 = features.append_local_features(x, zorder=True)
        t8 = _time(lambda: m8(x8), a.model_iters, warmup=5)
        tw = _time(lambda: w8(x), a.model_iters, warmup=5)
        t3 = _time(lambda: m3(x), a.model_iters, warmup=5)
    say(f"(c) eval forward, use_mFea model, precomputed [B,1,N,8] input  {t8 * 1e3:7.3f} ms")
    say(f"(c) eval forward, the same model inside LocalFeatureInput      {tw * 1e3:7.3f} ms  (+{(tw - t8) * 1e6:.0f} us)")
    say(f"(d) eval forward, xyz-only model                               {t3 * 1e3:7.3f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
