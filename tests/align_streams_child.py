"""The body of tests/test_align_gpu.py::test_two_launches_and_two_streams_give_the_same_bits, run as a process of its own:
lpd_align_pairs twice on the current stream and once on each of two streams of its own, on the path that splits a pair's hypotheses
over workgroups (P = 25) and on the one-workgroup path (P = 600); all four results must hold the same bits.  Prints one line per path
and `OK` at the end; any difference is an AssertionError (exit status 1)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import align_ref as R  # noqa: E402
from lpdnet_hip import ops  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("align_streams_child: needs a GPU")
    dev = torch.device("cuda:0")
    g = np.random.default_rng(11)
    sc = R.scene(1)
    centre = g.uniform(-20, 20, 2)
    clouds = np.stack([R.submap(sc, centre + g.uniform(-2.5, 2.5, 2), g.uniform(0, 2 * np.pi), 100 + i) for i in range(6)])
    a, b = torch.from_numpy(clouds[:3]).to(dev), torch.from_numpy(clouds[3:]).to(dev)
    for P, H in ((25, 120), (600, 8)):
        pairs = torch.from_numpy(np.stack((g.integers(0, 3, P), g.integers(0, 3, P)), axis=1).astype(np.int32)).to(dev)
        rot = torch.from_numpy(R.rot_table(H)).to(dev)

        def launch():
            return ops.align_pairs(a, b, pairs, rot, H, 2.0, 8, 0.0, 0.5, 4)
        first, again = launch(), launch()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            r1 = launch()
        with torch.cuda.stream(s2):
            r2 = launch()
        torch.cuda.synchronize()
        for name, other in (("second launch", again), ("stream 1", r1), ("stream 2", r2)):
            assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1]), (P, H, name)
        assert int(first[0][:, 3].min()) > 0 and bool((first[0][:, 6] == 1).all())
        print(f"P={P} H={H}: four launches, the same bits; scores {int(first[0][:, 3].min())} .. {int(first[0][:, 3].max())}")
    print("OK")


if __name__ == "__main__":
    main()
