"""Shared by tests/test_front_of_searches_gpu.py and the fresh interpreter it starts with the folds switched off: the eval forwards whose
descriptors the two must agree on, bit for bit.   python tests/front_of_searches_ref.py OUT.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def forwards():
    """LPD-Net eval descriptors at N = 4096: 2 clouds (the small-batch route: split searches, second stream, launch replay on the
    repeat), and two batches of 32 clouds in flight on two HIP streams (the benched shape) -> dict of numpy arrays"""
    import torch
    from oracle import lpd_oracle as orc, synth
    from util.PointNetVlad import PointNetVlad
    dev = torch.device("cuda:0")
    m = PointNetVlad(num_points=4096, featnet="lpdnet")
    m.load_state_dict(orc.synthetic_state("lpdnet", num_points=4096))
    m = m.to(dev).eval()
    x = torch.from_numpy(synth.cloud(41, 66, 4096)).unsqueeze(1).to(dev)
    out = {}
    with torch.no_grad():
        out["b2"] = m(x[64:66]).cpu().numpy()
        out["b2_again"] = m(x[64:66]).cpu().numpy()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for rep in range(2):
            got = []
            for j, s in enumerate(streams):
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    got.append(m(x[32 * j:32 * j + 32]))
            torch.cuda.synchronize()
            for j, g in enumerate(got):
                out[f"b32_stream{j}_rep{rep}"] = g.cpu().numpy()
    return out


if __name__ == "__main__":
    import numpy as np
    np.savez(sys.argv[1], **forwards())
