"""Writes tests/golden/knn_bound_table.npz: the bound table of the 64-channel kNN search for the seeded inputs of
tests/test_knn_bound_gpu.py, as the library selected with LPD_HIP_LIB writes it.  Run once on the GPU against the library built
from the commit BEFORE the candidate-tile loop of knn7_bound_kernel was pipelined:

    LPD_HIP_LIB=/path/to/parent/liblpd_hip.so python tests/golden/make_knn_bound_golden.py

so that the fixture records what the sequential kernel wrote.  The inputs are not stored: the test regenerates them from their
seeds and compares their SHA-256 with the one kept here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import test_knn_bound_gpu as t  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("LPD_HIP_LIB"), "select the parent commit's library with LPD_HIP_LIB"
    out = {}
    for name in t.GOLDEN_SHAPES:
        _, table = t.device_run(name)
        out["table_" + name] = np.array(table)
        out["input_sha256_" + name] = t.input_digest(t.cloud(name))
        print(name, table.shape, "+inf entries", int((table == t.INF_BITS).sum()))
    dst = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
