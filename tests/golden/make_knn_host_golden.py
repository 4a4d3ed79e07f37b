"""Writes tests/golden/knn_host_layout.npz: the host-side answers of the kNN entry points over the grid of
tests/test_front_of_searches_cpu.py (HOST_GRID) -- lpd_knn_workspace_floats, the regions of lpd_knn_pm_layout, lpd_knn_pm16_fused per
impl, lpd_morton_sort_knn_applies -- as the library selected with LPD_HIP_LIB gives them.  Run once, no GPU needed, against the
library built from the commit BEFORE the workspace layout and the route decision moved into csrc/lpd_knn_ws.h / KnnRoute:

    LPD_HIP_LIB=/path/to/parent/liblpd_hip.so python tests/golden/make_knn_host_golden.py

The library reads LPD_DEBUG once per process, so the second recording (LPD_DEBUG=no-knn-pre: the layout without the bound pass,
keys ending in _no_knn_pre) is made by a child process."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import test_front_of_searches_cpu as t  # noqa: E402
from lpdnet_hip import _lib  # noqa: E402

if __name__ == "__main__":
    assert os.environ.get("LPD_HIP_LIB"), "select the parent commit's library with LPD_HIP_LIB"
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        np.savez(sys.argv[2], **t.host_values(_lib.load()))
        sys.exit(0)
    assert "knn-pre" not in os.environ.get("LPD_DEBUG", "")
    out = t.host_values(_lib.load())
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "no_knn_pre.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=dict(os.environ, LPD_DEBUG="no-knn-pre"), check=True)
        with np.load(tmp) as z:
            out.update({name + "_no_knn_pre": z[name] for name in z.files})
    assert not np.array_equal(out["ws_floats"], out["ws_floats_no_knn_pre"]), "the switch did not reach the library"
    dst = sys.argv[1] if len(sys.argv) > 1 else t.HOST_GOLDEN
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(t.HOST_GRID), "grid points")
