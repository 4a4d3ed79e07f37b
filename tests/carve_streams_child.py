"""The body of tests/test_carve_gpu.py::test_two_streams_on_two_tables, run as a process of its own: lpd_map_pierce on the current
stream and on each of two streams of its own, against two tables of different capacity; every result must equal the restatement per
key, and the carved table and the flags made from the second stream's counts too.  Prints one line and `OK` at the end; any difference
is an AssertionError (exit status 1)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import test_carve_gpu as T  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("carve_streams_child: needs a GPU")
    pierces = T.streams_body(torch.device("cuda:0"))
    print(f"three launches, two streams, two tables: the restatement's counts per key; {pierces} pierces")
    print("OK")


if __name__ == "__main__":
    main()
