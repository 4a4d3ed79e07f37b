"""Every route of the A^T B and bf16-storage products (csrc/lpd_train2.hip: lpd_gemm_tn, lpd_gemm_tn_act, lpd_gemm_tn_bf16, lpd_gemm_bf16s;
csrc/lpd_train3.hip: lpd_edge_dw_sel_bf16 / _f32) per element against float64 on the CPU, at the smallest shape its route allows.
tests/tn_routes.py holds the table of cases and says which kernel instance, how many slabs and how many products per term each one runs;
tests/tn_checks.py makes the inputs, the references and the number-format terms (its docstring derives them) and
tests/test_tn_routes_cpu.py holds all of that to the sources.

Each case
  - calls the lpdnet_hip.ops wrapper with ops.PROFILE set and asserts the label of the case;
  - places the operands of lpd_gemm_tn as column slices of wider buffers (lda != KA): one fp32 buffer [A | B] for fp32 rows, one buffer
    per type otherwise, 2 guard rows above and below every problem of a batch.  Every column around the slices, every guard row and
    every row past `rows` holds 2^100: a correct kernel never lets one reach a sum, and check_bound refuses a non-finite result
    (lpd_gemm_tn_bf16, lpd_gemm_bf16s and the edge entries take contiguous tensors only; W2 of the edge entries is a slice);
  - compares with float64 through fp64_checks.check_bound and prints `MEASURE tn/<case> err= floor= bound=`.
A case that names LPD_DEBUG switches runs in a child interpreter, one child per switch set (the library reads the switches once per
process): the child makes the same seeded inputs, runs the cases of its set and hands the results back on the CPU; the parent computes
the references and checks.  A child that faults, aborts or runs out of time fails every case of its set; nothing runs it again.
"""
import os
import subprocess
import sys

import pytest
import torch

import tn_checks as tc
import tn_routes as tr
from fp64_checks import check_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240      # torch + HIP start-up and at most six launches of a few milliseconds; the largest set moves 150 MB to the device


def _ops():
    from lpdnet_hip import ops
    return ops


def _big(shape, dtype, dev):
    return torch.full(shape, tc.BIG, dtype=dtype, device=dev)


def _slices(c, d, dev):
    """A [nb, M (+ extra), KA] and B [.., KB] on the device as column slices of wider buffers; 2-D when nb == 1"""
    nb, M, KA, KB, R = c["nb"], c["M"], c["KA"], c["KB"], c["M"] + c["extra"]
    G = 2
    a16, b16 = c["a16"], c["b16"]

    def put(buf, x, col):
        buf[:, G:G + M, col:col + x.shape[2]] = x.to(dev).to(buf.dtype)
        return buf[:, G:G + R, col:col + x.shape[2]]

    if not a16 and not b16:
        wide = _big((nb, R + 2 * G, 4 + KA + KB + 4), torch.float32, dev)
        A, B = put(wide, d["A"], 4), put(wide, d["B"], 4 + KA)
    else:
        A = put(_big((nb, R + 2 * G, 8 + KA + 8), torch.bfloat16 if a16 else torch.float32, dev), d["A"], 8)
        B = put(_big((nb, R + 2 * G, 8 + KB + 8), torch.bfloat16 if b16 else torch.float32, dev), d["B"], 8)
    assert A.stride(1) != KA and B.stride(1) != KB
    return (A[0], B[0]) if nb == 1 else (A, B)


_DEVICE_LOST = []      # why no further case of this process may touch the device
_FAULT_WORDS = ("illegal memory access", "hiperror", "hip error", "launch failure", "device-side", "hardware exception")


def run_case(ops, c, d, dev):
    """-> (result on the device, the PROFILE labels of the call); after a device fault every later case fails without a launch"""
    if _DEVICE_LOST:
        pytest.fail("not run: " + _DEVICE_LOST[0])
    try:
        return _run_case(ops, c, d, dev)
    except Exception as exc:      # noqa: BLE001
        if any(w in str(exc).lower() for w in _FAULT_WORDS):
            _DEVICE_LOST.append(f"{c['name']} faulted the device ({str(exc).splitlines()[0][:200]})")
        raise


def _run_case(ops, c, d, dev):
    w = c["wrapper"]
    prof = ops.PROFILE = {}
    try:
        if w == "gemm_tn":
            A, B = _slices(c, d, dev)
            aff = (d["a_sc"].to(dev), d["a_sh"].to(dev), tc.LEAKY, tc.T_SLOPE) if c["affine"] else None
            got = ops.gemm_tn(A, B, rows=c["M"] if c["extra"] else None, a_affine=aff)
        elif w == "pool_tn":
            got = ops.pool_tn(d["A"].to(dev), d["B"].to(dev))
            assert got is not None, "ops.pool_tn declined"
        elif w == "gemm_tn_bf16":
            got = ops.gemm_tn_bf16(d["A"][0].to(dev).bfloat16(), d["B"][0].to(dev).bfloat16())
        elif w == "gemm_bf16s":
            W = d["W"] if c["b_kmajor"] else d["W"].t().contiguous()
            got = ops.gemm_bf16s(d["A"].to(dev).bfloat16(), W.to(dev), b_kmajor=c["b_kmajor"])
            assert got.dtype == torch.bfloat16
        else:
            dt = torch.bfloat16 if c["a16"] else torch.float32
            wide = _big((128, 4 + 128 + 4), torch.float32, dev)
            wide[:, 4:132] = d["W2"].to(dev)
            st = ops.BNStats(d["scale"].to(dev), None, d["mean"].to(dev), d["invstd"].to(dev), c["M"] * c["k"])
            fn = ops.edge_dw_sel_bf16 if c["a16"] else ops.edge_dw_sel_f32
            got = fn(d["Y"].to(dev).to(dt), d["arg"].to(dev), d["dpre"].to(dev).to(dt), c["k"], wide[:, 4:132], st, d["red"].to(dev))
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    return got, sorted(k for k in prof if k.startswith(("gemm_", "edge_dw_sel")))


def check_case(c, d, got, labels):
    assert labels == [c["label"]], (c["name"], labels, c["label"])
    ref, scale, f32 = tc.reference(c, d)
    got = got.detach().cpu()
    assert got.dtype == (torch.bfloat16 if c["wrapper"] == "gemm_bf16s" else torch.float32)
    check_bound(c["name"], got.reshape(ref.shape), ref, f32, scale, tc.term_of(c), round16=c["wrapper"] == "gemm_bf16s", what="tn")


# ------------------------------------------------------------------ the children: one per switch set
def _child(sw, path):
    assert os.environ.get("LPD_DEBUG") == sw
    dev = torch.device("cuda:0")
    ops = _ops()
    out = {}
    for c in tr.CASES:
        if c["sw"] == sw:
            got, labels = run_case(ops, c, tc.make_inputs(c), dev)
            out[c["name"]] = (got.cpu(), labels)
            del got
    torch.save(out, path)


_CHILDREN = {}      # switch set -> results, or the failure every case of the set reports


def _child_results(sw, tmp_path_factory):
    if sw not in _CHILDREN and _DEVICE_LOST:
        pytest.fail("not run: " + _DEVICE_LOST[0])
    if sw not in _CHILDREN:
        path = tmp_path_factory.mktemp("tn_child") / "out.pt"
        code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
                "import test_tn_routes_gpu as t\n"
                "t._child(%r, %r)\n") % (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "lpd-net-pytorch_amd"), sw, str(path))
        try:
            r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LPD_DEBUG=sw), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
            _CHILDREN[sw] = torch.load(path) if r.returncode == 0 else AssertionError(
                f"child LPD_DEBUG={sw} exited with {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:])
            if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stderr.lower() for w in _FAULT_WORDS):
                _DEVICE_LOST.append(f"the child LPD_DEBUG={sw} faulted or aborted (exit {r.returncode})")
        except subprocess.TimeoutExpired:
            _CHILDREN[sw] = AssertionError(f"child LPD_DEBUG={sw} did not finish in {CHILD_TIMEOUT} s")
            _DEVICE_LOST.append(f"the child LPD_DEBUG={sw} hung")
    if isinstance(_CHILDREN[sw], Exception):
        raise _CHILDREN[sw]
    return _CHILDREN[sw]


@pytest.mark.parametrize("name", [c["name"] for c in tr.CASES])
def test_tn_route(cuda, tmp_path_factory, name):
    c = tr.by_name(name)
    d = tc.make_inputs(c)
    if c["sw"]:
        got, labels = _child_results(c["sw"], tmp_path_factory)[name]
    else:
        assert not any(t in os.environ.get("LPD_DEBUG", "") for t in tr.SWITCHES), "the case table states the default switches"
        got, labels = run_case(_ops(), c, d, cuda)
    check_case(c, d, got, labels)
