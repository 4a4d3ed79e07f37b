"""CPU side of the device-resident training tuples (lpd_sample_items, lpd_gather_tuples, lpdnet_hip/tuples.py): the numpy restatement
(tests/tuples_ref.py) against published known answers and hand-made cases, the kernels' arithmetic header (csrc/lpd_tuple_math.h)
compiled by the host C++ compiler and compared with the restatement value for value, the host side of TupleBank, and the public
surface with its no-fallback rule.  The kernels themselves are tested on the GPU (tests/test_tuples_gpu.py)."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tuples_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATH_H = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc", "lpd_tuple_math.h")
F = 0xFFFFFFFF
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((F, F, F, F), (F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
SEEDS = (0, 0xDEADBEEFCAFE1234)


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert tuple(int(v) for v in R.philox(*ctr, *key)) == want


def test_uniform_is_exact_in_fp32_and_open():
    r = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0x80000000, F], dtype=np.uint64)
    u = R.uniform(r)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)      # representable: the fp32 expression has no rounding
    assert u.min() == 2.0 ** -24 and u.max() == 1 - 2.0 ** -24
    f = ((r >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert np.array_equal(f.astype(np.float64), u)


@pytest.mark.parametrize("c", [1, 2, 3, 5, 64, 65, 1000, 4097])
def test_perm_is_a_bijection(c):
    for seed in SEEDS:
        for row in (0, 7):
            p = R.perm_all(c, seed, row)
            assert sorted(p.tolist()) == list(range(c)), (c, seed, row)
            if c > 1:
                assert R.perm(c - 1, c, seed, row) == p[c - 1] and R.perm(0, c, seed, row) == p[0]
    if c >= 64:      # seed and row both matter
        assert not np.array_equal(R.perm_all(c, SEEDS[0], 0), R.perm_all(c, SEEDS[1], 0))
        assert not np.array_equal(R.perm_all(c, SEEDS[0], 0), R.perm_all(c, SEEDS[0], 7))


def test_perm_slot_zero_is_not_grossly_biased():
    """A coarse guard, not a statistical claim: at c = 13 over 4096 seeds every value lands in slot 0 between 0.5x and 1.5x of
    4096 / 13 times; that window is more than 9 standard deviations wide for a fair draw."""
    cnt = np.zeros(13, dtype=np.int64)
    for seed in range(4096):
        cnt[R.perm(0, 13, seed, 0)] += 1
    fair = 4096 / 13
    assert cnt.sum() == 4096 and (cnt > 0.5 * fair).all() and (cnt < 1.5 * fair).all(), cnt.tolist()


def test_jitter_restatement_moments():
    z = R.normals(4096, range(32), 20261018)      # 32 x 4096 x 3 normals
    print(f"MEASURE normals mean {z.mean():.4f} var {z.var():.4f}")      # -0.0021 / 1.0012
    assert z.shape == (32, 4096, 3) and abs(z.mean()) < 0.008 and abs(z.var() - 1.0) < 0.012      # five standard errors
    d = R.jitter(4096, [0, 1], 5, 0.05, 0.05)
    assert np.abs(d).max() <= float(np.float32(0.05))
    assert not np.array_equal(R.normals(64, [0], 1), R.normals(64, [1], 1)) and not np.array_equal(R.normals(64, [0], 1), R.normals(64, [0], 2))


def test_select_bit():
    assert R.select_bit(0b1011000, 0) == 3 and R.select_bit(0b1011000, 2) == 6 and R.select_bit(0b1011000, 3) == 32
    assert R.select_bit(0x80000000, 0) == 31 and R.select_bit(F, 17) == 17 and R.select_bit(0, 0) == 32


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.array([i for l in lists for i in l], dtype=np.int32)
    return off, idx


def test_sampling_restatement_on_hand_made_cases():
    T = 10
    off, idx = _csr([[], [3, 1, 3, 1], [1, 2, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [12, -4, 5]])
    # empty lists and unused slots: an empty union, its complement is everything
    out, cnt = R.sample_items(off, idx, T, [[0, -1], [-1, -1]], None, 4, 0, 11)
    assert cnt.tolist() == [0, 0] and (out == -1).all()
    out, cnt = R.sample_items(off, idx, T, [[0, -1]], None, 10, 1, 11)
    assert cnt.tolist() == [10] and sorted(out[0].tolist()) == list(range(10))
    # duplicates inside a list and overlapping lists: the union {1, 2, 3, 7}
    out, cnt = R.sample_items(off, idx, T, [[1, 2]], None, 4, 0, 3)
    assert cnt.tolist() == [4] and sorted(out[0].tolist()) == [1, 2, 3, 7]
    assert out[0].tolist() == [[1, 2, 3, 7][p] for p in R.perm_all(4, 3, 0)]      # z_perm(j): the definition, spelled out
    out, cnt = R.sample_items(off, idx, T, [[1, 2]], [[9, -1]], 8, 1, 3)
    assert cnt.tolist() == [5] and sorted(out[0, :5].tolist()) == [0, 4, 5, 6, 8] and (out[0, 5:] == -1).all()      # m > c
    # the whole of [0, T) excluded
    out, cnt = R.sample_items(off, idx, T, [[3]], None, 3, 1, 0)
    assert cnt.tolist() == [0] and (out == -1).all()
    # list numbers and items outside their ranges are ignored: list 4 holds only item 5 of [0, T)
    out, cnt = R.sample_items(off, idx, T, [[4, 99]], [[10, -7]], 3, 0, 0)
    assert cnt.tolist() == [1] and out[0].tolist() == [5, -1, -1]
    # rows draw different permutations of the same pool
    out, cnt = R.sample_items(off, idx, 1000, [[0], [0]], None, 64, 1, 5)
    assert cnt.tolist() == [1000, 1000] and len(set(out[0].tolist())) == 64 and out[0].tolist() != out[1].tolist()


def test_gather_restatement_by_hand():
    table = np.arange(2 * 2 * 3, dtype=np.float32).reshape(2, 2, 3)
    g = R.gather_tuples(table, [1, -1, 2, 0])
    assert np.array_equal(g[0], table[1]) and np.array_equal(g[3], table[0]) and (g[1] == 0).all() and (g[2] == 0).all()
    g = R.gather_tuples(table, [0], rot=[[0.0, 1.0]])      # a quarter turn: x' = y, y' = -x
    assert np.array_equal(g[0], [[1, 0, 2], [4, -3, 5]])


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "lpd_tuple_math.h"
int main(int argc, char** argv)
{
    // in: uint32 words -- np philox cases (6 words each), nq perm queries (j, c, seed_lo, seed_hi, row), ns selects (w, r);
    // out: 4 words per philox case, one per perm query, one per select, then the bits of uniform(r) for the words of the selects
    if (argc != 6) return 2;
    const int np = atoi(argv[3]), nq = atoi(argv[4]), ns = atoi(argv[5]);
    std::vector<uint32_t> in((size_t)np * 6 + (size_t)nq * 5 + (size_t)ns * 2), out;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi || fread(in.data(), 4, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    const uint32_t* p = in.data();
    for (int i = 0; i < np; ++i, p += 6) {
        const LpdPhilox4 r = lpd_philox4x32_10(p[0], p[1], p[2], p[3], p[4], p[5]);
        for (int k = 0; k < 4; ++k) out.push_back(r.v[k]);
    }
    for (int i = 0; i < nq; ++i, p += 5) out.push_back(lpd_tuple_perm(p[0], p[1], ((uint64_t)p[3] << 32) | p[2], p[4]));
    const uint32_t* s = p;
    for (int i = 0; i < ns; ++i, p += 2) out.push_back(lpd_tuple_select_bit(p[0], p[1]));
    for (int i = 0; i < ns; ++i, s += 2) {
        const float u = lpd_tuple_uniform(s[0]);
        uint32_t b;
        __builtin_memcpy(&b, &u, 4);
        out.push_back(b);
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo || fwrite(out.data(), 4, out.size(), fo) != out.size()) return 4;
    fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def math_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("tuple_math")
    src = d / "tuple_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "tuple_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.dirname(MATH_H), str(src), "-o", str(exe), "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_math_header_on_the_host_equals_numpy(math_program, tmp_path):
    """The kernels' own integer arithmetic, compiled for the host: Philox words, perm values, bit selects and the uniforms equal the
    restatement value for value -- checked before any launch."""
    rng = np.random.default_rng(20261018)
    ph = [list(c) + list(k) for c, k, _ in KNOWN] + rng.integers(0, 1 << 32, size=(61, 6)).tolist()
    pq = []
    for c in (1, 2, 3, 4, 5, 13, 16, 17, 64, 65, 1000, 4097, 21711, 262144):
        for seed in SEEDS + (int(rng.integers(0, 1 << 63)),):
            for row in (0, 7, 65534):
                for j in sorted({0, c // 2, c - 1}):
                    pq.append([j, c, seed & F, seed >> 32, row])
    sel = [[0, 0], [F, 0], [F, 31], [0x80000000, 0], [0b1011000, 2], [0b1011000, 3]]
    for w in rng.integers(0, 1 << 32, size=40).tolist():
        n = bin(w).count("1")
        sel += [[w, 0], [w, n // 2], [w, n - 1], [w, n]]
    words = np.array([v for row in ph + pq + sel for v in row], dtype=np.uint32)
    words.tofile(tmp_path / "in.bin")
    r = subprocess.run([str(math_program), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(len(ph)), str(len(pq)), str(len(sel))],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    w = np.fromfile(tmp_path / "out.bin", dtype=np.uint32)
    assert w.size == 4 * len(ph) + len(pq) + 2 * len(sel)
    a = np.array(ph, dtype=np.uint64)
    want = np.stack(R.philox(*(a[:, i] for i in range(6))), 1).astype(np.uint32)
    assert np.array_equal(w[:4 * len(ph)].reshape(-1, 4), want)
    assert tuple(w[:4].tolist()) == KNOWN[0][2]
    pos = 4 * len(ph)
    got = w[pos:pos + len(pq)].tolist()
    assert got == [R.perm(j, c, lo | (hi << 32), row) for j, c, lo, hi, row in pq]
    pos += len(pq)
    assert w[pos:pos + len(sel)].tolist() == [R.select_bit(a, b) for a, b in sel]
    pos += len(sel)
    u = R.uniform(np.array([a for a, _ in sel], dtype=np.uint64)).astype(np.float32)
    assert np.array_equal(w[pos:], u.view(np.uint32))


def _twelve():
    """12 places on a line, 10 m apart: positives within 10 m, negatives farther than 50 m"""
    x = np.arange(12) * 10.0
    d = np.abs(x[:, None] - x[None, :])
    return {i: {"query": f"run/{i}.bin", "positives": [int(j) for j in np.nonzero((d[i] <= 10) & (d[i] > 0))[0]],
                "negatives": [int(j) for j in np.nonzero(d[i] > 50)[0]]} for i in range(12)}


def test_bank_from_queries_dict_host_side():
    from lpdnet_hip import LpdHipError, tuples
    Q = _twelve()
    positives, near = tuples.TupleBank.lists_from_queries_dict(Q)
    assert positives[0] == [1] and positives[5] == [4, 6] and near[0].tolist() == [0, 1, 2, 3, 4, 5] and near[6].tolist() == list(range(1, 12))
    clouds = np.random.default_rng(0).standard_normal((12, 8, 3))      # float64
    bank = tuples.TupleBank.from_queries_dict(Q, clouds, device="cpu")      # the host side only
    assert (bank.T, bank.N) == (12, 8) and bank.pos_len.tolist() == [1] + [2] * 10 + [1] and bank.max_pos == 2 and bank.max_near == 11
    assert bank.near_len.tolist() == [6, 7, 8, 9, 10, 11, 11, 10, 9, 8, 7, 6]
    assert bank.table.dtype == torch.float32 and np.array_equal(bank.table.numpy(), clouds.astype(np.float32))
    off, idx = bank._pos_csr
    assert off.dtype == np.int32 and off.tolist() == np.concatenate(([0], np.cumsum(bank.pos_len))).tolist()
    assert idx[off[5]:off[6]].tolist() == [4, 6]
    # too few positives: named, found on the host before anything touches a device
    with pytest.raises(ValueError, match="query item 11 has 1 positives"):
        bank.sample([3, 11], 2, 1, seed=0)
    with pytest.raises(ValueError):
        bank.sample([12], 1, 1, seed=0)
    with pytest.raises(LpdHipError):      # a legal draw on a host-only bank: an error, not a CPU result
        bank.sample([3], 2, 1, seed=0)
    with pytest.raises(LpdHipError):
        bank.assemble(np.zeros((1, 4), dtype=np.int32))
    if not torch.cuda.is_available():
        with pytest.raises(LpdHipError):
            tuples.TupleBank.from_queries_dict(Q, clouds)
    with pytest.raises(ValueError):
        tuples.TupleBank(clouds, positives[:-1], near, device="cpu")
    with pytest.raises(ValueError):
        tuples.TupleBank(clouds, [[12]] + positives[1:], near, device="cpu")      # an item outside 0 .. T-1
    with pytest.raises(ValueError):
        tuples.TupleBank.lists_from_queries_dict({1: Q[1], 2: Q[2]})
    off, idx, lens = tuples.build_csr([[3, 1, 3], [], [2]], 4)
    assert off.tolist() == [0, 2, 2, 3] and idx.tolist() == [1, 3, 2] and lens.tolist() == [2, 0, 1]      # sorted, duplicates dropped


def test_run_dry_guarantee_and_seeds():
    from lpdnet_hip import tuples
    g = tuples.run_dry_guarantee
    assert g(21711, 600, 40, 18) == (True, True)
    assert g(100, 82, 5, 18) == (True, True) and g(100, 83, 5, 18) == (False, True)            # T - max|near| >= Ng
    assert g(95, 10, 5, 18) == (True, False) and g(96, 10, 5, 18) == (True, True)              # (1 + Ng) * max|positives| < T
    assert g(114, 10, 5, 18, exclude_members=True) == (True, False) and g(115, 10, 5, 18, exclude_members=True) == (True, True)
    s = [tuples.sub_seed(7, k) for k in range(5)]
    assert len(set(s)) == 5 and all(0 <= v < 2 ** 64 for v in s) and s[0] == (7 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert tuples.sub_seed(2 ** 64 - 1, 2) == (2 ** 64 - 1 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    r = tuples.TupleBank.rotations(1000, 3)
    assert r.dtype == np.float32 and r.shape == (1000, 2) and (r[:, 0] >= 0).all()      # |angle| <= pi/2: cos >= 0
    assert np.abs(r[:, 0] ** 2 + r[:, 1] ** 2 - 1).max() < 1e-6 and np.array_equal(r, tuples.TupleBank.rotations(1000, 3))
    assert (r[:, 1] < 0).any() and (r[:, 1] > 0).any()


def test_public_surface_and_no_cpu_fallback():
    from lpdnet_hip import LpdHipError, _lib, harness, ops, tuples
    i, p, f, u = _lib._c_int, _lib._c_p, _lib._c_f, __import__("ctypes").c_ulonglong
    assert _lib.SIGNATURES["lpd_sample_items"] == [p, p, i, i, i, p, i, p, i, i, i, i, u, p, p, p]
    assert _lib.SIGNATURES["lpd_gather_tuples"] == [p, i, i, p, i, p, f, f, u, p, p]
    assert [a for a in inspect.signature(ops.sample_items).parameters] == ["off", "idx", "T", "lists", "extra", "m", "invert", "seed"]
    sig = inspect.signature(ops.gather_tuples)
    assert [a for a in sig.parameters] == ["table", "items", "rot", "sigma", "clip", "seed", "out"]
    assert sig.parameters["sigma"].default == 0.0 and sig.parameters["clip"].default == 0.05 and sig.parameters["rot"].default is None
    assert [a for a in inspect.signature(tuples.TupleBank.sample).parameters] == ["self", "query_items", "P", "Ng", "seed", "hard", "exclude_members"]
    assert [a for a in inspect.signature(tuples.TupleBank.mine).parameters] == ["self", "latent", "query_items", "hard_neg_num", "n_sampled", "seed",
                                                                              "query_vecs"]
    assert inspect.signature(tuples.TupleBank.mine).parameters["n_sampled"].default == 4000
    assert [a for a in inspect.signature(tuples.TupleBank.assemble).parameters] == ["self", "items", "rotate", "jitter", "sigma", "clip", "seed"]
    assert [a for a in inspect.signature(harness.run_model_feed).parameters] == ["model", "feed", "bq", "P", "Ng", "require_grad", "output_dim"]
    assert [a for a in inspect.signature(harness.train_step_from_bank).parameters][:10] == [
        "model", "optimizer", "bank", "query_items", "P", "Ng", "seed", "hard", "rotate", "jitter"]
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(LpdHipError):
        ops.sample_items(z, z, 4, z.view(4, 1), None, 1, 0, 0)
    with pytest.raises(LpdHipError):
        ops.gather_tuples(torch.zeros(2, 4, 3), z, None)
    hdr = open(os.path.join(ROOT, "include", "lpd_hip.h")).read()
    assert "int lpd_sample_items(" in hdr and "int lpd_gather_tuples(" in hdr and "never used as an address" in hdr
    math = open(MATH_H).read()
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "cycle walking"):
        assert word in math
    src = open(tuples.__file__).read()
    assert "import oracle" not in src and "from oracle" not in src
