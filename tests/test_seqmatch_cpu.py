"""CPU side of the sequence scoring of retrieved candidates (lpd_seq_match, lpdnet_hip/sequence.py): the kernel's arithmetic header
(csrc/lpd_seq_math.h) compiled by the host C++ compiler and compared with the numpy restatement (tests/seq_ref.py) value for value,
hand-made drives with their answers written down, the quality of the restatement on seeded synthetic drives, and the validation of
SeqSearch, ops.seq_match and self_candidates.  The kernel itself is tested on the GPU (tests/test_seqmatch_gpu.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import seq_ref as R
from lpdnet_hip import LpdHipError, ops, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lpd-net-pytorch_amd", "csrc")
f32 = np.float32
i32 = np.int32

# ---- the gates ---------------------------------------------------------------------------------------------------------------------
# Quality on seq_ref.quality_drive(seed, noise = 2.5), seeds 0, 1, 2, K = 10 candidates by float64 distance, the default SeqSearch.
# The restatement shows (test_quality_on_synthetic_drives prints every seed):
#   single-frame top-1 right     0.506  0.450  0.450
#   best sequence candidate      0.894  0.913  0.906
#   after the shift              0.913  0.925  0.906
# (noise = 2.0: 0.80-0.82 -> 0.98-0.99 -> 0.99-1.00.)  The gates are the measured minimum minus 0.03, three seeds being a small sample;
# the single-frame share must stay at or below 0.6, so that the test shows a gain and not an easy input.
QUALITY_NOISE, QUALITY_K, QUALITY_SEEDS = 2.5, 10, (0, 1, 2)
QUALITY_SEQ_MEASURED, QUALITY_MOVED_MEASURED = 0.894, 0.906
QUALITY_SEQ_GATE, QUALITY_MOVED_GATE = QUALITY_SEQ_MEASURED - 0.03, QUALITY_MOVED_MEASURED - 0.03
QUALITY_SINGLE_MAX = 0.6

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lpd_seq_math.h"
// <mode> <in> <out> <n>: n fixed-size records in, n fixed-size records out
//   quant   1 f32                                        -> 1 i32
//   d2q     3 f32 (qn, dn, dot)                          -> 1 i32
//   counted 7 i32 (a, qlo, qhi, b, dlo, dhi, dq)         -> 1 i32
//   better  6 i32 (sum1, n1, key1, sum2, n2, key2)       -> 1 i32
//   number  5 i32 (v, s, S, row, j)                      -> 6 i32 (e, v(e), s(e), b', in band, centre ok for the run [row, j))
//   run     10 i32 (nruns, x, off[8])                    -> 1 i32
//   hypo    1024 i32 (block) + 31 i32 (steps row) + 8 i32 (h, s, i, qlo, qhi, j, dlo, dhi) -> 2 i32 (sum, n)
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    const char* mode = argv[1];
    const size_t n = (size_t)atol(argv[4]);
    size_t rin = 0, rout = 4;
    if (!strcmp(mode, "quant")) rin = 4;
    else if (!strcmp(mode, "d2q")) rin = 12;
    else if (!strcmp(mode, "counted")) rin = 28;
    else if (!strcmp(mode, "better")) rin = 24;
    else if (!strcmp(mode, "number")) { rin = 20; rout = 24; }
    else if (!strcmp(mode, "run")) rin = 40;
    else if (!strcmp(mode, "hypo")) { rin = 4 * (1024 + 31 + 8); rout = 8; }
    else return 2;
    std::vector<unsigned char> in(n * rin), out(n * rout);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi || fread(in.data(), 1, in.size(), fi) != in.size()) return 3;
    fclose(fi);
    for (size_t k = 0; k < n; ++k) {
        const unsigned char* r = &in[k * rin];
        unsigned char* o = &out[k * rout];
        if (!strcmp(mode, "quant")) {
            float v;
            memcpy(&v, r, 4);
            const int32_t q = lpd_seq_quant(v);
            memcpy(o, &q, 4);
        } else if (!strcmp(mode, "d2q")) {
            float f[3];
            memcpy(f, r, 12);
            const int32_t q = lpd_seq_d2q(f[0], f[1], f[2]);
            memcpy(o, &q, 4);
        } else if (!strcmp(mode, "counted")) {
            int32_t a[7];
            memcpy(a, r, 28);
            const int32_t q = lpd_seq_counted(a[0], a[1], a[2], a[3], a[4], a[5], a[6]) ? 1 : 0;
            memcpy(o, &q, 4);
        } else if (!strcmp(mode, "better")) {
            int32_t a[6];
            memcpy(a, r, 24);
            const int32_t q = lpd_seq_better(a[0], a[1], a[2], a[3], a[4], a[5]) ? 1 : 0;
            memcpy(o, &q, 4);
        } else if (!strcmp(mode, "number")) {
            int32_t a[5], q[6];
            memcpy(a, r, 20);
            q[0] = lpd_seq_hyp(a[0], a[1], a[2]);
            q[1] = lpd_seq_hyp_v(q[0], a[2]);
            q[2] = lpd_seq_hyp_s(q[0], a[2]);
            q[3] = lpd_seq_band(a[3], a[4]);
            q[4] = lpd_seq_in_band(q[3]) ? 1 : 0;
            q[5] = lpd_seq_centre_ok(a[0], a[1], a[3], a[4]) ? 1 : 0;
            memcpy(o, q, 24);
        } else if (!strcmp(mode, "run")) {
            int32_t a[10];
            memcpy(a, r, 40);
            const int32_t q = lpd_seq_run(a + 2, a[0], a[1]);
            memcpy(o, &q, 4);
        } else {
            std::vector<int32_t> a(1024 + 31 + 8);
            memcpy(a.data(), r, rin);
            const int32_t* p = a.data() + 1024 + 31;
            const LpdSeqSum t = lpd_seq_hypothesis(a.data(), 32, a.data() + 1024, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
            const int32_t q[2] = {t.sum, t.n};
            memcpy(o, q, 8);
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo || fwrite(out.data(), 1, out.size(), fo) != out.size()) return 4;
    fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("seq_math")
    src = d / "seq_math_host.cpp"
    src.write_text(PROGRAM)
    exe = d / "seq_math_host"
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(mode, records, out_ints=1):
        records = np.ascontiguousarray(records)
        n = len(records)
        (d / "in.bin").write_bytes(records.tobytes())
        r = subprocess.run([str(exe), mode, str(d / "in.bin"), str(d / "out.bin"), str(n)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (mode, r.returncode, r.stdout + r.stderr)
        got = np.fromfile(d / "out.bin", dtype=i32)
        assert got.size == n * out_ints
        return got.reshape(n, out_ints)
    return run


def _next(v, toward):
    return np.nextafter(f32(v), f32(toward))


# ---- 1. the arithmetic header against the restatement -------------------------------------------------------------------------------
def test_quantisation_at_halves_the_clamp_nan_and_inf(host):
    g = np.random.default_rng(1)
    q = f32(1.0 / 16384.0)
    edge = [0.0, -0.0, 0.5 * q, 1.5 * q, 2.5 * q, 3.5 * q, _next(0.5 * q, 0), _next(0.5 * q, 1), _next(1.5 * q, 0), _next(1.5 * q, 1), 16.0,
            _next(16.0, 0), _next(16.0, 100), 17.0, 1e30, np.inf, -np.inf, np.nan, -1.0, -1e-30, 2.0, 4.0, _next(4.0, 0)]
    v = np.concatenate((np.array(edge, dtype=f32), g.uniform(0, 4.5, 4000).astype(f32), g.uniform(0, 20, 500).astype(f32),
                        (g.integers(0, 1 << 18, 2000) + 0.5).astype(f32) * q))
    got = host("quant", v)[:, 0]
    assert np.array_equal(got, R.quant(v))
    # the written-down answers: halves go to the even integer, the clamp holds from 16 on, NaN is -1, -inf and negatives count as 0
    assert got[:len(edge)].tolist() == [0, 0, 0, 2, 2, 4, 0, 1, 1, 2, 1 << 18, 1 << 18, 1 << 18, 1 << 18, 1 << 18, 1 << 18, 0, -1, 0, 0,
                                        1 << 15, 1 << 16, 1 << 16]      # (one ulp below 16 is 2^-6 quanta below 2^18: it rounds up)
    assert got.max() == 1 << 18 and got.min() == -1


def test_distance_term_is_nan_before_the_clamp(host):
    g = np.random.default_rng(2)
    n = 4000
    qn, dn = g.uniform(0.5, 1.5, n).astype(f32), g.uniform(0.5, 1.5, n).astype(f32)
    dot = g.uniform(-1.2, 1.2, n).astype(f32)
    edge = [(1.0, 1.0, 1.0), (1.0, 1.0, 1.0001), (np.nan, 1.0, 0.5), (1.0, np.nan, 0.5), (1.0, 1.0, np.nan), (np.inf, 1.0, np.inf),
            (np.inf, 1.0, 0.0), (1.0, 1.0, -np.inf), (1.0, 1.0, np.inf), (9.0, 9.0, -1.0), (3e38, 3e38, 0.0)]
    rec = np.concatenate((np.stack((qn, dn, dot), 1), np.array(edge, dtype=f32)))
    got = host("d2q", rec)[:, 0]
    assert np.array_equal(got, R.d2q(rec[:, 0], rec[:, 1], rec[:, 2]))
    # x = 0 -> 0; x < 0 -> 0; a NaN anywhere -> -1; inf - inf -> -1; +inf -> the clamp; -inf -> 0 (not NaN: counted); 20 -> the clamp
    assert got[n:].tolist() == [0, 0, -1, -1, -1, -1, 1 << 18, 1 << 18, 0, 1 << 18, 1 << 18]


def test_counting_predicate_at_the_ends_of_a_run(host):
    rec, want = [], []
    for a in (9, 10, 11, 19, 20, 21):
        for b in (29, 30, 31, 39, 40, 41):
            for dq in (-1, 0, 5):
                rec.append((a, 10, 20, b, 30, 40, dq))
                want.append(int(10 <= a < 20 and 30 <= b < 40 and dq >= 0))
    rec += [(0, 0, 0, 0, 0, 1, 3), (0, 0, 1, 0, 0, 0, 3), (0, 0, 1, 0, 0, 1, 3)]      # empty runs hold nothing; runs of one row
    want += [0, 0, 1]
    got = host("counted", np.array(rec, dtype=i32))[:, 0]
    assert got.tolist() == want
    assert got.tolist() == [int(R.counted(*r)) for r in rec]


def test_comparator_equal_means_big_sums_and_none(host):
    g = np.random.default_rng(3)
    big = (1 << 23) - 1
    rec = [(6, 3, 0, 4, 2, 1), (4, 2, 1, 6, 3, 0), (6, 3, 1, 4, 2, 0), (4, 2, 0, 6, 3, 1),      # 6/3 = 4/2: the lower key
           (big, 31, 0, big, 30, 1), (big, 30, 1, big, 31, 0), (big, 31, 5, big - 1, 31, 2), (big - 1, 31, 2, big, 31, 5),
           (big, 31, 3, big, 31, 3), (0, 1, 7, 0, 31, 2), (0, 31, 2, 0, 1, 7),
           (0, 0, -1, 5, 1, 0), (5, 1, 0, 0, 0, -1), (0, 0, -1, 0, 0, -1), (7, 11, 0, 7, 11, 1)]
    want = [1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1]
    n = 4000
    rnd = np.stack((g.integers(0, big, n), g.integers(1, 32, n), g.integers(-1, 64, n), g.integers(0, big, n), g.integers(1, 32, n),
                    g.integers(-1, 64, n)), 1)
    rnd[::3, 3] = rnd[::3, 0] // rnd[::3, 1] * rnd[::3, 4]      # many near and exact ties
    rnd[::3, 0] = rnd[::3, 0] // rnd[::3, 1] * rnd[::3, 1]
    rec = np.concatenate((np.array(rec, dtype=np.int64), rnd)).astype(i32)
    got = host("better", rec)[:, 0]
    assert got[:len(want)].tolist() == want
    assert got.tolist() == [int(R.better(*map(int, r))) for r in rec]
    ties = (rec[:, 0].astype(np.int64) * rec[:, 4] == rec[:, 3].astype(np.int64) * rec[:, 1]).sum()
    assert ties > 500      # the tie rule is exercised


def test_hypothesis_numbering_band_and_runs(host):
    rec = [(v, s, S, row, j) for S in (0, 1, 2, 15) for v in (0, 1, 5, 30) for s in range(-S, S + 1) for row, j in ((0, 15), (7, 7), (40, 24), (9, 25), (41, 25))]
    rec = np.array(rec, dtype=i32)
    got = host("number", rec, 6)
    for r, o in zip(rec.tolist(), got.tolist()):
        v, s, S, row, j = r
        e = R.hyp(v, s, S)
        assert o[:5] == [e, R.hyp_v(e, S), R.hyp_s(e, S), R.band(row, j), int(0 <= R.band(row, j) <= 30)] and o[1] == v and o[2] == s
        assert o[5] == int(row <= v + s < j)
    assert len({tuple(o[:1]) for o in got[(rec[:, 2] == 2) & (rec[:, 3] == 0)].tolist()}) == 4 * 5      # e is one-to-one over (v, s)
    # the run search: empty runs are stepped over, every row of a table finds the run that holds it
    offs = [[0, 8], [0, 1, 8], [0, 3, 3, 8], [0, 0, 8], [0, 2, 4, 4, 4, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7]]
    rec, want = [], []
    for off in offs:
        for x in range(off[-1]):
            rec.append([len(off) - 1, x] + off + [0] * (8 - len(off)))
            m = max(k for k in range(len(off) - 1) if off[k] <= x)
            assert off[m] <= x < off[m + 1]
            want.append(m)
    got = host("run", np.array(rec, dtype=i32))[:, 0]
    assert got.tolist() == want
    assert got.tolist() == [int(R.run_of(r[2:2 + r[0] + 1], r[1])) for r in rec]


def test_one_hypothesis_over_a_block(host):
    g = np.random.default_rng(4)
    rec, want = [], []
    for _ in range(600):
        h = int(g.choice([1, 5, 15]))
        L = 2 * h + 1
        blk = g.integers(0, 1 << 18, (32, 32)).astype(i32)
        blk[g.random((32, 32)) < 0.1] = -1
        blk[31], blk[:, 31] = -1, -1
        reach = int(g.integers(0, 18))      # up to 17: some tables break the band
        st = np.zeros(31, dtype=i32)
        st[:L] = g.integers(-reach, reach + 1, L)
        st[h] = 0
        s = int(g.integers(-3, 4))
        i, j = int(g.integers(0, 60)), int(g.integers(0, 60))
        qlo, dlo = int(g.integers(0, i + 1)), int(g.integers(0, j + 1))
        qhi, dhi = int(g.integers(i + 1, 70)), int(g.integers(j + 1, 70))
        rec.append(np.concatenate((blk.reshape(-1), st, np.array([h, s, i, qlo, qhi, j, dlo, dhi], dtype=i32))))
        want.append(R.hypothesis(blk, st, h, s, i, qlo, qhi, j, dlo, dhi))
    got = host("hypo", np.stack(rec).astype(i32), 2)
    assert got.tolist() == [list(w) for w in want]
    assert (got[:, 1] > 0).sum() > 300 and len(set(got[:, 1].tolist())) > 8


# ---- 2. hand-made drives with written-down answers ----------------------------------------------------------------------------------
VEL = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def _unit_table(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)


def _planted(vel, h=5, nd=80, nq=40, i0=20, j0=40, seed=0):
    """a database of random unit rows and queries of which rows i0 - h .. i0 + h are the database rows j0 + steps(vel)"""
    D = _unit_table(nd, 64, seed)
    Q = _unit_table(nq, 64, seed + 100)
    st = R.steps_table((vel,), h)[0]
    Q[i0 - h:i0 + h + 1] = D[j0 + st]
    return Q, D


@pytest.mark.parametrize("vel", (1.0, 2.0, 0.5, -1.0))
def test_query_drive_at_a_velocity_finds_its_line(vel):
    h, S, i0, j0 = 5, 2, 20, 40
    Q, D = _planted(vel, h, i0=i0, j0=j0)
    cand = np.full((len(Q), 3), -1, dtype=i32)
    cand[i0] = (7, j0, 63)      # two distractors around the truth
    steps = R.steps_table(VEL, h)
    for fn in (R.match, R.match_slow):
        best, order = fn(R.blocks_f64(Q, D, cand, h), cand, steps, S, h + 1, len(D))
        assert best[i0, 1].tolist() == [R.hyp(VEL.index(vel), 0, S), 0, 2 * h + 1, j0]      # the planted line: every term 0, all 11 counted
        assert order[i0].tolist() == [1, 0, 2] or order[i0].tolist() == [1, 2, 0]
        assert best[i0, 0, 0] >= 0 and best[i0, 0, 1] > 11 * 16384      # a distractor's line: unit rows lie sqrt(2) apart
        assert (best[0] == (-1, 0, 0, -1)).all() and order[0].tolist() == [0, 1, 2]      # skipped candidates keep the retrieval order


def test_shift_moves_a_candidate_two_rows_back():
    h, S, i0, j0 = 5, 2, 20, 40
    Q, D = _planted(1.0, h, i0=i0, j0=j0)
    steps = R.steps_table(VEL, h)
    for off in (-2, -1, 1, 2):
        cand = np.full((len(Q), 1), j0 + off, dtype=i32)
        best, _ = R.match(R.blocks_f64(Q, D, cand, h), cand, steps, S, h + 1, len(D))
        assert best[i0, 0].tolist() == [R.hyp(VEL.index(1.0), -off, S), 0, 11, j0]
    cand = np.full((len(Q), 1), j0 + 3, dtype=i32)      # three rows off is out of reach of two shifts
    best, _ = R.match(R.blocks_f64(Q, D, cand, h), cand, steps, S, h + 1, len(D))
    assert best[i0, 0, 1] > 0 and best[i0, 0, 3] != j0


def test_short_runs_and_min_terms():
    h, S, i0, j0 = 5, 0, 20, 40
    Q, D = _planted(1.0, h, i0=i0, j0=j0)
    steps = R.steps_table(VEL, h)
    cand = np.full((len(Q), 1), j0, dtype=i32)
    blk = R.blocks_f64(Q, D, cand, h)
    q_off = np.array([0, 19, 23, 40])      # the query's run is rows 19 .. 22: t = -1 .. 2, four terms
    e = R.hyp(VEL.index(1.0), 0, S)
    for fn in (R.match, R.match_slow):
        assert fn(blk, cand, steps, S, 4, len(D), q_off=q_off)[0][i0, 0].tolist() == [e, 0, 4, j0]
        assert fn(blk, cand, steps, S, 5, len(D), q_off=q_off)[0][i0, 0].tolist() == [-1, 0, 0, -1]      # min_terms refuses it
        # the database run cut as well: rows 40 .. 41 -> t = 0 .. 1; a run of one row counts one term
        assert fn(blk, cand, steps, S, 2, len(D), q_off=q_off, d_off=[0, 40, 42, 80])[0][i0, 0].tolist() == [e, 0, 2, j0]
        b1 = fn(blk, cand, steps, S, 1, len(D), q_off=[0, 20, 21, 40])[0][i0, 0].tolist()
        assert b1[1:] == [0, 1, j0] and b1[0] == 0      # one term, the same for every velocity: the lowest e
    # a shift must stay inside the candidate's run
    best, _ = R.match(R.blocks_f64(Q, D, cand + 1, h), cand + 1, steps, 2, 1, len(D), d_off=[0, 41, 80])
    assert best[i0, 0, 3] >= 41


# ---- 3. quality of the restatement --------------------------------------------------------------------------------------------------
def quality_case(seed, topk=None, scorer=None):
    """(single, sequence, moved) shares of one seeded drive; topk / scorer let the GPU test put the device in"""
    Q, D, truth, q_off = R.quality_drive(seed, QUALITY_NOISE)
    s = sequence.SeqSearch()
    if scorer is None:
        cand = R.topk_f64(Q, D, QUALITY_K)
        best, order = R.match(R.blocks_f64(Q, D, cand, s.half_length), cand, s.steps_table(), s.shifts, s.min_terms, len(D), q_off=q_off)
    else:
        cand, best, order = scorer(Q, D, q_off, s)
    return R.quality(cand, best, order, truth)


def test_quality_on_synthetic_drives():
    for seed in QUALITY_SEEDS:
        single, seq, moved = quality_case(seed)
        print(f"MEASURE seq/quality seed={seed} noise={QUALITY_NOISE} single-frame {single:.3f} sequence {seq:.3f} after the shift {moved:.3f}")
        assert single <= QUALITY_SINGLE_MAX
        assert seq >= QUALITY_SEQ_GATE and moved >= QUALITY_MOVED_GATE


# ---- 4. validation ------------------------------------------------------------------------------------------------------------------
def test_seqsearch_is_validated_and_frozen():
    s = sequence.SeqSearch()
    assert (s.velocities, s.half_length, s.shifts, s.min_terms, s.hypotheses) == (VEL, 5, 2, 6, 30)
    assert sequence.SeqSearch(min_terms=3).min_terms == 3 and sequence.SeqSearch(half_length=2).min_terms == 3
    assert s == sequence.SeqSearch() and hash(s) == hash(sequence.SeqSearch()) and s != sequence.SeqSearch(shifts=1)
    with pytest.raises(AttributeError):
        s.shifts = 3
    for kw in (dict(velocities=()), dict(velocities="1"), dict(velocities=(1.0, float("nan"))), dict(velocities=(float("inf"),)), dict(velocities=(True,)),
               dict(velocities=1.0), dict(half_length=0), dict(half_length=16), dict(half_length=2.0), dict(shifts=-1), dict(shifts=16), dict(shifts=True),
               dict(min_terms=0), dict(min_terms=12), dict(min_terms=1.5),
               dict(velocities=(2.0,), half_length=7, shifts=2),      # 14 + 2 > 15
               dict(velocities=(3.0,), half_length=5, shifts=1),      # 15 + 1
               dict(velocities=tuple(range(1, 343)), half_length=1, shifts=1)):      # 342 x 3 = 1026 hypotheses
        with pytest.raises(ValueError):
            sequence.SeqSearch(**kw)
    assert sequence.SeqSearch(velocities=(3.0,), half_length=5, shifts=0).steps_table().max() == 15      # the band's edge is allowed
    assert sequence.SeqSearch(velocities=[0.25 * k for k in range(-4, 5)] * 37 + [0.0], half_length=15, shifts=0).hypotheses == 334


def test_steps_table_rounds_half_to_even_like_round():
    for vel, h in ((VEL, 5), ((0.5, -0.5, 1.5, -1.5, 0.25, 0.75), 10), ((1.0,), 15), ((0.3, -0.7, 0.0), 15)):
        s = sequence.SeqSearch(velocities=vel, half_length=h, shifts=0)
        t = s.steps_table()
        assert t.dtype == np.int32 and t.shape == (len(vel), 2 * h + 1) and (t[:, h] == 0).all()
        assert np.array_equal(t, R.steps_table(vel, h))
    assert sequence.SeqSearch(velocities=(0.5,), half_length=5, shifts=0).steps_table().tolist() == [[-2, -2, -2, -1, 0, 0, 0, 1, 2, 2, 2]]


def test_seq_match_checks_its_arguments_on_the_host():
    Q, D = torch.zeros((8, 64)), torch.zeros((9, 64))
    cand = torch.zeros((8, 3), dtype=torch.int32)
    st = R.steps_table(VEL, 5)
    ok = dict(Q=Q, D=D, cand=cand, steps=st, S=2, min_terms=6)

    def bad(exc, **kw):
        with pytest.raises(exc):
            ops.seq_match(**{**ok, **kw})
    bad(TypeError, Q=Q.double())
    bad(TypeError, D=None)
    bad(TypeError, cand=cand.long())
    bad(ValueError, D=torch.zeros((9, 128)))
    bad(ValueError, Q=torch.zeros((8, 512)), D=torch.zeros((9, 512)))
    bad(ValueError, Q=torch.zeros((0, 64)), cand=torch.zeros((0, 3), dtype=torch.int32))
    bad(ValueError, cand=torch.zeros((7, 3), dtype=torch.int32))
    bad(ValueError, cand=torch.zeros((8, 65), dtype=torch.int32))
    bad(ValueError, cand=torch.zeros((8, 0), dtype=torch.int32))
    bad(ValueError, steps=st.astype(np.int64))
    bad(ValueError, steps=st[:, :10])                      # an even length
    bad(ValueError, steps=st[0])
    bad(ValueError, steps=st + 1)                          # the middle column is not 0
    bad(ValueError, S=6)                                   # 10 + 6 > 15
    bad(ValueError, S=-1)
    bad(ValueError, S=1.0)
    bad(ValueError, steps=np.zeros((400, 11), dtype=np.int32), S=1)      # 1200 hypotheses
    bad(ValueError, min_terms=0)
    bad(ValueError, min_terms=12)
    bad(ValueError, q_off=np.array([0, 4, 9], dtype=np.int32))          # ends past the table
    bad(ValueError, q_off=np.array([1, 8], dtype=np.int32))
    bad(ValueError, d_off=np.array([0, 5, 4, 9], dtype=np.int32))       # falls
    bad(ValueError, d_off=np.array([0, 9], dtype=np.int64))
    bad(ValueError, d_off=np.array([0, 8], dtype=np.int32))             # ends before the table does
    bad(LpdHipError)                                       # everything in order, but on the host: there is no CPU path
    assert ops.seq_steps(st, 5)[1] == 5 and (ops.SEQ_BAND, ops.SEQ_QBITS, ops.SEQ_KMAX, ops.SEQ_MAX_HYP) == (15, 14, 64, 1024)


def test_wrappers_check_their_arguments_on_the_host():
    Q = torch.zeros((8, 64))
    idx = torch.zeros((8, 3), dtype=torch.int32)
    with pytest.raises(TypeError):
        sequence.match_sequences(Q, Q, idx, search=dict(shifts=2))
    with pytest.raises(TypeError):
        sequence.match_sequences(Q, Q, idx.float())
    with pytest.raises(TypeError):
        sequence.match_sequences(Q, Q, idx[0])
    for mm in (-0.1, float("nan"), 17.0, True, "1"):
        with pytest.raises(ValueError):
            sequence.match_sequences(Q, Q, idx, max_mean=mm)
    with pytest.raises(LpdHipError):
        sequence.match_sequences(Q, Q, idx.long(), max_mean=0.5)
    with pytest.raises(TypeError):
        sequence.self_candidates(Q.double())
    for kw in (dict(k=0), dict(k=65), dict(k=2.0), dict(exclude=-1), dict(exclude=True), dict(offsets=np.array([0, 7], dtype=np.int32))):
        with pytest.raises(ValueError):
            sequence.self_candidates(Q, **kw)
    with pytest.raises(ValueError):
        sequence.self_candidates(torch.zeros((8,)))
    with pytest.raises(LpdHipError):
        sequence.self_candidates(Q, k=3, exclude=1)


def test_restatements_fast_and_slow_agree():
    g = np.random.default_rng(9)
    for case in range(6):
        nq, nd, K = int(g.integers(1, 30)), int(g.integers(1, 40)), int(g.integers(1, 7))
        h, S = int(g.choice([1, 3, 5])), int(g.integers(0, 3))
        Q, D = _unit_table(nq, 64, case), _unit_table(nd, 64, case + 50)
        D[g.integers(0, nd, 3)] = D[0]      # duplicated rows: ties
        cand = g.integers(-1, nd + 1, (nq, K)).astype(i32)
        steps = R.steps_table((-1.0, 0.5, 1.0, 1.0), h)      # a duplicated velocity: ties between hypotheses
        blk = R.blocks_f64(Q, D, cand, h)
        q_off = np.unique(np.concatenate(([0, nq], g.integers(0, nq + 1, 2))))
        d_off = np.unique(np.concatenate(([0, nd], g.integers(0, nd + 1, 2))))
        a = R.match(blk, cand, steps, S, 1 + case % 3, nd, q_off, d_off)
        b = R.match_slow(blk, cand, steps, S, 1 + case % 3, nd, q_off, d_off)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert (np.sort(a[1], axis=1) == np.arange(K)).all()
