// lpd_seq_math.h -- the arithmetic of lpd_seq_match (csrc/lpd_seqmatch.hip): the quantisation of a squared descriptor distance, the
// numbering of the hypotheses (velocity, shift) of a candidate, the band index of a database row, the run search, the predicate
// that decides whether a term is counted, the sum of one hypothesis over a candidate's block of quantised distances, and the order of
// hypotheses and of candidates.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/seq_ref.py
// restates every function in numpy, and tests/test_seqmatch_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernel includes it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: the three fp32 operations of lpd_seq_d2q are
// rounded once each.  Everything behind the quantisation is integers, so every order of evaluation gives the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_SEQ_FN __host__ __device__ __forceinline__
#else
#define LPD_SEQ_FN static inline
#endif

// LPD_SEQ_BAND (a candidate's block holds the database rows j - 15 .. j + 15), LPD_SEQ_QBITS (the quantum of a squared distance is
// 2^-14), LPD_SEQ_KMAX and LPD_SEQ_MAX_HYP are the public header's
#define LPD_SEQ_CLAMP 16.0f               // a squared distance is clamped at 16: dq <= 2^18, a sum of 31 terms < 2^23
#define LPD_SEQ_QUANT 16384.0f            // 2^LPD_SEQ_QBITS
#define LPD_SEQ_TILE 32                   // the block is [32][32]; row 31 and column 31 are -1

// ---------------------------------------------------------------------------------------------------------------------------------
// the quantised distance
// ---------------------------------------------------------------------------------------------------------------------------------
// (int) rint(min(d2, 16) * 2^14), half to even; -1 for a NaN ("not counted").  +inf gives 2^18; a negative d2 (which the clamp of
// lpd_seq_d2q never hands over) counts as 0.
LPD_SEQ_FN int32_t lpd_seq_quant(float d2)
{
    if (!(d2 == d2)) return -1;
    const float v = fminf(fmaxf(d2, 0.0f), LPD_SEQ_CLAMP);
    return (int32_t)rintf(v * LPD_SEQ_QUANT);
}

// The term of a (query row, database row): qn, dn their squared norms (fmaf chains in channel order), dot the k-ordered fmaf chain
// of the products (what the f32-input MFMA computes).  x = (qn + dn) - (2 * dot), three operations; a NaN x -- a NaN or an inf in
// either row -- is "not counted" (-1), and is looked at BEFORE the clamp at 0, which would otherwise hide it: fmaxf(NaN, 0) is 0.
LPD_SEQ_FN int32_t lpd_seq_d2q(float qn, float dn, float dot)
{
    const float x = (qn + dn) - (2.0f * dot);
    if (!(x == x)) return -1;
    return lpd_seq_quant(fmaxf(x, 0.0f));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// numbering
// ---------------------------------------------------------------------------------------------------------------------------------
// hypothesis e = v (2S + 1) + (s + S): velocity row v of the steps table, shift s in -S .. S of the candidate's row
LPD_SEQ_FN int lpd_seq_hyp(int v, int s, int S) { return v * (2 * S + 1) + (s + S); }
LPD_SEQ_FN int lpd_seq_hyp_v(int e, int S) { return e / (2 * S + 1); }
LPD_SEQ_FN int lpd_seq_hyp_s(int e, int S) { return e % (2 * S + 1) - S; }

// column b' of database row `row` in the block of the candidate whose centre row is j; inside the block iff 0 <= b' <= 30
LPD_SEQ_FN int lpd_seq_band(int row, int j) { return row - j + LPD_SEQ_BAND; }
LPD_SEQ_FN bool lpd_seq_in_band(int bp) { return bp >= 0 && bp <= 2 * LPD_SEQ_BAND; }

// The run of row x: the largest m in [0, nruns) with off[m] <= x (a lower-bound search; empty runs are stepped over).  off [nruns + 1]
// rises from 0; for 0 <= x < off[nruns] the run is [off[m], off[m + 1]) and holds x.  Whatever off holds, 0 <= m < nruns.
LPD_SEQ_FN int lpd_seq_run(const int32_t* off, int nruns, int x)
{
    int lo = 0, hi = nruns;      // off[lo] <= x is assumed (off[0] = 0 <= x), the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

LPD_SEQ_FN bool lpd_seq_in_run(int x, int lo, int hi) { return x >= lo && x < hi; }

// ---------------------------------------------------------------------------------------------------------------------------------
// one term, one hypothesis
// ---------------------------------------------------------------------------------------------------------------------------------
// The term (query row a, database row b, quantised distance dq) is counted iff a lies in the query's run [qlo, qhi), b lies in the
// run [dlo, dhi) of the shifted candidate row, and the distance is not NaN (dq >= 0).
LPD_SEQ_FN bool lpd_seq_counted(int a, int qlo, int qhi, int b, int dlo, int dhi, int32_t dq)
{
    return lpd_seq_in_run(a, qlo, qhi) && lpd_seq_in_run(b, dlo, dhi) && dq >= 0;
}

struct LpdSeqSum { int32_t sum, n; };

// Hypothesis (steps row `st` [2h + 1], shift s) of query row i and candidate centre j over the candidate's block: blk[(t + h) *
// stride + b'] is the quantised distance of query row i + t and database row j - 15 + b', or -1.  [qlo, qhi) is the run of i and
// [dlo, dhi) the run of j, which must hold j + s as well (the caller tests that: lpd_seq_centre_ok).  A term whose b' leaves the block
// -- a table that breaks max|steps| + S <= 15 -- is not counted and nothing is read for it.
LPD_SEQ_FN LpdSeqSum lpd_seq_hypothesis(const int32_t* blk, int stride, const int32_t* st, int h, int s, int i, int qlo, int qhi, int j, int dlo,
                                        int dhi)
{
    LpdSeqSum o = {0, 0};
    for (int t = -h; t <= h; ++t) {
        const int b = j + s + st[t + h];
        const int bp = lpd_seq_band(b, j);
        if (!lpd_seq_in_band(bp)) continue;
        const int32_t dq = blk[(t + h) * stride + bp];
        if (lpd_seq_counted(i + t, qlo, qhi, b, dlo, dhi, dq)) {
            o.sum += dq;
            o.n += 1;
        }
    }
    return o;
}

// the shifted centre j + s must be a row of the table that lies in the run of j: [dlo, dhi) is that run, a part of [0, nd)
LPD_SEQ_FN bool lpd_seq_centre_ok(int j, int s, int dlo, int dhi) { return lpd_seq_in_run(j + s, dlo, dhi); }

// ---------------------------------------------------------------------------------------------------------------------------------
// order
// ---------------------------------------------------------------------------------------------------------------------------------
// (sum1, n1, key1) is better than (sum2, n2, key2): the smaller mean sum / n, compared without a division; equal means go to the
// lower key.  key < 0 marks "none": it loses to everything, and two of them are not ordered (false both ways).  The keys are the
// hypothesis numbers e when a candidate's hypotheses are compared and the ranks r when a query's candidates are: with distinct keys
// this is a strict total order, so every reduction order gives the same winner.
LPD_SEQ_FN bool lpd_seq_better(int32_t sum1, int32_t n1, int key1, int32_t sum2, int32_t n2, int key2)
{
    if (key1 < 0) return false;
    if (key2 < 0) return true;
    const int64_t l = (int64_t)sum1 * (int64_t)n2, r = (int64_t)sum2 * (int64_t)n1;
    return l < r || (l == r && key1 < key2);
}
