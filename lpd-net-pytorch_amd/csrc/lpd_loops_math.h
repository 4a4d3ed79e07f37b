// lpd_loops_math.h -- the arithmetic of lpd_loop_consistency and the integer rules of lpd_loop_select (csrc/lpd_loops.hip): which loops
// are valid, the pair statistic of two loops of one graph (the rigid-motion chain round the cycle through both, its residual by the
// solver's quaternion rule, the two variances with the lever-arm term, the gate), and the packed keys by which the selection ranks
// loops.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/loops_ref.py restates every function
// in numpy, and tests/test_loops_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged.  Compile with
// -ffp-contract=off, as the library is: every product, sum, difference, quotient and square root below is ONE float64 IEEE operation
// rounded once.  Every comparison is written so that a NaN fails it.  The relative pose, the quaternion, the rotation residual and
// the edge test are those of csrc/lpd_pgo_math.h.
#pragma once
#include <stdint.h>

#include "lpd_pgo_math.h"

#define LPD_LOOPS_FN LPD_PGO_FN

#define LPD_LOOPS_THREADS 1024            // threads of a workgroup of the selection: sixteen waves share the candidates of a step
#define LPD_LOOPS_KEY_BITS 12             // a loop's number takes 12 bits of a key: LPD_LOOPS_MAX = 1 << 12
// status (info[0]); the values are in include/lpd_hip.h as LPD_LOOPS_OK .. LPD_LOOPS_TOO_MANY
#define LPD_LOOPS_ST_OK 0
#define LPD_LOOPS_ST_NOTHING 1
#define LPD_LOOPS_ST_TOO_FEW 2
#define LPD_LOOPS_ST_TOO_MANY 3

// A loop is valid iff the solver would use it (lpd_pgo_edge_ok: both ends inside the graph of V nodes and different, a finite
// measurement, finite weights >= 0) and both weights are > 0: their reciprocals are variances.
LPD_LOOPS_FN bool lpd_loops_valid(int i, int j, int V, const double* Z, const double* w)
{
    return lpd_pgo_edge_ok(i, j, V, Z, w) && w[0] > 0.0 && w[1] > 0.0;
}

// out [12] = A B for two poses [12] = (R | t) row-major: R = Ra Rb, t = (Ra tb) + ta
LPD_LOOPS_FN void lpd_loops_mul(const double* A, const double* B, double* out)
{
    for (int r = 0; r < 3; ++r) {
        const double a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2];
        for (int c = 0; c < 3; ++c) out[4 * r + c] = lpd_pgo_dot3(a0, a1, a2, B[c], B[4 + c], B[8 + c]);
        out[4 * r + 3] = lpd_pgo_dot3(a0, a1, a2, B[3], B[7], B[11]) + A[4 * r + 3];
    }
}

// out [12] = X^-1 Y as a pose (lpd_pgo_between, packed)
LPD_LOOPS_FN void lpd_loops_between(const double* X, const double* Y, double* out)
{
    double R[9], t[3];
    lpd_pgo_between(X, Y, R, t);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = R[3 * r + c];
        out[4 * r + 3] = t[r];
    }
}

// |t(X) - t(Y)|^2
LPD_LOOPS_FN double lpd_loops_chord2(const double* X, const double* Y)
{
    const double d0 = X[3] - Y[3], d1 = X[7] - Y[7], d2 = X[11] - Y[11];
    return lpd_pgo_dot3(d0, d1, d2, d0, d1, d2);
}

// The cycle through two valid loops a = (ia, ja, Za) and b = (ib, jb, Zb) of one graph, a the lower number:
//   E = Za (Xja^-1 Xjb) (Xib Zb)^-1 Xia  =  ((Za T1) T2),  T1 = Xja^-1 Xjb,  T2 = (Xib Zb)^-1 Xia,
// the identity when both loops and the odometry between their ends agree.
LPD_LOOPS_FN void lpd_loops_cycle(const double* Xia, const double* Xja, const double* Za, const double* Xib, const double* Xjb, const double* Zb,
                                  double* E)
{
    double T1[12], M1[12], Ab[12], T2[12];
    lpd_loops_between(Xja, Xjb, T1);
    lpd_loops_mul(Za, T1, M1);
    lpd_loops_mul(Xib, Zb, Ab);
    lpd_loops_between(Ab, Xia, T2);
    lpd_loops_mul(M1, T2, E);
}

// its residual r [6] = (2 sgn(q_w) q_xyz of R_E, t_E), the quaternion by the solver's rule
LPD_LOOPS_FN void lpd_loops_residual(const double* Xia, const double* Xja, const double* Za, const double* Xib, const double* Xjb, const double* Zb,
                                     double* r)
{
    double E[12];
    lpd_loops_cycle(Xia, Xja, Za, Xib, Xjb, Zb, E);
    const double Re[9] = {E[0], E[1], E[2], E[4], E[5], E[6], E[8], E[9], E[10]};
    lpd_pgo_rot_residual(Re, r);
    r[3] = E[3];
    r[4] = E[7];
    r[5] = E[11];
}

// The pair statistic: |r_rot|^2 / var_r + |r_t|^2 / var_t with
//   n_i = |ia - ib|, n_j = |ja - jb| (odometry steps between the ends: the nodes of a graph are consecutive windows),
//   c_i^2 = |t(Xia) - t(Xib)|^2, c_j^2 = |t(Xja) - t(Xjb)|^2 (the chords those steps span),
//   var_r = ((1 / wa_rot) + (1 / wb_rot)) + ((n_i + n_j) / w_or),
//   var_t = (((1 / wa_trans) + (1 / wb_trans)) + ((n_i + n_j) / w_ot)) + (((n_i * c_i^2) + (n_j * c_j^2)) / w_or);
// the last term is the lever arm: a heading error at the start of an odometry segment swings the whole chord.
LPD_LOOPS_FN double lpd_loops_stat(const double* Xia, const double* Xja, const double* Za, const double* wa, int ia, int ja, const double* Xib,
                                   const double* Xjb, const double* Zb, const double* wb, int ib, int jb, double w_or, double w_ot)
{
    double r[6];
    lpd_loops_residual(Xia, Xja, Za, Xib, Xjb, Zb, r);
    const double ni = (double)(ia > ib ? ia - ib : ib - ia), nj = (double)(ja > jb ? ja - jb : jb - ja);
    const double nn = ni + nj;
    const double ci2 = lpd_loops_chord2(Xia, Xib), cj2 = lpd_loops_chord2(Xja, Xjb);
    const double var_r = ((1.0 / wa[0]) + (1.0 / wb[0])) + (nn / w_or);
    const double var_t = (((1.0 / wa[1]) + (1.0 / wb[1])) + (nn / w_ot)) + (((ni * ci2) + (nj * cj2)) / w_or);
    const double rr = lpd_pgo_dot3(r[0], r[1], r[2], r[0], r[1], r[2]), tt = lpd_pgo_dot3(r[3], r[4], r[5], r[3], r[4], r[5]);
    return (rr / var_r) + (tt / var_t);
}

// two valid loops agree iff their statistic is within the gate (false for NaN)
LPD_LOOPS_FN bool lpd_loops_consistent(double stat, double gate) { return stat <= gate; }

// ---- the selection's integers ----
// The key by which loops are ranked: a larger count wins, a tie goes to the LOWER loop number u (0 <= count, u < 4096).  -1 is "none".
LPD_LOOPS_FN int lpd_loops_key(int count, int u) { return (count << LPD_LOOPS_KEY_BITS) | (((1 << LPD_LOOPS_KEY_BITS) - 1) - u); }
LPD_LOOPS_FN int lpd_loops_key_loop(int key) { return ((1 << LPD_LOOPS_KEY_BITS) - 1) - (key & ((1 << LPD_LOOPS_KEY_BITS) - 1)); }
// the bits of word w (columns 64 w .. 64 w + 63) that are columns of a graph of P loops
LPD_LOOPS_FN uint64_t lpd_loops_word_mask(int w, int P)
{
    const int left = P - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}
