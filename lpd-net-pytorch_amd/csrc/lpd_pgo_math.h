// lpd_pgo_math.h -- the arithmetic of lpd_pgo_solve (csrc/lpd_pgo.hip): the relative pose of two nodes, the residual of an edge (the
// unit quaternion of a rotation by Shepperd's largest-of-four branch), its chi-squared, the Huber cost and its IRLS weight, the
// first-order Jacobians of the two ends, the products J u, J^T s and J^T W J, the damped block solve of the preconditioner, the
// retraction, the Levenberg-Marquardt bookkeeping and the layout of the workspace.
// THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/pgo_ref.py restates every function in numpy,
// and tests/test_posegraph_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernel includes it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: every product, sum, difference, quotient and
// square root below is ONE float64 IEEE operation rounded once.  Every comparison is written so that a NaN fails it.  No trigonometric
// function.  A dot product of three is ((a0*b0) + (a1*b1)) + (a2*b2); a dot product of six continues the same chain to the right.
//
// The 6 x 6 solve (lpd_icp_ldl6) and the rotation of a small step (lpd_icp_dR) are those of csrc/lpd_icp_math.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lpd_icp_math.h"

#define LPD_PGO_FN LPD_ICP_FN

#define LPD_PGO_THREADS 256               // threads of the one workgroup that solves a graph: the stride of every partial sum
#define LPD_PGO_NODE_WS 69                // float64 per node: trial pose 12, g 6, D 21, x r z p Ap 6 each
#define LPD_PGO_EDGE_WS 50                // float64 per edge: A B C Re 9 each, residual 6, IRLS-scaled weights 2, s 6
#define LPD_PGO_FTOL 1e-12                // an accepted step that lowers the cost by no more than FTOL * cost ends the solve: converged
#define LPD_PGO_XTOL 1e-12                // a solution x of a trial with x'x <= XTOL * XTOL is not applied: converged
#define LPD_PGO_LAMBDA_MIN 1e-9           // the least lambda a refusal leaves behind
// status (info[0]); the values are in include/lpd_hip.h as LPD_PGO_CONVERGED .. LPD_PGO_REFUSED
#define LPD_PGO_ST_CONVERGED 0
#define LPD_PGO_ST_ITERATIONS 1
#define LPD_PGO_ST_NOTHING 2
#define LPD_PGO_ST_REFUSED 3

LPD_PGO_FN double lpd_pgo_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return ((a0 * b0) + (a1 * b1)) + (a2 * b2); }

LPD_PGO_FN double lpd_pgo_dot6(const double* a, const double* b)
{
    return (((((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])) + (a[3] * b[3])) + (a[4] * b[4])) + (a[5] * b[5]);
}

// An edge is used iff both ends lie in its graph of V nodes and differ, all twelve entries of its measurement are finite and both
// weights are finite and >= 0.  Z and w are read only when the ends pass.
LPD_PGO_FN bool lpd_pgo_edge_ok(int i, int j, int V, const double* Z, const double* w)
{
    if (!(i >= 0 && i < V && j >= 0 && j < V && i != j)) return false;
    bool ok = true;
    for (int a = 0; a < 12; ++a) ok = ok && lpd_icp_finite64(Z[a]);
    return ok && lpd_icp_finite64(w[0]) && lpd_icp_finite64(w[1]) && w[0] >= 0.0 && w[1] >= 0.0;
}

// (R [9], t [3]) = X^-1 Y for two poses [12] = (R | t) row-major: R = Rx^T Ry, t = Rx^T (ty - tx)
LPD_PGO_FN void lpd_pgo_between(const double* X, const double* Y, double* R, double* t)
{
    const double d0 = Y[3] - X[3], d1 = Y[7] - X[7], d2 = Y[11] - X[11];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = lpd_pgo_dot3(X[r], X[4 + r], X[8 + r], Y[c], Y[4 + c], Y[8 + c]);
        t[r] = lpd_pgo_dot3(X[r], X[4 + r], X[8 + r], d0, d1, d2);
    }
}

// q [4] = (w, x, y, z) of the rotation R [9], by the branch of the largest of (trace, R00, R11, R22); a later entry wins only when
// strictly larger, so a tie goes to the earlier one and a NaN never wins.  Returns the branch.  The sign is the branch's own.
LPD_PGO_FN int lpd_pgo_quat(const double* R, double* q)
{
    const double tr = (R[0] + R[4]) + R[8];
    const double c[4] = {tr, R[0], R[4], R[8]};
    int m = 0;
    double best = c[0];
    for (int a = 1; a < 4; ++a)
        if (c[a] > best) {
            best = c[a];
            m = a;
        }
    if (m == 0) {
        const double s = sqrt(1.0 + tr) * 2.0;
        q[0] = s * 0.25; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (m == 1) {
        const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
        q[0] = (R[7] - R[5]) / s; q[1] = s * 0.25; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (m == 2) {
        const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = s * 0.25; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = s * 0.25;
    }
    return m;
}

// r [3] = 2 sgn(q_w) (q_x, q_y, q_z); sgn(0) = +1
LPD_PGO_FN void lpd_pgo_rot_residual(const double* R, double* r)
{
    double q[4];
    lpd_pgo_quat(R, q);
    const bool neg = q[0] < 0.0;
    for (int a = 0; a < 3; ++a) {
        const double v = 2.0 * q[1 + a];
        r[a] = neg ? -v : v;
    }
}

// The residual r [6] of an edge and what its Jacobians are made of, jc [36] = (A, B, C, Re), 3 x 3 row-major each:
//   T = Xi^-1 Xj, E = Z^-1 T = (Re, te), r = (rot_residual(Re), te), A = R_T^T, C = R_Z^T, B = C [t_T]x.
LPD_PGO_FN void lpd_pgo_edge(const double* Xi, const double* Xj, const double* Z, double* jc, double* r)
{
    double RT[9], tT[3], Zr[12];
    lpd_pgo_between(Xi, Xj, RT, tT);
    const double Tp[12] = {RT[0], RT[1], RT[2], tT[0], RT[3], RT[4], RT[5], tT[1], RT[6], RT[7], RT[8], tT[2]};
    for (int a = 0; a < 12; ++a) Zr[a] = Z[a];
    lpd_pgo_between(Zr, Tp, jc + 27, r + 3);
    lpd_pgo_rot_residual(jc + 27, r);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            jc[3 * a + b] = RT[3 * b + a];
            jc[18 + 3 * a + b] = Zr[4 * b + a];
        }
    for (int a = 0; a < 3; ++a) {
        const double c0 = jc[18 + 3 * a], c1 = jc[19 + 3 * a], c2 = jc[20 + 3 * a];
        jc[9 + 3 * a] = (c1 * tT[2]) - (c2 * tT[1]);
        jc[10 + 3 * a] = (c2 * tT[0]) - (c0 * tT[2]);
        jc[11 + 3 * a] = (c0 * tT[1]) - (c1 * tT[0]);
    }
}

// the residual alone (the exact cost of a trial step)
LPD_PGO_FN void lpd_pgo_residual(const double* Xi, const double* Xj, const double* Z, double* r)
{
    double jc[36];
    lpd_pgo_edge(Xi, Xj, Z, jc, r);
}

LPD_PGO_FN double lpd_pgo_chi2(const double* r, double w_rot, double w_trans)
{
    return (w_rot * lpd_pgo_dot3(r[0], r[1], r[2], r[0], r[1], r[2])) + (w_trans * lpd_pgo_dot3(r[3], r[4], r[5], r[3], r[4], r[5]));
}

// rho(s): s itself without a threshold (huber <= 0); else Huber's function of a = sqrt(s): s for a <= huber, 2 huber a - huber^2 beyond
LPD_PGO_FN double lpd_pgo_rho(double s, double huber)
{
    if (!(huber > 0.0)) return s;
    const double a = sqrt(s);
    return a > huber ? ((2.0 * huber) * a) - (huber * huber) : s;
}

// rho'(s): the factor on both weights of an edge at a linearisation
LPD_PGO_FN double lpd_pgo_irls(double s, double huber)
{
    if (!(huber > 0.0)) return 1.0;
    const double a = sqrt(s);
    return a > huber ? huber / a : 1.0;
}

// J [36] row-major = d r / d (w, v) of one end, to first order (J_r^-1 ~ I): end 0 (node i) [[-A, 0], [B, -C]], end 1 (node j)
// [[I, 0], [0, Re]]
LPD_PGO_FN void lpd_pgo_jac(const double* jc, int end, double* J)
{
    for (int a = 0; a < 36; ++a) J[a] = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            if (end == 0) {
                J[6 * a + b] = -jc[3 * a + b];
                J[6 * (3 + a) + b] = jc[9 + 3 * a + b];
                J[6 * (3 + a) + 3 + b] = -jc[18 + 3 * a + b];
            } else {
                J[6 * a + b] = a == b ? 1.0 : 0.0;
                J[6 * (3 + a) + 3 + b] = jc[27 + 3 * a + b];
            }
        }
}

// s [6] = W (Ji pi + Jj pj): each row the six-term chain over Ji, plus the six-term chain over Jj, times its weight
LPD_PGO_FN void lpd_pgo_ju(const double* jc, const double* w, const double* pi, const double* pj, double* s)
{
    double Ji[36], Jj[36];
    lpd_pgo_jac(jc, 0, Ji);
    lpd_pgo_jac(jc, 1, Jj);
    for (int a = 0; a < 6; ++a) s[a] = (a < 3 ? w[0] : w[1]) * (lpd_pgo_dot6(Ji + 6 * a, pi) + lpd_pgo_dot6(Jj + 6 * a, pj));
}

// s [6] = W r
LPD_PGO_FN void lpd_pgo_wr(const double* r, const double* w, double* s)
{
    for (int a = 0; a < 6; ++a) s[a] = (a < 3 ? w[0] : w[1]) * r[a];
}

// o [6] = J^T s: column c the six-term chain over the rows
LPD_PGO_FN void lpd_pgo_jt(const double* J, const double* s, double* o)
{
    for (int c = 0; c < 6; ++c)
        o[c] = (((((J[c] * s[0]) + (J[6 + c] * s[1])) + (J[12 + c] * s[2])) + (J[18 + c] * s[3])) + (J[24 + c] * s[4])) + (J[30 + c] * s[5]);
}

// blk [21] = the upper triangle of J^T W J, row-major (r <= c): the six-term chain over the rows a of (w_a J[a][r]) J[a][c]
LPD_PGO_FN void lpd_pgo_jtwj(const double* J, const double* w, double* blk)
{
    int e = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) {
            double acc = (w[0] * J[r]) * J[c];
            for (int a = 1; a < 6; ++a) acc = acc + (((a < 3 ? w[0] : w[1]) * J[6 * a + r]) * J[6 * a + c]);
            blk[e++] = acc;
        }
}

// the diagonal entry a of a block [21]
LPD_PGO_FN double lpd_pgo_diag(const double* D, int a)
{
    const int at[6] = {0, 6, 11, 15, 18, 20};
    return D[at[a]];
}

// z = (D + lambda diag(D))^-1 r for a diagonal block D [21]: the damped diagonal is D_aa + (lambda * D_aa).  Returns 0, z untouched,
// when a pivot is not positive and finite or an entry of z is not finite.
LPD_PGO_FN int lpd_pgo_precond(const double* D, double lambda, const double* r, double* z)
{
    double A[6][6], o[6];
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = D[e++];
    for (int a = 0; a < 6; ++a) A[a][a] = A[a][a] + (lambda * A[a][a]);
    if (!lpd_icp_ldl6(A, r, o)) return 0;
    for (int a = 0; a < 6; ++a)
        if (!lpd_icp_finite64(o[a])) return 0;
    for (int a = 0; a < 6; ++a) z[a] = o[a];
    return 1;
}

// out [12] = the pose moved by x = (w, v) on the right: R <- R dR(w), t <- t + R v.  Returns 0 when x or the new pose is not finite
// (out is then not to be used).
LPD_PGO_FN int lpd_pgo_retract(const double* pose, const double* x, double* out)
{
    double dR[3][3];
    lpd_icp_dR(x, dR);
    bool ok = true;
    for (int a = 0; a < 6; ++a) ok = ok && lpd_icp_finite64(x[a]);
    for (int i = 0; i < 3; ++i) {
        const double r0 = pose[4 * i], r1 = pose[4 * i + 1], r2 = pose[4 * i + 2];
        for (int j = 0; j < 3; ++j) out[4 * i + j] = lpd_pgo_dot3(r0, r1, r2, dR[0][j], dR[1][j], dR[2][j]);
        out[4 * i + 3] = pose[4 * i + 3] + lpd_pgo_dot3(r0, r1, r2, x[3], x[4], x[5]);
    }
    for (int a = 0; a < 12; ++a) ok = ok && lpd_icp_finite64(out[a]);
    return ok ? 1 : 0;
}

// Levenberg-Marquardt: a trial step is accepted iff its exact cost is below the current one (false for NaN)
LPD_PGO_FN bool lpd_pgo_accept(double cost, double trial) { return trial < cost; }
LPD_PGO_FN bool lpd_pgo_converged(double cost, double trial) { return (cost - trial) <= LPD_PGO_FTOL * cost; }
LPD_PGO_FN bool lpd_pgo_small_step(double xx) { return xx <= LPD_PGO_XTOL * LPD_PGO_XTOL; }
LPD_PGO_FN double lpd_pgo_lambda_down(double lambda) { return lambda * 0.1; }
LPD_PGO_FN double lpd_pgo_lambda_up(double lambda)
{
    const double l = lambda * 10.0;
    return l > LPD_PGO_LAMBDA_MIN ? l : LPD_PGO_LAMBDA_MIN;
}
// conjugate gradients go on while r'z > (cg_tol * cg_tol) * (r'z at the start); false for NaN
LPD_PGO_FN bool lpd_pgo_cg_continue(double rz, double rz0, double cg_tol) { return rz > (cg_tol * cg_tol) * rz0; }
