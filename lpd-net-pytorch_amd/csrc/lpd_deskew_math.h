// lpd_deskew_math.h -- the arithmetic of lpd_scan_deskew (csrc/lpd_deskew.hip), lpd_drive_motions (the same file) and lpd_odom_motion
// (csrc/lpd_odom.hip): the motion of the sensor during one sweep, what of it depends on the scan alone, and the transform of one row
// into the frame of the sweep's reference time.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open;
// tests/deskew_ref.py restates every function in numpy, and tests/test_deskew_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged.  Compile with
// -ffp-contract=off, as the library is: every product, sum, difference, quotient and square root below is ONE IEEE operation rounded
// once.  A pose or a motion is twelve doubles, the rows of (R | t).  The blended pose is lpd_map_blend's (lpd_map_math.h), the relative
// pose lpd_pgo_between's (lpd_pgo_math.h); nothing of theirs is defined a second time: the split below into a per-scan and a per-row
// part performs lpd_map_blend(identity, motion, a)'s own operations in its own order, and the CPU test holds the two together bit for
// bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_map_math.h"

#define LPD_DESKEW_FN LPD_MAP_FN

// ---- the motions --------------------------------------------------------------------------------------------------------------------------
// out [12] = X^-1 Y as a pose: lpd_pgo_between, packed.  A value of X or Y that is not finite leaves at least one value of out that is
// not finite (every output is a sum of products with it, or of products with a difference that holds it).
LPD_DESKEW_FN void lpd_deskew_between(const double* X, const double* Y, double* out)
{
    double R[9], t[3];
    lpd_pgo_between(X, Y, R, t);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = R[3 * r + c];
        out[4 * r + 3] = t[r];
    }
}

LPD_DESKEW_FN void lpd_deskew_identity(double* out)
{
    for (int k = 0; k < 12; ++k) out[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
}

// lpd_drive_motions: the motion during scan i of a drive with the poses [S][12] -- to the next scan's pose; the last scan repeats the
// motion before it; a drive of one scan does not move.
LPD_DESKEW_FN void lpd_deskew_drive_motion(const double* poses, int S, int i, double* out)
{
    if (S == 1) {
        lpd_deskew_identity(out);
        return;
    }
    const int a = i < S - 1 ? i : S - 2;
    lpd_deskew_between(poses + (size_t)12 * a, poses + (size_t)12 * (a + 1), out);
}

// lpd_odom_motion: the motion during scan t of the odometry, known before the scan is localised -- the one between the two poses before
// it (the constant-velocity model of lpd_odom_predict_pose); for t < 2 first_motion as it is, the identity without one.
LPD_DESKEW_FN void lpd_deskew_odom_motion(const double* poses, int t, const double* first_motion, double* out)
{
    if (t >= 2) {
        lpd_deskew_between(poses + (size_t)12 * (t - 2), poses + (size_t)12 * (t - 1), out);
        return;
    }
    if (first_motion)
        for (int k = 0; k < 12; ++k) out[k] = first_motion[k];
    else
        lpd_deskew_identity(out);
}

// ---- what depends on the scan alone -------------------------------------------------------------------------------------------------------
// lpd_map_blend(A = identity, B = motion, alpha) up to the first use of alpha.  The identity's quaternion is (1, 0, 0, 0) exactly
// (lpd_pgo_quat: trace 3, s = sqrt(4) * 2 = 4, 4 * 0.25 and 0 / 4), its translation 0.  dq = q_B - q_A with q_B negated when the
// four-term dot product with q_A is negative; dt = t_B - 0.  ok: every value of the motion is finite (lpd_map_finite12).
struct LpdDeskewScan {
    double dq[4], dt[3];
    int ok;
};

LPD_DESKEW_FN LpdDeskewScan lpd_deskew_scan(const double* motion)
{
    LpdDeskewScan s;
    s.ok = lpd_map_finite12(motion) ? 1 : 0;
    const double RB[9] = {motion[0], motion[1], motion[2], motion[4], motion[5], motion[6], motion[8], motion[9], motion[10]};
    const double qa[4] = {1.0, 0.0, 0.0, 0.0};
    double qb[4];
    lpd_pgo_quat(RB, qb);
    const double d = (((qa[0] * qb[0]) + (qa[1] * qb[1])) + (qa[2] * qb[2])) + (qa[3] * qb[3]);
    if (d < 0.0)
        for (int k = 0; k < 4; ++k) qb[k] = -qb[k];
    for (int k = 0; k < 4; ++k) s.dq[k] = qb[k] - qa[k];
    for (int r = 0; r < 3; ++r) s.dt[r] = motion[4 * r + 3] - 0.0;
    return s;
}

// ---- one row --------------------------------------------------------------------------------------------------------------------------------
// Is the row transformed?  Its time lies in 0 .. 1 (-0.0 does; a NaN does not) and its scan's motion is finite.  Otherwise it is
// passed through: written as a copy of its input.
LPD_DESKEW_FN int lpd_deskew_row_ok(const LpdDeskewScan& s, float time) { return s.ok && time >= 0.0f && time <= 1.0f; }

// P [12] = lpd_map_blend(identity, motion, a) from the scan's part: q = q_A + a dq, divided by the square root of its squared norm, the
// rotation of q by lpd_map_blend's quadratic form, t = 0 + a dt.  One square root and four divisions a row.
LPD_DESKEW_FN void lpd_deskew_pose(const LpdDeskewScan& s, double a, double* P)
{
    const double q0 = 1.0 + (a * s.dq[0]), q1 = 0.0 + (a * s.dq[1]), q2 = 0.0 + (a * s.dq[2]), q3 = 0.0 + (a * s.dq[3]);
    const double n = sqrt((((q0 * q0) + (q1 * q1)) + (q2 * q2)) + (q3 * q3));
    const double w = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    P[0] = 1.0 - (2.0 * (yy + zz));
    P[1] = 2.0 * (xy - wz);
    P[2] = 2.0 * (xz + wy);
    P[4] = 2.0 * (xy + wz);
    P[5] = 1.0 - (2.0 * (xx + zz));
    P[6] = 2.0 * (yz - wx);
    P[8] = 2.0 * (xz - wy);
    P[9] = 2.0 * (yz + wx);
    P[10] = 1.0 - (2.0 * (xx + yy));
    for (int r = 0; r < 3; ++r) P[4 * r + 3] = 0.0 + (a * s.dt[r]);
}

// one output coordinate: lpd_drive_coord's order in float64, rounded to fp32 ONCE
LPD_DESKEW_FN float lpd_deskew_coord(const double* m, double u, double x, double y, double z) { return (float)((((m[0] * x) + (m[1] * y)) + (m[2] * z)) + u); }

// The row (x, y, z) measured at `time` -> o [3] in the frame of the time `ref`: a = (double) time - ref, o = R_a (x, y, z) + a t.
// Returns 1 for a transformed row, 0 for one passed through.  Under the identity motion R_a = I and a t = 0 exactly, so o compares equal
// to the input (a -0.0 becomes +0.0).
LPD_DESKEW_FN int lpd_deskew_row(const LpdDeskewScan& s, float time, double ref, float x, float y, float z, float* o)
{
    if (!lpd_deskew_row_ok(s, time)) {
        o[0] = x;
        o[1] = y;
        o[2] = z;
        return 0;
    }
    double P[12];
    lpd_deskew_pose(s, (double)time - ref, P);
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    o[0] = lpd_deskew_coord(P + 0, P[3], xd, yd, zd);
    o[1] = lpd_deskew_coord(P + 4, P[7], xd, yd, zd);
    o[2] = lpd_deskew_coord(P + 8, P[11], xd, yd, zd);
    return 1;
}
