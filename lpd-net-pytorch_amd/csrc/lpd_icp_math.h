// lpd_icp_math.h -- the arithmetic of lpd_point_normals and lpd_icp_pairs (csrc/lpd_icp.hip): the unit normal of a neighbourhood
// from its centred moments (the three-row form of lpd_feat_math.h's Jacobi), the fp32 transform of a point by a float64 pose, the
// squared distance and the dmax decision of the correspondence search, the quantised point-to-plane row (J, r), the layout of the
// 29 integer sums, and the float64 step: unpivoted LDL^T of the 6 x 6 normal equations and the pose update by a unit quaternion
// (lpd_icp_ldl6 and lpd_icp_dR, which csrc/lpd_pgo_math.h shares).
// THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/icp_ref.py restates every function in
// numpy, and tests/test_icp_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: every product, sum, difference, quotient and
// square root below is ONE IEEE operation rounded once, in fp32 or float64 as written.  Every comparison is written so that a NaN
// fails it.  No trigonometric function.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#include "lpd_feat_math.h"

#if defined(__HIPCC__)
#define LPD_ICP_FN __host__ __device__ __forceinline__
#else
#define LPD_ICP_FN static inline
#endif

// LPD_ICP_MAX_POINTS, LPD_ICP_MAX_PAIRS, LPD_ICP_MAX_ITERS, LPD_ICP_MIN_INLIERS and LPD_ICP_SUMS are the public header's
#define LPD_ICP_MAX_DMAX 16.0f            // metres
#define LPD_ICP_RANGE 512.0f              // a transformed point beyond +-512 m on any axis has no correspondence
#define LPD_ICP_Q 1024.0f                 // quantisation steps per unit of J and r
#define LPD_ICP_CLAMP 1048576.0f          // 2^20: |Ji|, |ri| <= 2^20, a product <= 2^40
#define LPD_ICP_SUM_M 0                   // the count
#define LPD_ICP_SUM_H 1                   // 21 entries sum Ji_a Ji_b, a <= b, row-major over the upper triangle
#define LPD_ICP_SUM_G 22                  // 6 entries sum Ji_a ri
#define LPD_ICP_SUM_RR 28                 // sum ri ri

LPD_ICP_FN bool lpd_icp_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf
LPD_ICP_FN bool lpd_icp_finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// ---------------------------------------------------------------------------------------------------------------------------------
// normals
// ---------------------------------------------------------------------------------------------------------------------------------
// One rotation of lpd_feat_math.h applied to all three rows of V.  lpd_feat_rotate carries one row; it is a pure function, so the
// rows 0 and 1 ride through calls on copies of the matrix entries and row 2 through the call that updates them: the matrix and the
// z row are bit for bit what lpd_feat_eig computes.
LPD_ICP_FN void lpd_icp_rotate3(float& app, float& aqq, float& apq, float& arp, float& arq, float* vp, float* vq)
{
    for (int r = 0; r < 2; ++r) {
        float a = app, b = aqq, c = apq, d = arp, e = arq;
        lpd_feat_rotate(a, b, c, d, e, vp[r], vq[r]);
    }
    lpd_feat_rotate(app, aqq, apq, arp, arq, vp[2], vq[2]);
}

// n [3] = the unit eigenvector of the smallest eigenvalue of the neighbourhood's covariance (the sign is what the sweeps give),
// *flat = l3 / l2 (0 where l2 == 0).  (0, 0, 0) and 0 when a moment is not finite (a coordinate was NaN or inf, or a square
// overflowed), when the neighbourhood has no extent (l1 == 0), or when the eigenvector's length is 0 or not finite.
LPD_ICP_FN void lpd_icp_normal(const LpdFeatMoments& m, int k, float* n, float* flat)
{
    const LpdFeatCov S = lpd_feat_cov(m, k);
    float a0 = S.xx, a1 = S.yy, a2 = S.zz, a01 = S.xy, a02 = S.xz, a12 = S.yz;
    float c0[3] = {1.0f, 0.0f, 0.0f}, c1[3] = {0.0f, 1.0f, 0.0f}, c2[3] = {0.0f, 0.0f, 1.0f};      // the COLUMNS of V = I; c[r] = row r
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < LPD_FEAT_SWEEPS; ++sweep) {
        lpd_icp_rotate3(a0, a1, a01, a02, a12, c0, c1);      // (0, 1), r = 2
        lpd_icp_rotate3(a0, a2, a02, a01, a12, c0, c2);      // (0, 2), r = 1
        lpd_icp_rotate3(a1, a2, a12, a01, a02, c1, c2);      // (1, 2), r = 0
    }
    const float l1 = fmaxf(fmaxf(a0, fmaxf(a1, a2)), 0.0f);
    const float l3 = fmaxf(fminf(a0, fminf(a1, a2)), 0.0f);
    const float l2 = fmaxf(fmaxf(fminf(a0, a1), fminf(fmaxf(a0, a1), a2)), 0.0f);
    const bool first = a0 <= a1 && a0 <= a2, second = a1 <= a2;      // lpd_feat_eig's choice of the column
    const float x = first ? c0[0] : (second ? c1[0] : c2[0]);
    const float y = first ? c0[1] : (second ? c1[1] : c2[1]);
    const float z = first ? c0[2] : (second ? c1[2] : c2[2]);
    const float len = sqrtf(((x * x) + (y * y)) + (z * z));
    const bool fin = lpd_icp_finite(m.sx) && lpd_icp_finite(m.sy) && lpd_icp_finite(m.sz) && lpd_icp_finite(m.sxx) && lpd_icp_finite(m.sxy) &&
                     lpd_icp_finite(m.sxz) && lpd_icp_finite(m.syy) && lpd_icp_finite(m.syz) && lpd_icp_finite(m.szz);
    const bool ok = fin && l1 > 0.0f && len > 0.0f && lpd_icp_finite(len);
    n[0] = ok ? x / len : 0.0f;
    n[1] = ok ? y / len : 0.0f;
    n[2] = ok ? z / len : 0.0f;
    *flat = ok && l2 > 0.0f ? l3 / l2 : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// one pass
// ---------------------------------------------------------------------------------------------------------------------------------
struct LpdIcpPose32 { float m[9], u[3]; };      // the pose rounded to fp32 once: rows of M, then u

LPD_ICP_FN LpdIcpPose32 lpd_icp_pose32(const double* pose)
{
    LpdIcpPose32 o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.m[3 * r + c] = (float)pose[4 * r + c];
        o.u[r] = (float)pose[4 * r + 3];
    }
    return o;
}

// p = M (x, y, z) sc + u.  false: p is not finite or lies beyond +-512 on an axis -- the point has no correspondence.
LPD_ICP_FN bool lpd_icp_transform(const LpdIcpPose32& T, float x, float y, float z, float sc, float* p)
{
    const float ax = x * sc, ay = y * sc, az = z * sc;
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        p[c] = (((T.m[3 * c] * ax) + (T.m[3 * c + 1] * ay)) + (T.m[3 * c + 2] * az)) + T.u[c];
        ok = ok && fabsf(p[c]) <= LPD_ICP_RANGE;      // false for NaN and inf as well
    }
    return ok;
}

LPD_ICP_FN float lpd_icp_d2(float qx, float qy, float qz, float px, float py, float pz)
{
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// The running minimum of the search: candidates are visited in ascending j, a later one wins only when strictly nearer, a NaN or
// +inf distance never wins.  The start is (+inf, -1).
LPD_ICP_FN bool lpd_icp_nearer(float d2, float best) { return d2 < best; }

LPD_ICP_FN bool lpd_icp_within(float d2, float dmax) { return d2 <= dmax * dmax; }

LPD_ICP_FN bool lpd_icp_normal_zero(float nx, float ny, float nz) { return nx == 0.0f && ny == 0.0f && nz == 0.0f; }

// (int64) rint(v * 1024) clamped to +-2^20, half to even; NaN gives 0
LPD_ICP_FN int64_t lpd_icp_quant(float v)
{
    float s = v * LPD_ICP_Q;
    s = s > LPD_ICP_CLAMP ? LPD_ICP_CLAMP : s;
    s = s < -LPD_ICP_CLAMP ? -LPD_ICP_CLAMP : s;
    return s == s ? (int64_t)rintf(s) : 0;      // the conversion only of a finite value in range
}

// The row of a correspondence: Ji [6] = the quantised (p x n, n), *ri = the quantised (q - p) . n
LPD_ICP_FN void lpd_icp_row(const float* p, const float* q, const float* n, int64_t* Ji, int64_t* ri)
{
    const float ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
    const float r = ((ex * n[0]) + (ey * n[1])) + (ez * n[2]);
    Ji[0] = lpd_icp_quant((p[1] * n[2]) - (p[2] * n[1]));
    Ji[1] = lpd_icp_quant((p[2] * n[0]) - (p[0] * n[2]));
    Ji[2] = lpd_icp_quant((p[0] * n[1]) - (p[1] * n[0]));
    Ji[3] = lpd_icp_quant(n[0]);
    Ji[4] = lpd_icp_quant(n[1]);
    Ji[5] = lpd_icp_quant(n[2]);
    *ri = lpd_icp_quant(r);
}

// what a correspondence adds to the 29 sums; t [LPD_ICP_SUMS] (entries 29..31 are not touched)
LPD_ICP_FN void lpd_icp_terms(const int64_t* Ji, int64_t ri, int64_t* t)
{
    t[LPD_ICP_SUM_M] = 1;
    int e = LPD_ICP_SUM_H;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) t[e++] = Ji[a] * Ji[b];
    for (int a = 0; a < 6; ++a) t[LPD_ICP_SUM_G + a] = Ji[a] * ri;
    t[LPD_ICP_SUM_RR] = ri * ri;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the step, float64
// ---------------------------------------------------------------------------------------------------------------------------------
// A x = g by an unpivoted LDL^T of a symmetric 6 x 6 A (both triangles filled).  Returns 0 and leaves x alone when a pivot is not
// positive and finite.  lpd_pgo_math.h inverts its diagonal blocks with this routine as well.
LPD_ICP_FN int lpd_icp_ldl6(const double (*A)[6], const double* g, double* x)
{
    double L[6][6], D[6], v[6], y[6];
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) {
            v[k] = L[j][k] * D[k];
            d = d - (L[j][k] * v[k]);
        }
        if (!(d > 0.0 && lpd_icp_finite64(d))) return 0;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - (L[i][k] * v[k]);
            L[i][j] = s / d;
        }
    }
    for (int i = 0; i < 6; ++i) {      // L y = g, then z = y / D
        double s = g[i];
        for (int k = 0; k < i; ++k) s = s - (L[i][k] * y[k]);
        y[i] = s;
    }
    for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
    for (int i = 5; i >= 0; --i) {     // L^T x = z
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - (L[k][i] * x[k]);
        x[i] = s;
    }
    return 1;
}

// H x = g, H = sum Ji Ji^T, g = sum Ji ri (the factor 1024^2 is on both sides: x is in radians and metres).  Returns 0 and leaves x
// alone when a pivot is not positive and finite.
LPD_ICP_FN int lpd_icp_ldl(const int64_t* sums, double* x)
{
    double A[6][6], g[6];
    int e = LPD_ICP_SUM_H;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = (double)sums[e++];
    for (int i = 0; i < 6; ++i) g[i] = (double)sums[LPD_ICP_SUM_G + i];
    return lpd_icp_ldl6(A, g, x);
}

// dR [3][3] = the rotation of the unit quaternion (1, w / 2) / |(1, w / 2)|, w = x[0..2]
LPD_ICP_FN void lpd_icp_dR(const double* x, double (*dR)[3])
{
    const double hx = x[0] * 0.5, hy = x[1] * 0.5, hz = x[2] * 0.5;
    const double len = sqrt(((1.0 + (hx * hx)) + (hy * hy)) + (hz * hz));
    const double qw = 1.0 / len, qx = hx / len, qy = hy / len, qz = hz / len;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    dR[0][0] = 1.0 - (2.0 * (yy + zz)); dR[0][1] = 2.0 * (xy - wz); dR[0][2] = 2.0 * (xz + wy);
    dR[1][0] = 2.0 * (xy + wz); dR[1][1] = 1.0 - (2.0 * (xx + zz)); dR[1][2] = 2.0 * (yz - wx);
    dR[2][0] = 2.0 * (xz - wy); dR[2][1] = 2.0 * (yz + wx); dR[2][2] = 1.0 - (2.0 * (xx + yy));
}

// pose [12] = (R | t) row-major <- (dR R | dR t + dt), dR the rotation of the unit quaternion (1, w / 2) / |(1, w / 2)|
LPD_ICP_FN void lpd_icp_update(const double* x, double* pose)
{
    double dR[3][3];
    lpd_icp_dR(x, dR);
    double out[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) out[4 * i + j] = ((dR[i][0] * pose[j]) + (dR[i][1] * pose[4 + j])) + (dR[i][2] * pose[8 + j]);
        out[4 * i + 3] = out[4 * i + 3] + x[3 + i];
    }
    for (int i = 0; i < 12; ++i) pose[i] = out[i];
}

// One step from a pass's sums.  Returns 1 and updates the pose, or 0 -- fewer than min_inliers correspondences, a pivot that is not
// positive and finite, or a solution or a new pose that is not finite -- and leaves the pose bit for bit as it is.
LPD_ICP_FN int lpd_icp_solve(const int64_t* sums, int min_inliers, double* pose)
{
    if (sums[LPD_ICP_SUM_M] < (int64_t)min_inliers) return 0;
    double x[6], np[12];
    if (!lpd_icp_ldl(sums, x)) return 0;
    for (int i = 0; i < 6; ++i)
        if (!lpd_icp_finite64(x[i])) return 0;
    for (int i = 0; i < 12; ++i) np[i] = pose[i];
    lpd_icp_update(x, np);
    for (int i = 0; i < 12; ++i)
        if (!lpd_icp_finite64(np[i])) return 0;
    for (int i = 0; i < 12; ++i) pose[i] = np[i];
    return 1;
}
