// lpd_clean_math.h -- the arithmetic of lpd_road_planes / lpd_clean_count / lpd_clean_fill (csrc/lpd_clean.hip): which rows of a raw
// scan are live, the plane through three rows and whether it may stand for the road, the residual of a row, the quantisation and
// the float64 solve of the refinement.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open;
// tests/clean_ref.py restates every function in numpy, and tests/test_clean_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: every product, sum and quotient below is ONE
// IEEE operation rounded once -- a fused multiply-add would move rows across tau and clearance.  Every comparison is written so
// that a NaN fails it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_tuple_math.h"      // lpd_philox4x32_10: the draws of the hypotheses

#if defined(__HIPCC__)
#define LPD_CLEAN_FN __host__ __device__ __forceinline__
#else
#define LPD_CLEAN_FN static inline
#endif

// LPD_CLEAN_MAX_H and LPD_CLEAN_CHUNK (256 threads x LPD_CLEAN_LANE_ROWS) are the public header's
#define LPD_CLEAN_MAX_RANGE 512.0f        // r_max, metres: |dx| <= 1024 m, so |X| <= 2^20 and 2^20 rows x 2^40 < 2^63
#define LPD_CLEAN_MAX_POINTS (1 << 20)    // rows of one scan (LPD_SUBMAP_MAX_POINTS)
#define LPD_CLEAN_LANE_ROWS 4
#define LPD_CLEAN_QSCALE 1024.0f          // quantisation steps per metre (2^-10 m, a little under 1 mm)
#define LPD_CLEAN_QMAX 1048576.0f         // the quantised coordinate is clamped to +-2^20 before the conversion to an integer

// r * r: ONE product (both sides of the range comparison are squares)
LPD_CLEAN_FN float lpd_clean_sq(float r) { return r * r; }

LPD_CLEAN_FN bool lpd_clean_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// 1. Live: finite, r_min^2 <= x^2 + y^2 <= r_max^2, z_lo <= z <= z_hi.  A finite x whose square overflows gives inf: outside every
// r_max <= 512.
LPD_CLEAN_FN bool lpd_clean_live(float x, float y, float z, float rmin2, float rmax2, float z_lo, float z_hi)
{
    const float d = (x * x) + (y * y);
    return lpd_clean_finite(x) && lpd_clean_finite(y) && lpd_clean_finite(z) && d >= rmin2 && d <= rmax2 && z >= z_lo && z <= z_hi;
}

// the seed band of a hypothesis's three rows (a sensor-height prior)
LPD_CLEAN_FN bool lpd_clean_in_band(float z, float lo, float hi) { return z >= lo && z <= hi; }

// 2. row number j of hypothesis h: ((uint64) r * n) >> 32, 0 <= result < n for n >= 1
LPD_CLEAN_FN uint32_t lpd_clean_row(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * (uint64_t)n) >> 32); }

struct LpdCleanRows { uint32_t i[3]; };

LPD_CLEAN_FN LpdCleanRows lpd_clean_draw(uint32_t h, uint32_t b, uint32_t n, uint32_t seed_lo, uint32_t seed_hi)
{
    const LpdPhilox4 r = lpd_philox4x32_10(h, b, 0u, 0u, seed_lo, seed_hi);
    LpdCleanRows o;
    o.i[0] = lpd_clean_row(r.v[0], n);
    o.i[1] = lpd_clean_row(r.v[1], n);
    o.i[2] = lpd_clean_row(r.v[2], n);
    return o;
}

struct LpdCleanPlane { float a, b, c; int valid; };      // z = a x + b y + c

LPD_CLEAN_FN bool lpd_clean_slope_ok(float a, float b, float slope2) { return (a * a) + (b * b) <= slope2; }

// The plane through p0, p1, p2 (three floats each).  ok = the three rows are live and inside the seed band.  valid needs
// |det| >= min_det (twice the triangle's area in plan view) and a^2 + b^2 <= max_slope^2; det == 0 gives inf or NaN slopes, which
// fail the slope test whatever min_det is.  The plane is computed (and returned) whether or not ok holds, from whatever the rows
// contain: only `valid` says that it may be used.
LPD_CLEAN_FN LpdCleanPlane lpd_clean_triple(const float* p0, const float* p1, const float* p2, bool ok, float min_det, float slope2)
{
    const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const float vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const float det = (ux * vy) - (uy * vx);
    LpdCleanPlane P;
    P.a = ((uz * vy) - (vz * uy)) / det;
    P.b = ((ux * vz) - (vx * uz)) / det;
    P.c = p0[2] - ((P.a * p0[0]) + (P.b * p0[1]));
    P.valid = ok && fabsf(det) >= min_det && lpd_clean_slope_ok(P.a, P.b, slope2) && lpd_clean_finite(P.c);
    return P;
}

// 3. / 5. residual of a row: its height above the plane
LPD_CLEAN_FN float lpd_clean_residual(float x, float y, float z, float a, float b, float c) { return z - (((a * x) + (b * y)) + c); }
LPD_CLEAN_FN bool lpd_clean_inlier(float e, float tau) { return fabsf(e) <= tau; }
LPD_CLEAN_FN bool lpd_clean_removed(float e, float clearance) { return e <= clearance; }      // the road and everything under it

// the key of the choice among the valid hypotheses: larger S first, then the lower h.  max over the keys = h*.
LPD_CLEAN_FN long long lpd_clean_choice_key(int S, int h) { return ((long long)S << 10) | (long long)(LPD_CLEAN_MAX_H - 1 - h); }

// 4. quantised offset from the origin, in steps of 2^-10 m: rintf (half to even) of ONE difference times 1024 (exact), clamped to
// +-2^20 so that the conversion is defined for every input (an inlier of a plane within the slope limit never reaches the clamp)
LPD_CLEAN_FN int32_t lpd_clean_quant(float x, float o)
{
    const float q = rintf((x - o) * LPD_CLEAN_QSCALE);
    return (int32_t)fminf(fmaxf(q, -LPD_CLEAN_QMAX), LPD_CLEAN_QMAX);
}

// The least-squares plane of the inliers from their nine integer sums S = (m, SX, SY, SZ, SXX, SXY, SYY, SXZ, SYZ), origin o in
// metres.  Float64, every operation rounded once, in THIS order.  -> 1 and (a, b, c) in fp32 when the refined plane stands, 0 when
// the plane of h* is kept: m < 3, D not positive and finite, or the refined slope (the fp32 values) breaks max_slope.
LPD_CLEAN_FN int lpd_clean_solve(const int64_t* S, float ox, float oy, float oz, float slope2, float* abc)
{
    if (S[0] < 3) return 0;
    const double m = (double)S[0], sx = (double)S[1], sy = (double)S[2], sz = (double)S[3];
    const double sxx = (double)S[4], sxy = (double)S[5], syy = (double)S[6], sxz = (double)S[7], syz = (double)S[8];
    const double cxx = sxx - ((sx * sx) / m);
    const double cxy = sxy - ((sx * sy) / m);
    const double cyy = syy - ((sy * sy) / m);
    const double cxz = sxz - ((sx * sz) / m);
    const double cyz = syz - ((sy * sz) / m);
    const double D = (cxx * cyy) - (cxy * cxy);
    if (!(D > 0.0 && D <= 1.7976931348623157e308)) return 0;
    const double a = ((cxz * cyy) - (cyz * cxy)) / D;
    const double b = ((cyz * cxx) - (cxz * cxy)) / D;
    const double cq = ((sz - (a * sx)) - (b * sy)) / m;      // in quantisation steps, relative to the origin
    const double c = (((double)oz + (cq / 1024.0)) - (a * (double)ox)) - (b * (double)oy);
    const float af = (float)a, bf = (float)b, cf = (float)c;
    if (!(lpd_clean_slope_ok(af, bf, slope2) && lpd_clean_finite(cf))) return 0;
    abc[0] = af;
    abc[1] = bf;
    abc[2] = cf;
    return 1;
}
