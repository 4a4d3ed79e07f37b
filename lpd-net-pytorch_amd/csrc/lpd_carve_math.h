// lpd_carve_math.h -- the arithmetic of lpd_map_pierce / lpd_map_carve / lpd_scan_moving (csrc/lpd_carve.hip): the record of a scan
// (its rigid transform, its sensor position, whether its rays are traversed), the integer walk of a ray through the cells between the
// sensor and the endpoint, which of the cells stepped into are looked up, the pierce rule at a found cell, and when a cell counts as
// MOVING.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/carve_ref.py restates every function
// in numpy, and tests/test_carve_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged.  Compile with
// -ffp-contract=off, as the library is: every operation is ONE IEEE operation rounded once, in fp32 or float64 as written.  The world
// row, the cell, the key and the pose of a scan are lpd_map_math.h's; the lookup and the surf row are lpd_loc_math.h's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_loc_math.h"
#include "lpd_map_math.h"

#define LPD_CARVE_FN LPD_MAP_FN

// LPD_CARVE_MAX_SKIP, LPD_CARVE_MAX_STEPS, LPD_CARVE_RATIO_UNITS and LPD_CARVE_MAX_RATIO_Q are the public header's
#define LPD_CARVE_SUB 512      // units of a cell in the walk: cell walls are the multiples of 512

// ---- one scan ----------------------------------------------------------------------------------------------------------------------------
// r = lpd_map_rel(pose, origin), the insert's; o = r.u is the sensor; e_c = o_c * inv_cell in fp32, the very product lpd_map_index floors.
// ok: the pose is finite and o has a cell -- the rows of every other scan are dropped.
struct LpdCarveScan {
    LpdDriveRel r;
    float e[3];
    int ok;
};

LPD_CARVE_FN LpdCarveScan lpd_carve_scan(const double* pose, const double* origin, float inv_cell)
{
    LpdCarveScan s;
    s.r = lpd_map_rel(pose, origin);
    int q[3];
    bool ok = lpd_map_finite12(pose);
    for (int c = 0; c < 3; ++c) {
        s.e[c] = s.r.u[c] * inv_cell;
        ok = lpd_map_index(s.r.u[c], inv_cell, q + c) && ok;
    }
    s.ok = ok ? 1 : 0;
    return s;
}

// ---- the walk, in integers ---------------------------------------------------------------------------------------------------------------
// f = a coordinate in cells (fp32, |floorf(f)| <= 2^20) -> its position in units of 1/512 cell, always ODD: never on a cell wall.
// (double) f * 256 is exact; A >> 9 == (int) floorf(f).
LPD_CARVE_FN int64_t lpd_carve_sub(float f) { return 2 * (int64_t)floor((double)f * 256.0) + 1; }

// A ray from B (the sensor) to A (the endpoint).  q is the cell the walk stands in, N_c the distance from B_c to the next wall on axis
// c in units of 1/512 cell, D = A - B, s = sign(D), n = the walls between the two cells.
struct LpdCarveRay {
    int64_t D[3], N[3];      // |D_c| <= 2^30, N_c <= 2^30 + 512: a product of the two fits an int64
    int q[3], s[3], qa[3], qb[3];
    int64_t n;
};

// f [3] = w_c * inv_cell of the endpoint, e [3] = o_c * inv_cell of the sensor; both have a cell
LPD_CARVE_FN void lpd_carve_ray(const float* f, const float* e, LpdCarveRay* r)
{
    r->n = 0;
    for (int c = 0; c < 3; ++c) {
        const int64_t A = lpd_carve_sub(f[c]), B = lpd_carve_sub(e[c]);
        const int qa = (int)(A >> 9), qb = (int)(B >> 9);
        const int64_t D = A - B;
        const int s = D > 0 ? 1 : (D < 0 ? -1 : 0);
        const int64_t W = (int64_t)LPD_CARVE_SUB * ((int64_t)qb + (s > 0 ? 1 : 0)), N = W - B;
        r->D[c] = D < 0 ? -D : D;
        r->N[c] = N < 0 ? -N : N;
        r->s[c] = s;
        r->q[c] = r->qb[c] = qb;
        r->qa[c] = qa;
        r->n += qa > qb ? (int64_t)qa - qb : (int64_t)qb - qa;
    }
}

// One step: the axis whose next wall comes first along the ray, N_i |D_j| < N_j |D_i| by cross-multiplication; ties go to the lowest
// axis; an axis with D_c == 0 is never taken.  -> the axis (-1 for a ray that has none: D == 0); q is then the cell stepped into.
LPD_CARVE_FN int lpd_carve_step(LpdCarveRay* r)
{
    int b = -1;
    int64_t Nb = 0, Db = 0;      // the best axis so far, kept as values: no array is indexed by a run-time axis, so the record stays in registers
    for (int c = 0; c < 3; ++c) {
        const bool take = r->D[c] != 0 && (b < 0 || r->N[c] * Db < Nb * r->D[c]);
        b = take ? c : b;
        Nb = take ? r->N[c] : Nb;
        Db = take ? r->D[c] : Db;
    }
    if (b < 0) return b;
    for (int c = 0; c < 3; ++c) {
        r->q[c] += b == c ? r->s[c] : 0;
        r->N[c] += b == c ? (int64_t)LPD_CARVE_SUB : 0;
    }
    return b;
}

// the cells stepped into: those after steps 1 .. min(n - 1, max_steps) -- neither the sensor's cell nor the endpoint's
LPD_CARVE_FN int64_t lpd_carve_visits(int64_t n, int max_steps)
{
    const int64_t v = n - 1;
    return v < 0 ? 0 : (v > (int64_t)max_steps ? (int64_t)max_steps : v);
}

LPD_CARVE_FN int lpd_carve_cut(int64_t n, int max_steps) { return n - 1 > (int64_t)max_steps; }

LPD_CARVE_FN int lpd_carve_cheb(const int* a, const int* b)
{
    int d = 0;
    for (int c = 0; c < 3; ++c) {
        const int v = a[c] > b[c] ? a[c] - b[c] : b[c] - a[c];
        d = v > d ? v : d;
    }
    return d;
}

// is the cell q (stepped into) looked up?  Not when it is nearer than skip_end cells (Chebyshev) to the endpoint's cell or nearer than
// skip_start to the sensor's.
LPD_CARVE_FN int lpd_carve_looked(const int* q, const int* qa, const int* qb, int skip_end, int skip_start)
{
    return lpd_carve_cheb(q, qa) >= skip_end && lpd_carve_cheb(q, qb) >= skip_start;
}

// ---- the pierce rule ---------------------------------------------------------------------------------------------------------------------
// a surf row (cx, cy, cz, nx, ny, nz, flatness, .) is reliable iff it has a normal and is flat enough
LPD_CARVE_FN int lpd_carve_reliable(const float* row, float max_flat) { return !lpd_icp_normal_zero(row[3], row[4], row[5]) && row[6] <= max_flat; }

// n . (a - b) in float64 on fp32 values: three differences, then the dot product ((n0 d0) + (n1 d1)) + (n2 d2)
LPD_CARVE_FN double lpd_carve_off(const float* n, const float* a, const float* b)
{
    const double d0 = (double)a[0] - (double)b[0], d1 = (double)a[1] - (double)b[1], d2 = (double)a[2] - (double)b[2];
    return lpd_pgo_dot3((double)n[0], (double)n[1], (double)n[2], d0, d1, d2);
}

// Does the ray o -> w pierce the found cell with the surf row `row`?  erow: the surf row of the endpoint's own cell, NULL when that cell
// is not in the table.  A comparison with a NaN is false, so a NaN centroid never counts.
//   1  the endpoint's row reliable: |n_e . (c - w)| > clearance -- the cell does not lie on the surface the ray ended on;
//   2  the cell's row reliable: g = n_c . (o - c), h = n_c . (w - c), and (g > clearance and h < -clearance) or (g < -clearance and
//      h > clearance) -- the ray crosses the cell's plane and ends well behind it;
//      else: v = w - o, a = c - o, (a.a)(v.v) - (a.v)^2 < (radius radius)(v.v) -- the ray passes within radius of the centroid.
LPD_CARVE_FN int lpd_carve_pierced(const float* o, const float* w, const float* row, const float* erow, float max_flat, double clearance,
                                   double radius)
{
    if (erow && lpd_carve_reliable(erow, max_flat)) {
        if (!(fabs(lpd_carve_off(erow + 3, row, w)) > clearance)) return 0;
    }
    if (lpd_carve_reliable(row, max_flat)) {
        const double g = lpd_carve_off(row + 3, o, row), h = lpd_carve_off(row + 3, w, row);
        return (g > clearance && h < -clearance) || (g < -clearance && h > clearance);
    }
    const double v0 = (double)w[0] - (double)o[0], v1 = (double)w[1] - (double)o[1], v2 = (double)w[2] - (double)o[2];
    const double a0 = (double)row[0] - (double)o[0], a1 = (double)row[1] - (double)o[1], a2 = (double)row[2] - (double)o[2];
    const double aa = lpd_pgo_dot3(a0, a1, a2, a0, a1, a2), vv = lpd_pgo_dot3(v0, v1, v2, v0, v1, v2), av = lpd_pgo_dot3(a0, a1, a2, v0, v1, v2);
    return ((aa * vv) - (av * av)) < ((radius * radius) * vv);
}

// ---- lpd_map_carve / lpd_scan_moving -------------------------------------------------------------------------------------------------------
// a cell of m rows that p rays pierced is MOVING iff it is occupied, pierced often enough, and pierced ratio_q / 1024 times a row:
// p * 1024 >= ratio_q * m in exact integers.  p * 1024 < 2^41, so an m >= 2^42 fails for every ratio_q >= 1 before the product is made:
// ratio_q <= 2^20 times m < 2^42 stays inside an int64.
LPD_CARVE_FN int lpd_carve_moving(int64_t m, int32_t p, int min_pierce, int ratio_q)
{
    if (!(m > 0 && p >= min_pierce)) return 0;
    if (ratio_q == 0) return 1;
    return m < ((int64_t)1 << 42) && (int64_t)p * LPD_CARVE_RATIO_UNITS >= (int64_t)ratio_q * m;
}
