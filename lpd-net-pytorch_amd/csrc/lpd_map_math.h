// lpd_map_math.h -- the arithmetic of lpd_drive_correct / lpd_map_insert / lpd_map_rehash (csrc/lpd_map.hip): the bracket of a scan among
// the nodes of a pose graph, the two rigid candidates of its corrected pose and their blend, the world row of a point, its cell, the
// cell's key, the fixed-point value that is summed, and the slot a key starts probing at.  THIS HEADER IS THE DEFINITION of every detail
// that include/lpd_hip.h leaves open; tests/map_ref.py restates every function in numpy, and tests/test_map_cpu.py compares the two value
// for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is a pure
// function of its arguments and of the tables it is handed).  Compile with -ffp-contract=off, as the library is: every product, sum,
// difference, quotient and square root below is ONE IEEE operation rounded once.  A pose is twelve doubles, the rows of (R | t).  The
// world row is lpd_drive_rel / lpd_drive_coord of lpd_drive_math.h with frame = 0; the quaternion of a rotation is lpd_pgo_quat of
// lpd_pgo_math.h.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_drive_math.h"
#include "lpd_pgo_math.h"

#define LPD_MAP_FN LPD_DRIVE_FN

// LPD_MAP_QLIM, LPD_MAP_CHUNK, LPD_MAP_MAX_PROBES, LPD_MAP_MIN_CAPACITY and LPD_MAP_MAX_CAPACITY are the public header's
#define LPD_MAP_QLIM_F 1048576.0f            // LPD_MAP_QLIM
#define LPD_MAP_UNITS 65536.0                // fixed-point units per metre, those of the drive step
#define LPD_MAP_LDS_SLOTS 1024               // slots of a workgroup's own table (a power of two)
#define LPD_MAP_LDS_PROBES 8                 // probes there before a row goes straight to the caller's table
#define LPD_MAP_EMPTY (-1LL)                 // the key of an empty slot
// cell = 1 / inv_cell lies in [2^-10, 16] m.  A row that gets a cell has |fl(w * inv_cell)| <= 2^20, so |w| <= 2^20 * 16 * (1 + 2^-24)
// = 2^24 + 1 and |U| = |rint(w * 65536)| < 2^41: the sum of FEWER THAN 2^22 ROWS IN ONE CELL cannot leave an int64 wherever the cell
// lies, and within 32 km of the origin (|w| < 2^15, |U| < 2^31) the same holds for fewer than 2^32 rows in one cell.
#define LPD_MAP_INV_CELL_MIN 0.0625f
#define LPD_MAP_INV_CELL_MAX 1024.0f

// ---- lpd_map_insert ---------------------------------------------------------------------------------------------------------------------
// The pose of a scan for its rows: M = R_i, u = t_i - origin in float64, the twelve numbers rounded to fp32 once -- lpd_drive_rel with
// frame = 0 and t_ref = origin.  The float64 subtraction FIRST is what keeps a UTM northing of 5.7e6 usable: there an fp32 ulp is 0.5 m,
// the difference to an origin on the drive is a few kilometres at most.
LPD_MAP_FN LpdDriveRel lpd_map_rel(const double* Pi, const double* origin)
{
    const double Pr[12] = {0.0, 0.0, 0.0, origin[0], 0.0, 0.0, 0.0, origin[1], 0.0, 0.0, 0.0, origin[2]};
    return lpd_drive_rel(Pi, Pr, 0);
}

// q = (int) floorf(w * inv_cell) when that lies in [-2^20, 2^20); 0 is returned (q untouched) for a NaN, an inf or a cell out of range.
// The comparison is made on the float: no conversion of a value that an int cannot hold.
LPD_MAP_FN int lpd_map_index(float w, float inv_cell, int* q)
{
    const float f = floorf(w * inv_cell);
    if (!(f >= -LPD_MAP_QLIM_F && f < LPD_MAP_QLIM_F)) return 0;
    *q = (int)f;
    return 1;
}

// 63 bits, never -1; ascending key = z-major order of the cells
LPD_MAP_FN int64_t lpd_map_key(int qx, int qy, int qz)
{
    return (int64_t)((uint64_t)(qx + LPD_MAP_QLIM) | ((uint64_t)(qy + LPD_MAP_QLIM) << 21) | ((uint64_t)(qz + LPD_MAP_QLIM) << 42));
}

// the value that is summed: rint (half to even) of the exact product w * 2^16
LPD_MAP_FN int64_t lpd_map_fixed(float w) { return (int64_t)rint((double)w * LPD_MAP_UNITS); }

// the 64-bit mix of a key (the finaliser of splitmix64, arithmetic modulo 2^64); the first slot probed is mix & (capacity - 1), the next
// ones follow with wrap-around
LPD_MAP_FN uint64_t lpd_map_mix(int64_t key)
{
    uint64_t x = (uint64_t)key;
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

LPD_MAP_FN int64_t lpd_map_slot(int64_t key, int64_t capacity) { return (int64_t)(lpd_map_mix(key) & (uint64_t)(capacity - 1)); }

// a table's capacity: a power of two in LPD_MAP_MIN_CAPACITY .. LPD_MAP_MAX_CAPACITY (every entry point's check)
LPD_MAP_FN int lpd_map_capacity_ok(int64_t c) { return c >= LPD_MAP_MIN_CAPACITY && c <= LPD_MAP_MAX_CAPACITY && (c & (c - 1)) == 0; }

// probes of one insert into a table of `capacity` slots
LPD_MAP_FN int lpd_map_probes(int64_t capacity) { return capacity < LPD_MAP_MAX_PROBES ? (int)capacity : LPD_MAP_MAX_PROBES; }

// One row: its world coordinates w [3] (lpd_drive_coord), and -- the return value 1 -- its key and the three values U [3] that are
// summed; 0 for a row that is dropped (a coordinate that is not finite or a cell out of range).
LPD_MAP_FN int lpd_map_row(const LpdDriveRel& r, float inv_cell, float x, float y, float z, float* w, int64_t* key, int64_t* U)
{
    w[0] = lpd_drive_coord(r.m + 0, r.u[0], x, y, z);
    w[1] = lpd_drive_coord(r.m + 3, r.u[1], x, y, z);
    w[2] = lpd_drive_coord(r.m + 6, r.u[2], x, y, z);
    int q[3];
    if (!(lpd_map_index(w[0], inv_cell, q + 0) && lpd_map_index(w[1], inv_cell, q + 1) && lpd_map_index(w[2], inv_cell, q + 2))) return 0;
    *key = lpd_map_key(q[0], q[1], q[2]);
    U[0] = lpd_map_fixed(w[0]);
    U[1] = lpd_map_fixed(w[1]);
    U[2] = lpd_map_fixed(w[2]);
    return 1;
}

// The rows of a call are those of the scans scan0 .. scan1-1: lo = offsets[scan0] .. hi - 1 = offsets[scan1] - 1, and nothing is read
// unless 0 <= lo <= hi <= rows.  They are taken in CHUNKS: chunk c is the rows of [lo, hi) in [1024 c, 1024 c + 1024).  With i_lo / i_hi
// the scans of the chunk's first / last row (lpd_drive_scan_of over scan0 .. scan1), the chunk is READ iff its part of the table is one:
// offsets[i_lo] <= first row, last row < offsets[i_hi + 1], i_lo <= i_hi and offsets[i_lo .. i_hi + 1] does not descend.  The scan of a
// row is then the last i in [i_lo, i_hi] with offsets[i] <= row, which a binary search finds.  The rows of a chunk that is not read are
// counted as dropped.  Whatever the table holds, every index lies in [scan0, scan1] and every row in [lo, hi) within [0, rows).
LPD_MAP_FN int lpd_map_chunk_ok(const int32_t* offsets, int i_lo, int i_hi, int64_t g_first, int64_t g_last)
{
    if (!(i_lo <= i_hi && (int64_t)offsets[i_lo] <= g_first && g_last < (int64_t)offsets[i_hi + 1])) return 0;
    for (int i = i_lo; i <= i_hi; ++i)
        if (offsets[i] > offsets[i + 1]) return 0;
    return 1;
}

// ---- lpd_map extraction (plain torch in lpdnet_hip/mapping.py; restated in tests/map_ref.py) ---------------------------------------------
// One coordinate of a cell's point: (float)(((double)S / (double)m) * 2^-16): two conversions, one division, one exact product, one
// rounding to fp32.
LPD_MAP_FN float lpd_map_mean(int64_t S, int64_t m) { return (float)(((double)S / (double)m) * (1.0 / LPD_MAP_UNITS)); }

// ---- lpd_drive_correct ------------------------------------------------------------------------------------------------------------------
// a = the last node with node_scan[a] <= i, -1 when there is none; b = a + 1 is the first node with node_scan[b] > i (V when there is
// none).  Reads node_scan[0 .. V-1] only; the result lies in [-1, V-1] whatever the table holds.
LPD_MAP_FN int lpd_map_bracket(const int32_t* node_scan, int V, int i)
{
    int lo = 0, hi = V;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (node_scan[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

LPD_MAP_FN bool lpd_map_finite12(const double* P)
{
    bool ok = true;
    for (int a = 0; a < 12; ++a) ok = ok && lpd_icp_finite64(P[a]);
    return ok;
}

// out [12] = the pose X composed with (R [9], t [3]): R' = R_X R, t' = R_X t + t_X (the dot product first, then one addition)
LPD_MAP_FN void lpd_map_compose(const double* X, const double* R, const double* t, double* out)
{
    for (int r = 0; r < 3; ++r) {
        const double x0 = X[4 * r], x1 = X[4 * r + 1], x2 = X[4 * r + 2];
        for (int c = 0; c < 3; ++c) out[4 * r + c] = lpd_pgo_dot3(x0, x1, x2, R[c], R[3 + c], R[6 + c]);
        out[4 * r + 3] = lpd_pgo_dot3(x0, x1, x2, t[0], t[1], t[2]) + X[4 * r + 3];
    }
}

// The candidate of scan i from a node: the node's optimised pose Xn composed with the INPUT pose of the scan relative to the INPUT pose
// Pn of the node's scan, rel = (R_n^T R_i, R_n^T (t_i - t_n)), the difference first (lpd_pgo_between).  The input odometry stays rigid
// around the node.
LPD_MAP_FN void lpd_map_candidate(const double* Pn, const double* Xn, const double* Pi, double* out)
{
    double R[9], t[3];
    lpd_pgo_between(Pn, Pi, R, t);
    lpd_map_compose(Xn, R, t, out);
}

// the blend weight from the distances travelled (units of 2^-16 m): 0 when the two nodes are no distance apart
LPD_MAP_FN double lpd_map_alpha(int64_t Di, int64_t Da, int64_t Db)
{
    const int64_t den = (int64_t)((uint64_t)Db - (uint64_t)Da), num = (int64_t)((uint64_t)Di - (uint64_t)Da);
    return den == 0 ? 0.0 : (double)num / (double)den;
}

// out [12] = the blend of two candidates: t = t_A + alpha (t_B - t_A); the quaternions of both (lpd_pgo_quat), q_B negated when the
// four-term dot product is negative, q = q_A + alpha (q_B - q_A) divided by the square root of its squared norm, and the rotation of q by
// the usual quadratic form.
LPD_MAP_FN void lpd_map_blend(const double* A, const double* B, double alpha, double* out)
{
    double RA[9], RB[9], qa[4], qb[4], q[4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            RA[3 * r + c] = A[4 * r + c];
            RB[3 * r + c] = B[4 * r + c];
        }
    lpd_pgo_quat(RA, qa);
    lpd_pgo_quat(RB, qb);
    const double d = (((qa[0] * qb[0]) + (qa[1] * qb[1])) + (qa[2] * qb[2])) + (qa[3] * qb[3]);
    if (d < 0.0)
        for (int k = 0; k < 4; ++k) qb[k] = -qb[k];
    for (int k = 0; k < 4; ++k) q[k] = qa[k] + (alpha * (qb[k] - qa[k]));
    const double n = sqrt((((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])) + (q[3] * q[3]));
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    out[0] = 1.0 - (2.0 * (yy + zz));
    out[1] = 2.0 * (xy - wz);
    out[2] = 2.0 * (xz + wy);
    out[4] = 2.0 * (xy + wz);
    out[5] = 1.0 - (2.0 * (xx + zz));
    out[6] = 2.0 * (yz - wx);
    out[8] = 2.0 * (xz - wy);
    out[9] = 2.0 * (yz + wx);
    out[10] = 1.0 - (2.0 * (xx + yy));
    for (int r = 0; r < 3; ++r) out[4 * r + 3] = A[4 * r + 3] + (alpha * (B[4 * r + 3] - A[4 * r + 3]));
}

// The corrected pose of scan i -> out [12]; returns 1 when it was made from the nodes, 0 when the scan's input pose was passed through
// as a bit copy.  In this order:
//   the bracket a, b = a + 1;  sa = node_scan[a] (a >= 0), sb = node_scan[b] (b < V);
//   pass through when the table is not one here (not 0 <= sa <= i, not i < sb < S) or the scan's input pose is not finite;
//   i == sa: the copy of node_pose[a] when that is finite, else pass through;
//   pass through when an input pose of a bracket scan or an optimised pose of a bracket node is not finite;
//   one candidate (before the first node, behind the last): that candidate; two: their blend with lpd_map_alpha.
// Nothing outside [0, S) of poses and D and [0, V) of the nodes is read, whatever node_scan holds.
LPD_MAP_FN int lpd_map_correct(const double* poses, const int64_t* D, int S, const int32_t* node_scan, const double* node_pose, int V, int i,
                               double* out)
{
    const double* Pi = poses + (size_t)12 * i;
    const int a = lpd_map_bracket(node_scan, V, i), b = a + 1;
    const bool ha = a >= 0, hb = b < V;
    const int sa = ha ? node_scan[a] : 0, sb = hb ? node_scan[b] : 0;
    bool ok = (!ha || (sa >= 0 && sa <= i)) && (!hb || (sb > i && sb < S)) && (ha || hb) && lpd_map_finite12(Pi);
    if (ok && ha && sa == i) {
        const double* X = node_pose + (size_t)12 * a;
        if (lpd_map_finite12(X)) {
            for (int k = 0; k < 12; ++k) out[k] = X[k];
            return 1;
        }
        ok = false;
    }
    if (ok && ha) ok = lpd_map_finite12(poses + (size_t)12 * sa) && lpd_map_finite12(node_pose + (size_t)12 * a);
    if (ok && hb) ok = lpd_map_finite12(poses + (size_t)12 * sb) && lpd_map_finite12(node_pose + (size_t)12 * b);
    if (!ok) {
        for (int k = 0; k < 12; ++k) out[k] = Pi[k];
        return 0;
    }
    double A[12], B[12];
    if (ha) lpd_map_candidate(poses + (size_t)12 * sa, node_pose + (size_t)12 * a, Pi, A);
    if (hb) lpd_map_candidate(poses + (size_t)12 * sb, node_pose + (size_t)12 * b, Pi, B);
    if (ha && hb) {
        lpd_map_blend(A, B, lpd_map_alpha(D[i], D[sa], D[sb]), out);
    } else {
        const double* C = ha ? A : B;
        for (int k = 0; k < 12; ++k) out[k] = C[k];
    }
    return 1;
}
