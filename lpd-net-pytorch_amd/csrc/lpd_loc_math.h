// lpd_loc_math.h -- the arithmetic of lpd_map_surface / lpd_map_localize (csrc/lpd_localize.hip): the read side of the voxel hash table
// (the lookup of a key, the neighbour of a cell, the centroid / normal / flatness row of a slot) and the trimmed point-to-plane ICP of a
// posed scan against it (the validity of a scan, its centre, the correspondence of a world row among the 27 cells around it, the centred
// row, the centred step).  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves open; tests/loc_ref.py restates
// every function in numpy, and tests/test_localize_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged.  Compile with
// -ffp-contract=off, as the library is: every operation is ONE IEEE operation rounded once, in fp32 or float64 as written.  The world row,
// the cell, the key, the first slot, the probe count and the mean of a cell are lpd_map_math.h's; the moments are lpd_feat_math.h's; the
// normal, the distance, the decisions, the quantised row, its 29 terms, the LDL^T and the pose update are lpd_icp_math.h's.  Nothing of
// theirs is written out again here.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_icp_math.h"
#include "lpd_map_math.h"

#define LPD_LOC_FN LPD_MAP_FN

// LPD_LOC_MAX_ITERS, LPD_LOC_MAX_SCAN_ROWS and LPD_LOC_SURF are the public header's
#define LPD_LOC_KEY_MASK 0x1FFFFFLL      // 21 bits an axis

// ---- the read side of a table --------------------------------------------------------------------------------------------------------------
// The lookup with its first load already made: `first` = keys[s0], s0 = lpd_map_slot(key, capacity).  -> the slot that holds the key, or
// -1: the first empty slot, or lpd_map_probes(capacity) probes without the key.  A kernel issues the first loads of many keys before it
// follows any chain; the answer is that of lpd_loc_find.
LPD_LOC_FN int64_t lpd_loc_find_after(const int64_t* keys, int64_t capacity, int64_t key, int64_t s0, int64_t first)
{
    const uint64_t mask = (uint64_t)capacity - 1;
    const int probes = lpd_map_probes(capacity);
    uint64_t s = (uint64_t)s0;
    int64_t cur = first;
    for (int p = 1;; ++p) {
        if (cur == key) return (int64_t)s;
        if (cur == LPD_MAP_EMPTY || p >= probes) return -1;
        s = (s + 1) & mask;
        cur = keys[s];
    }
}

LPD_LOC_FN int64_t lpd_loc_find(const int64_t* keys, int64_t capacity, int64_t key)
{
    const int64_t s0 = lpd_map_slot(key, capacity);
    return lpd_loc_find_after(keys, capacity, key, s0, keys[s0]);
}

// the cell of a key (the inverse of lpd_map_key)
LPD_LOC_FN void lpd_loc_unkey(int64_t key, int* q)
{
    q[0] = (int)(key & LPD_LOC_KEY_MASK) - LPD_MAP_QLIM;
    q[1] = (int)((key >> 21) & LPD_LOC_KEY_MASK) - LPD_MAP_QLIM;
    q[2] = (int)((key >> 42) & LPD_LOC_KEY_MASK) - LPD_MAP_QLIM;
}

// the key of the cell q + (dx, dy, dz); 0 (key untouched) when an index leaves [-2^20, 2^20): that cell is absent without a lookup
LPD_LOC_FN int lpd_loc_neighbour(const int* q, int dx, int dy, int dz, int64_t* key)
{
    const int x = q[0] + dx, y = q[1] + dy, z = q[2] + dz;
    if (x < -LPD_MAP_QLIM || x >= LPD_MAP_QLIM || y < -LPD_MAP_QLIM || y >= LPD_MAP_QLIM || z < -LPD_MAP_QLIM || z >= LPD_MAP_QLIM) return 0;
    *key = lpd_map_key(x, y, z);
    return 1;
}

// the centroid of slot s -> c [3]; 0 when the slot's count is not positive (such a slot is absent)
LPD_LOC_FN int lpd_loc_centroid(const int64_t* acc, int64_t s, float* c)
{
    const int64_t m = acc[4 * s + 3];
    if (m <= 0) return 0;
    c[0] = lpd_map_mean(acc[4 * s + 0], m);
    c[1] = lpd_map_mean(acc[4 * s + 1], m);
    c[2] = lpd_map_mean(acc[4 * s + 2], m);
    return 1;
}

// The surf row of slot s -> row [LPD_LOC_SURF] = (cx, cy, cz, nx, ny, nz, flatness, cells used); returns 0 for an empty slot (the row is
// all zeros), 1 for a row with a normal, 2 for a row without one.  The (2 reach + 1)^3 cells around the slot's own are visited in
// ascending dz, dy, dx -- ascending key order, the cell itself among them; d = c_j - c in fp32 of every present one goes into
// lpd_feat_add, k counts them; k < min_cells: no normal and flatness 0, else lpd_icp_normal(moments, k).  An OCCUPIED slot whose count is
// not positive (no insert makes one) gets (NaN, NaN, NaN, 0, 0, 0, 0, 0): its distance to anything is NaN, which never wins a search, so
// the pass treats it as absent from its first 16 bytes alone.
LPD_LOC_FN int lpd_loc_surface(const int64_t* keys, const int64_t* acc, int64_t capacity, int64_t s, int reach, int min_cells, float* row)
{
    for (int e = 0; e < LPD_LOC_SURF; ++e) row[e] = 0.0f;
    const int64_t key = keys[s];
    if (key < 0) return 0;
    float c[3];
    if (!lpd_loc_centroid(acc, s, c)) {
        row[0] = row[1] = row[2] = NAN;
        return 2;
    }
    int q[3];
    lpd_loc_unkey(key, q);
    LpdFeatMoments m;
    lpd_feat_init(m);
    int k = 0;
    for (int dz = -reach; dz <= reach; ++dz)
        for (int dy = -reach; dy <= reach; ++dy)
            for (int dx = -reach; dx <= reach; ++dx) {
                int64_t nk;
                if (!lpd_loc_neighbour(q, dx, dy, dz, &nk)) continue;
                const int64_t t = lpd_loc_find(keys, capacity, nk);
                float cj[3];
                if (t < 0 || !lpd_loc_centroid(acc, t, cj)) continue;
                lpd_feat_add(m, cj[0] - c[0], cj[1] - c[1], cj[2] - c[2]);
                ++k;
            }
    row[0] = c[0];
    row[1] = c[1];
    row[2] = c[2];
    row[7] = (float)k;
    if (k < min_cells) return 2;
    lpd_icp_normal(m, k, row + 3, row + 6);
    return lpd_icp_normal_zero(row[3], row[4], row[5]) ? 2 : 1;
}

// ---- one scan ----------------------------------------------------------------------------------------------------------------------------
// A scan is valid iff its pose is finite, 0 <= offsets[i] <= offsets[i+1] <= rows and it has at most 2^20 rows (2^20 terms of at most
// 2^40 stay inside an int64).
LPD_LOC_FN int lpd_loc_scan_valid(const double* pose, int64_t o0, int64_t o1, int64_t rows)
{
    return lpd_map_finite12(pose) && o0 >= 0 && o0 <= o1 && o1 <= rows && o1 - o0 <= (int64_t)LPD_LOC_MAX_SCAN_ROWS;
}

// The centre of a scan, fixed once at entry: g = t_in - origin in float64, g32 = g rounded to fp32.  Residuals are formed around it.
LPD_LOC_FN void lpd_loc_centre(const double* pose, const double* origin, double* g, float* g32)
{
    for (int c = 0; c < 3; ++c) {
        g[c] = pose[4 * c + 3] - origin[c];
        g32[c] = (float)g[c];
    }
}

// The world row of a point (the insert's, bit for bit) and its cell.  0: the row has no cell, hence no correspondence.
LPD_LOC_FN int lpd_loc_world(const LpdDriveRel& r, float inv_cell, float x, float y, float z, float* w, int* q)
{
    w[0] = lpd_drive_coord(r.m + 0, r.u[0], x, y, z);
    w[1] = lpd_drive_coord(r.m + 3, r.u[1], x, y, z);
    w[2] = lpd_drive_coord(r.m + 6, r.u[2], x, y, z);
    return lpd_map_index(w[0], inv_cell, q + 0) && lpd_map_index(w[1], inv_cell, q + 1) && lpd_map_index(w[2], inv_cell, q + 2);
}

// p = w - g32, one fp32 subtraction a coordinate.  0: a |p_c| beyond 512 m -- no correspondence.
LPD_LOC_FN int lpd_loc_centred(const float* w, const float* g32, float* p)
{
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        p[c] = w[c] - g32[c];
        ok = ok && fabsf(p[c]) <= LPD_ICP_RANGE;
    }
    return ok;
}

// The nearest centroid among the 27 cells around q, visited in ascending dz, dy, dx (ascending key): a later cell wins only when
// strictly nearer, a distance that is not finite never wins.  -> the winner's slot (-1: none) and its squared distance.  This is the
// plain form; the pass kernel loads the 27 first probes before it follows a chain and finds the same winner.
LPD_LOC_FN int64_t lpd_loc_nearest(const int64_t* keys, const float* surf, int64_t capacity, const int* q, const float* w, float* best)
{
    int64_t at = -1;
    *best = INFINITY;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                int64_t nk;
                if (!lpd_loc_neighbour(q, dx, dy, dz, &nk)) continue;
                const int64_t t = lpd_loc_find(keys, capacity, nk);
                if (t < 0) continue;
                const float* c = surf + LPD_LOC_SURF * t;
                const float d2 = lpd_icp_d2(c[0], c[1], c[2], w[0], w[1], w[2]);
                if (lpd_icp_nearer(d2, *best)) {
                    *best = d2;
                    at = t;
                }
            }
    return at;
}

// Is the winner (its surf row, its squared distance) the correspondence?  Within dmax, a normal, flat enough.
LPD_LOC_FN int lpd_loc_accept(const float* row, float d2, float dmax, float max_flat)
{
    return lpd_icp_within(d2, dmax) && !lpd_icp_normal_zero(row[3], row[4], row[5]) && row[6] <= max_flat;
}

// What a correspondence adds to the sums: p the centred row, the winner's surf row; q = c - g32, then lpd_icp_row and lpd_icp_terms.
LPD_LOC_FN void lpd_loc_terms(const float* p, const float* row, const float* g32, int64_t* t)
{
    const float q[3] = {row[0] - g32[0], row[1] - g32[1], row[2] - g32[2]};
    int64_t Ji[6], ri;
    lpd_icp_row(p, q, row + 3, Ji, &ri);
    lpd_icp_terms(Ji, ri, t);
}

// One step from a pass's sums, the rotation taken about the centre: lpd_icp_solve's sequence on (R | T), T = (t - origin) - g, then
// t = (T' + g) + origin.  Returns 1 and updates the pose, or 0 under lpd_icp_solve's conditions and leaves it bit for bit as it is.
LPD_LOC_FN int lpd_loc_step(const int64_t* sums, int min_inliers, const double* origin, const double* g, double* pose)
{
    if (sums[LPD_ICP_SUM_M] < (int64_t)min_inliers) return 0;
    double x[6], np[12];
    if (!lpd_icp_ldl(sums, x)) return 0;
    for (int i = 0; i < 6; ++i)
        if (!lpd_icp_finite64(x[i])) return 0;
    for (int i = 0; i < 12; ++i) np[i] = pose[i];
    for (int c = 0; c < 3; ++c) np[4 * c + 3] = (pose[4 * c + 3] - origin[c]) - g[c];
    lpd_icp_update(x, np);
    for (int c = 0; c < 3; ++c) np[4 * c + 3] = (np[4 * c + 3] + g[c]) + origin[c];
    for (int i = 0; i < 12; ++i)
        if (!lpd_icp_finite64(np[i])) return 0;
    for (int i = 0; i < 12; ++i) pose[i] = np[i];
    return 1;
}
