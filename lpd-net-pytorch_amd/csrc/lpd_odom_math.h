// lpd_odom_math.h -- the arithmetic of LiDAR odometry on the device (csrc/lpd_odom.hip): the constant-velocity start of a scan from the
// two poses before it, the decision whether a localised scan is accepted, and which cells of a table a crop keeps.  THIS HEADER IS THE
// DEFINITION of every detail that include/lpd_hip.h leaves open; tests/odom_ref.py restates every function in numpy, and
// tests/test_odometry_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged.  Compile with
// -ffp-contract=off, as the library is: every operation is ONE IEEE operation rounded once.  The relative pose, the composition, the
// renormalisation through the quaternion and the finiteness of a pose are lpd_map_math.h's; the cell of a translation, the inverse of a
// key and the lookup are lpd_map_math.h's and lpd_loc_math.h's.  Nothing of theirs is written out again here.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C
#include "lpd_loc_math.h"
#include "lpd_map_math.h"

#define LPD_ODOM_FN LPD_MAP_FN

// LPD_ODOM_MAX_KEEP_CELLS and LPD_ODOM_SHARE_UNITS are the public header's

// ---- lpd_odom_predict -------------------------------------------------------------------------------------------------------------------
// The start of scan t -> out [12], from the poses [S][12] of the scans before it.
//   t == 0: the pose of scan 0, a bit copy.
//   t == 1: the pose of scan 0, a bit copy; with a first_motion [12] that pose composed with it (lpd_map_compose, no renormalisation).
//   t >= 2: P[t-1] not finite: P[t-1], a bit copy (the scan is invalid for lpd_map_localize);  P[t-2] not finite: P[t-1], a bit copy;
//           else c = lpd_map_candidate(P[t-2], P[t-1], P[t-1]) = P[t-1] (P[t-2]^-1 P[t-1]), its rotation renormalised through the
//           quaternion by lpd_map_blend(c, c, 0.0).
LPD_ODOM_FN void lpd_odom_predict_pose(const double* poses, int t, const double* first_motion, double* out)
{
    if (t <= 1) {
        const double* P0 = poses;
        if (t == 1 && first_motion) {
            const double R[9] = {first_motion[0], first_motion[1], first_motion[2], first_motion[4], first_motion[5],
                                 first_motion[6], first_motion[8], first_motion[9], first_motion[10]};
            const double u[3] = {first_motion[3], first_motion[7], first_motion[11]};
            lpd_map_compose(P0, R, u, out);
            return;
        }
        for (int k = 0; k < 12; ++k) out[k] = P0[k];
        return;
    }
    const double* P1 = poses + (size_t)12 * (t - 1);
    const double* P2 = poses + (size_t)12 * (t - 2);
    if (!lpd_map_finite12(P1) || !lpd_map_finite12(P2)) {
        for (int k = 0; k < 12; ++k) out[k] = P1[k];
        return;
    }
    double c[12];
    lpd_map_candidate(P2, P1, P1, c);
    lpd_map_blend(c, c, 0.0, out);
}

// ---- lpd_odom_accept --------------------------------------------------------------------------------------------------------------------
// Is the localised pose of scan t accepted?  info = the scan's four numbers of lpd_map_localize (valid, steps applied, steps refused,
// correspondences of the last pass), len = its rows, share_q = rint(min_share * 1024) made on the host.
//   t == 0: iff the pose is finite and len > 0 (scan 0 is not localised: there is no map yet).
//   t >= 1: iff info[0] == 1, info[1] >= 1, len > 0, (int64) corr * 1024 >= (int64) share_q * len, and the squared translation between
//           pose and pred -- the three differences, then lpd_pgo_dot3 -- is <= max_jump * max_jump (false for a NaN).
LPD_ODOM_FN int lpd_odom_accepted(const double* pred, const double* pose, const int32_t* info, int64_t len, int t, int share_q, double max_jump)
{
    if (t == 0) return lpd_map_finite12(pose) && len > 0;
    if (!(info[0] == 1 && info[1] >= 1 && len > 0)) return 0;
    if (!((int64_t)info[3] * (int64_t)LPD_ODOM_SHARE_UNITS >= (int64_t)share_q * len)) return 0;
    const double d0 = pose[3] - pred[3], d1 = pose[7] - pred[7], d2 = pose[11] - pred[11];
    return lpd_pgo_dot3(d0, d1, d2, d0, d1, d2) <= max_jump * max_jump;
}

// The whole decision on the three poses of scan t.  Accepted (1): insert = pose.  Otherwise (0): pose = pred bit for bit and insert =
// twelve NaNs, so that lpd_map_insert drops the scan's rows by its own rule 2.
LPD_ODOM_FN int lpd_odom_accept_pose(const double* pred, double* pose, const int32_t* info, int64_t len, int t, int share_q, double max_jump,
                                     double* insert)
{
    const int ok = lpd_odom_accepted(pred, pose, info, len, t, share_q, max_jump);
    for (int k = 0; k < 12; ++k) {
        if (!ok) pose[k] = pred[k];
        insert[k] = ok ? pose[k] : (double)NAN;
    }
    return ok;
}

// ---- lpd_map_crop -----------------------------------------------------------------------------------------------------------------------
// The centre cell of a crop -> qc [3]: the cell of the centre pose's translation by the insert's own rule, u = (float)(t - origin)
// (lpd_map_rel), qc_c = lpd_map_index(u_c, inv_cell).  0 when the pose is not finite or an axis has no cell: every cell is kept then.
LPD_ODOM_FN int lpd_odom_centre_cell(const double* centre, const double* origin, float inv_cell, int* qc)
{
    if (!lpd_map_finite12(centre)) return 0;
    const LpdDriveRel r = lpd_map_rel(centre, origin);
    return lpd_map_index(r.u[0], inv_cell, qc + 0) && lpd_map_index(r.u[1], inv_cell, qc + 1) && lpd_map_index(r.u[2], inv_cell, qc + 2);
}

// Does the cell of `key` go into the new table?  Without a centre every cell does; with one, iff |q_c - qc_c| <= keep_cells on all three
// axes, in integers (both lie in [-2^20, 2^20): the difference cannot overflow).
LPD_ODOM_FN int lpd_odom_keep(int64_t key, int has_centre, const int* qc, int keep_cells)
{
    if (!has_centre) return 1;
    int q[3];
    lpd_loc_unkey(key, q);
    for (int c = 0; c < 3; ++c) {
        const int d = q[c] - qc[c];
        if (d > keep_cells || -d > keep_cells) return 0;
    }
    return 1;
}
