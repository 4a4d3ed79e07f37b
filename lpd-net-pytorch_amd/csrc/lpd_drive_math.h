// lpd_drive_math.h -- the arithmetic of lpd_drive_steps / lpd_drive_plan / lpd_drive_rows (csrc/lpd_drive.hip): the quantised step
// between two poses, the three lower bounds that cut a drive into windows, which scan an input row belongs to, the pose of a scan
// relative to its window's reference scan, and the transform of a row.  THIS HEADER IS THE DEFINITION of every detail that
// include/lpd_hip.h leaves open; tests/drive_ref.py restates every function in numpy, and tests/test_drive_cpu.py compares the two
// value for value.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments and of the tables it is handed).  Compile with -ffp-contract=off, as the library is: every product,
// sum and square root below is ONE IEEE operation rounded once.  A pose is twelve doubles, the rows of (R | t): R[r][c] = P[4 r + c],
// t[r] = P[4 r + 3].
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_DRIVE_FN __host__ __device__ __forceinline__
#else
#define LPD_DRIVE_FN static inline
#endif

// LPD_DRIVE_MAX_SCANS, LPD_DRIVE_MAX_WINDOWS, LPD_DRIVE_MAX_WINDOW_NO and LPD_DRIVE_MAX_UNITS are the public header's
#define LPD_DRIVE_MAX_POINTS (1 << 20)       // rows of one window (LPD_SUBMAP_MAX_POINTS)
#define LPD_DRIVE_CHUNK 1024                 // rows of one workgroup
#define LPD_DRIVE_QSCALE 65536.0             // distance units per metre
#define LPD_DRIVE_QMAX 68719476736.0         // 2^36 units = 2^20 m: the largest step

// ((a0*b0) + (a1*b1)) + (a2*b2): the one dot product of the definition
LPD_DRIVE_FN double lpd_drive_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return ((a0 * b0) + (a1 * b1)) + (a2 * b2);
}

// 1. the length of a step in units of 2^-16 m: rint (half to even), clamped to [0, 2^36]; a length that is not finite gives 0
LPD_DRIVE_FN int64_t lpd_drive_quant(double dl)
{
    if (!(fabs(dl) <= 1.7976931348623157e308)) return 0;      // NaN, inf
    const double v = rint(dl * LPD_DRIVE_QSCALE);             // may be inf: clamped
    if (!(v >= 0.0)) return 0;
    return (int64_t)(v > LPD_DRIVE_QMAX ? LPD_DRIVE_QMAX : v);
}

LPD_DRIVE_FN double lpd_drive_step_length(const double* prev, const double* cur)
{
    const double dx = cur[3] - prev[3], dy = cur[7] - prev[7], dz = cur[11] - prev[11];
    return sqrt(lpd_drive_dot3(dx, dy, dz, dx, dy, dz));
}

LPD_DRIVE_FN int64_t lpd_drive_step(const double* prev, const double* cur) { return lpd_drive_quant(lpd_drive_step_length(prev, cur)); }

// the first i in [0, S] with D[i] >= v (S when there is none).  Reads D[0 .. S-1] only, whatever D holds.
LPD_DRIVE_FN int lpd_drive_lower_bound(const int64_t* D, int S, int64_t v)
{
    int lo = 0, hi = S;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (D[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// 3. window w of a drive with the inclusive distances D [S]: scans first .. end-1, the reference scan ref.  An empty window
// (first == end; ref = -1) is what a step longer than L leaves.  A window behind the drive's last one (w*T + L > D[S-1]) is (S, S, -1).
// The clamps on the right only act on a D that does not ascend: first <= ref < end <= S holds for every D.
struct LpdDriveWindow { int first, end, ref; };

LPD_DRIVE_FN LpdDriveWindow lpd_drive_window(const int64_t* D, int S, int64_t L, int64_t T, int64_t w)
{
    const int64_t lo = w * T;
    LpdDriveWindow W;
    if (lo + L > D[S - 1]) {
        W.first = W.end = S;
        W.ref = -1;
        return W;
    }
    W.first = lpd_drive_lower_bound(D, S, lo);
    W.end = lpd_drive_lower_bound(D, S, lo + L);
    if (W.end <= W.first) {
        W.end = W.first;
        W.ref = -1;
        return W;
    }
    const int mid = lpd_drive_lower_bound(D, S, lo + L / 2);
    W.ref = mid < W.end - 1 ? mid : W.end - 1;
    if (W.ref < W.first) W.ref = W.first;
    return W;
}

// the windows of a drive: the w with w*T + L <= D[S-1]
LPD_DRIVE_FN int64_t lpd_drive_window_count(int64_t D_last, int64_t L, int64_t T) { return D_last >= L ? (D_last - L) / T + 1 : 0; }

// The scan of input row g among the scans lo .. hi-1 (offsets[lo] <= g < offsets[hi]): the last i with offsets[i] <= g, so a scan of
// no rows is never the answer.  Reads offsets[lo+1 .. hi-1]; the result lies in [lo, hi-1] whatever they hold.
LPD_DRIVE_FN int lpd_drive_scan_of(const int32_t* offsets, int lo, int hi, int64_t g)
{
    int a = lo + 1, b = hi;
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((int64_t)offsets[mid] > g) b = mid; else a = mid + 1;
    }
    return a - 1;
}

// 5. the pose of scan i relative to the reference scan: row c of M at m[3 c ..], u[c].  frame 1: M = R_ref^T R_i, u = R_ref^T (t_i -
// t_ref); frame 0: M = R_i, u = t_i - t_ref.  Float64, then ONE rounding to fp32.
struct LpdDriveRel { float m[9], u[3]; };

LPD_DRIVE_FN LpdDriveRel lpd_drive_rel(const double* Pi, const double* Pr, int frame)
{
    const double d0 = Pi[3] - Pr[3], d1 = Pi[7] - Pr[7], d2 = Pi[11] - Pr[11];
    LpdDriveRel o;
    if (frame) {
        for (int c = 0; c < 3; ++c) {
            const double a0 = Pr[c], a1 = Pr[4 + c], a2 = Pr[8 + c];      // column c of R_ref
            for (int k = 0; k < 3; ++k) o.m[3 * c + k] = (float)lpd_drive_dot3(a0, a1, a2, Pi[k], Pi[4 + k], Pi[8 + k]);
            o.u[c] = (float)lpd_drive_dot3(a0, a1, a2, d0, d1, d2);
        }
    } else {
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) o.m[3 * c + k] = (float)Pi[4 * c + k];
        o.u[0] = (float)d0;
        o.u[1] = (float)d1;
        o.u[2] = (float)d2;
    }
    return o;
}

// 6. one output coordinate: row c of M, u[c] and the input row, fp32
LPD_DRIVE_FN float lpd_drive_coord(const float* m, float u, float x, float y, float z) { return (((m[0] * x) + (m[1] * y)) + (m[2] * z)) + u; }
