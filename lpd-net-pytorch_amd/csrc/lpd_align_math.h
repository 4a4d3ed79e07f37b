// lpd_align_math.h -- the arithmetic of lpd_align_pairs (csrc/lpd_align.hip): which cell of the 128 x 128 x layers occupancy grid a
// point falls into under a yaw hypothesis, the 128-bit row shift, the score of a row pair, the table index of a hypothesis and the
// key that orders the (hypothesis, dy, dx) candidates.  THIS HEADER IS THE DEFINITION of every detail that include/lpd_hip.h leaves
// open; tests/align_ref.py restates every function in numpy, and tests/test_align_cpu.py compares the two value for value.
//
// Plain C++, no HIP types: the kernel includes it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: every product, sum and difference below is ONE
// IEEE operation rounded once -- a fused multiply-add would move points across cell boundaries.  Every comparison is written so that
// a NaN fails it.  No trigonometric function: (cos, sin) come from the caller's table.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_ALIGN_FN __host__ __device__ __forceinline__
#else
#define LPD_ALIGN_FN static inline
#endif

// LPD_ALIGN_GRID and the LPD_ALIGN_MAX_* (LAYERS, S, H, R, POINTS, PAIRS) are the public header's
#define LPD_ALIGN_HALF 64.0f              // the cell of the origin: LPD_ALIGN_GRID / 2
#define LPD_ALIGN_SPAN 33                 // 2 * LPD_ALIGN_MAX_S + 1: the radix of (dy + S, dx + S) in the candidate's number

LPD_ALIGN_FN bool lpd_align_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// entry of the table that hypothesis h of a pair uses: (first + h) mod R, the mathematical (non-negative) remainder
LPD_ALIGN_FN int lpd_align_rot_index(int32_t first, int h, int R)
{
    long long m = ((long long)first + (long long)h) % (long long)R;
    return (int)(m < 0 ? m + R : m);
}

struct LpdAlignCell { int ix, iy, iz; bool valid; };

// What a point contributes whatever the hypothesis is: the scaled planar position and the layer.  ok = the point's own coordinates are
// finite and its layer exists; the kernel keeps (px, py, iz) of a cloud in LDS and turns a point that is not ok into (NaN, NaN, 0),
// which fails lpd_align_plan under every hypothesis.
struct LpdAlignPre { float px, py; int iz; bool ok; };

LPD_ALIGN_FN LpdAlignPre lpd_align_pre(float x, float y, float z, float sc, float z0, float inv_zcell, int layers)
{
    const bool raw = lpd_align_finite(x) && lpd_align_finite(y) && lpd_align_finite(z);
    const float pz = z * sc;
    const float fz = floorf((pz - z0) * inv_zcell);
    LpdAlignPre o;
    o.px = x * sc;
    o.py = y * sc;
    o.ok = raw && fz >= 0.0f && fz < (float)layers;
    o.iz = o.ok ? (int)fz : 0;      // the conversion only after the test: it is undefined for NaN and out-of-range values
    return o;
}

// the planar cell of a metric position (xr, yr): false when it lies outside the grid (or is NaN)
LPD_ALIGN_FN bool lpd_align_plan(float xr, float yr, float inv_cell, int* ix, int* iy)
{
    const float fx = floorf(xr * inv_cell) + LPD_ALIGN_HALF;
    const float fy = floorf(yr * inv_cell) + LPD_ALIGN_HALF;
    const bool in = fx >= 0.0f && fx < 128.0f && fy >= 0.0f && fy < 128.0f;
    *ix = in ? (int)fx : 0;
    *iy = in ? (int)fy : 0;
    return in;
}

// cloud A's planar position under (c, s), with the pre-translation when there is one
LPD_ALIGN_FN bool lpd_align_plan_a(float px, float py, float c, float s, bool has_t0, float t0x, float t0y, float inv_cell, int* ix, int* iy)
{
    float xr = (px * c) - (py * s);
    float yr = (px * s) + (py * c);
    if (has_t0) {
        xr = xr + t0x;
        yr = yr + t0y;
    }
    return lpd_align_plan(xr, yr, inv_cell, ix, iy);
}

// cloud A: scale, rotate by (c, s), add the pre-translation when there is one
LPD_ALIGN_FN LpdAlignCell lpd_align_cell_a(float x, float y, float z, float sc, float c, float s, bool has_t0, float t0x, float t0y,
                                           float inv_cell, float z0, float inv_zcell, int layers)
{
    const LpdAlignPre p = lpd_align_pre(x, y, z, sc, z0, inv_zcell, layers);
    LpdAlignCell o;
    const bool in = lpd_align_plan_a(p.px, p.py, c, s, has_t0, t0x, t0y, inv_cell, &o.ix, &o.iy);
    o.valid = p.ok && in;
    o.ix = o.valid ? o.ix : 0;
    o.iy = o.valid ? o.iy : 0;
    o.iz = o.valid ? p.iz : 0;
    return o;
}

// cloud B: scale only
LPD_ALIGN_FN LpdAlignCell lpd_align_cell_b(float x, float y, float z, float sc, float inv_cell, float z0, float inv_zcell, int layers)
{
    const LpdAlignPre p = lpd_align_pre(x, y, z, sc, z0, inv_zcell, layers);
    LpdAlignCell o;
    const bool in = lpd_align_plan(p.px, p.py, inv_cell, &o.ix, &o.iy);
    o.valid = p.ok && in;
    o.ix = o.valid ? o.ix : 0;
    o.iy = o.valid ? o.iy : 0;
    o.iz = o.valid ? p.iz : 0;
    return o;
}

// out = the row a with bit ix moved to ix + dx, -16 <= dx <= 16; bits that leave [0, 128) are dropped
LPD_ALIGN_FN void lpd_align_shift128(const uint32_t* a, int dx, uint32_t* out)
{
    if (dx > 0) {
        const int r = 32 - dx;      // 16 .. 31
        out[3] = (a[3] << dx) | (a[2] >> r);
        out[2] = (a[2] << dx) | (a[1] >> r);
        out[1] = (a[1] << dx) | (a[0] >> r);
        out[0] = a[0] << dx;
    } else if (dx < 0) {
        const int m = -dx, r = 32 + dx;
        out[0] = (a[0] >> m) | (a[1] << r);
        out[1] = (a[1] >> m) | (a[2] << r);
        out[2] = (a[2] >> m) | (a[3] << r);
        out[3] = a[3] >> m;
    } else {
        out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
    }
}

// popcount(a & b) over a row
LPD_ALIGN_FN int lpd_align_row_score(const uint32_t* a, const uint32_t* b)
{
    return __builtin_popcount(a[0] & b[0]) + __builtin_popcount(a[1] & b[1]) + __builtin_popcount(a[2] & b[2]) + __builtin_popcount(a[3] & b[3]);
}

// The key of the choice: larger score first, then the smaller (h, dy, dx) in lexicographic order, dy and dx counted from -S.  The
// candidate's number is (h * 33 + (dy + S)) * 33 + (dx + S) < 1024 * 1089 < 2^21; nA (the occupied cells of A under h, <= 16384) rides
// in the low bits: it is a function of h, so it never decides.  The maximum over the keys = the winner, in any order.
LPD_ALIGN_FN unsigned long long lpd_align_key(int score, int h, int dyi, int dxi, int nA)
{
    const unsigned long long num = (unsigned long long)((h * LPD_ALIGN_SPAN + dyi) * LPD_ALIGN_SPAN + dxi);
    return ((unsigned long long)score << 36) | ((0x1FFFFFull - num) << 15) | (unsigned long long)nA;
}

// best [8] = (h, dy, dx, score, nA, nB, 1, 0) from the winning key
LPD_ALIGN_FN void lpd_align_unkey(unsigned long long key, int S, int nB, int32_t* best)
{
    const int num = (int)(0x1FFFFFull - ((key >> 15) & 0x1FFFFFull));
    best[0] = num / (LPD_ALIGN_SPAN * LPD_ALIGN_SPAN);
    best[1] = (num / LPD_ALIGN_SPAN) % LPD_ALIGN_SPAN - S;
    best[2] = num % LPD_ALIGN_SPAN - S;
    best[3] = (int)(key >> 36);
    best[4] = (int)(key & 0x7FFFull);
    best[5] = nB;
    best[6] = 1;
    best[7] = 0;
}
