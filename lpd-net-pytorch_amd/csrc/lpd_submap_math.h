// lpd_submap_math.h -- the per-point arithmetic of lpd_make_submaps (csrc/lpd_submap.hip): the ladder of grid resolutions, the
// Morton key of a point on one rung, the integer quantisation behind the cell averages, and the index of a fill row.  The
// definition is in include/lpd_hip.h.
//
// Plain fp32 C++, no HIP types: the kernel includes it for the device, and a host compiler can include it unchanged to run the
// same arithmetic against the numpy restatement without a GPU (every function is a pure function of its arguments).  Compile with
// -ffp-contract=off, as the library is: (x - mn) * s is a subtraction and a multiplication, each rounded once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_SUBMAP_FN __host__ __device__ __forceinline__
#else
#define LPD_SUBMAP_FN static inline
#endif

#define LPD_SUBMAP_RUNGS 128                 // j = 0 .. 127
// LPD_SUBMAP_MIN_N, LPD_SUBMAP_MAX_N and LPD_SUBMAP_MAX_POINTS are the public header's
#define LPD_SUBMAP_QBITS 20                  // u = rint((x - mn) * 2^20 / E)

// 2^(-i/16) rounded to fp32, i = 0 .. 15
LPD_SUBMAP_FN float lpd_submap_literal(int i)
{
    switch (i & 15) {
    case 0: return 1.0f;
    case 1: return 0.957603276f;
    case 2: return 0.917004049f;
    case 3: return 0.878126085f;
    case 4: return 0.840896428f;
    case 5: return 0.805245161f;
    case 6: return 0.771105409f;
    case 7: return 0.738413095f;
    case 8: return 0.707106769f;
    case 9: return 0.677127779f;
    case 10: return 0.648419797f;
    case 11: return 0.620928884f;
    case 12: return 0.594603539f;
    case 13: return 0.56939429f;
    case 14: return 0.545253873f;
    default: return 0.522136867f;
    }
}

// R_j = 1024 * 2^(-j/16) cells per extent: a literal times two exact powers of two (no rounding beyond the literal's own)
LPD_SUBMAP_FN float lpd_submap_resolution(int j)
{
    return ldexpf(lpd_submap_literal(j & 15) * 1024.0f, -((j >> 4) & 7));
}

// s_j = R_j / E: ONE IEEE division per cloud and rung; an extent of 0 (all points equal) puts every point into cell 0
LPD_SUBMAP_FN float lpd_submap_scale(int j, float E) { return E > 0.0f ? lpd_submap_resolution(j) / E : 0.0f; }

// f = 2^20 / E of the quantisation, and the step E * 2^-20 that takes a mean of u back to coordinates
LPD_SUBMAP_FN float lpd_submap_qscale(float E) { return E > 0.0f ? 1048576.0f / E : 0.0f; }
LPD_SUBMAP_FN float lpd_submap_qstep(float E) { return E * 9.5367431640625e-07f; }

LPD_SUBMAP_FN uint32_t lpd_submap_spread10(uint32_t v)
{
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x030000ff;
    v = (v | (v << 8)) & 0x0300f00f;
    v = (v | (v << 4)) & 0x030c30c3;
    v = (v | (v << 2)) & 0x09249249;
    return v;
}

LPD_SUBMAP_FN uint32_t lpd_submap_cell(float x, float mn, float s)
{
    float t = (x - mn) * s;
    t = fminf(fmaxf(t, 0.0f), 1023.0f);
    return (uint32_t)t;
}

// 30-bit Morton key of a point on the rung with scale s: x in bit 0, y in bit 1, z in bit 2 of every triple (lpd_morton.hip's order)
LPD_SUBMAP_FN uint32_t lpd_submap_key(float x, float y, float z, float mnx, float mny, float mnz, float s)
{
    return lpd_submap_spread10(lpd_submap_cell(x, mnx, s)) | (lpd_submap_spread10(lpd_submap_cell(y, mny, s)) << 1) |
           (lpd_submap_spread10(lpd_submap_cell(z, mnz, s)) << 2);
}

// u = rint((x - mn) * f), round half to even; 0 <= u <= 2^20 (+1 at most from the rounding of f)
LPD_SUBMAP_FN uint32_t lpd_submap_quant(float x, float mn, float f) { return (uint32_t)rintf((x - mn) * f); }

// coordinate of a cell row from its integer sum S over m points
LPD_SUBMAP_FN float lpd_submap_centroid(unsigned long long S, int m, float mn, float qstep)
{
    return mn + (float)((double)S / (double)m) * qstep;
}

// raw index of fill row p of `fill` = N - M rows over n raw points: the midpoints of `fill` equal shares of 0 .. n-1
LPD_SUBMAP_FN long long lpd_submap_fill_index(long long p, long long n, long long fill) { return ((2 * p + 1) * n) / (2 * fill); }
