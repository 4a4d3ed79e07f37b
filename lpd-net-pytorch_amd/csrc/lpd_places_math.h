// lpd_places_math.h -- the membership predicate of lpd_radius_count / lpd_radius_fill (csrc/lpd_places.hip): is a database position
// within r of a query position?  THIS HEADER IS THE DEFINITION (include/lpd_hip.h refers to it); tests/places_ref.py restates it in
// numpy, and tests/test_places_cpu.py compares the two decision for decision.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is a
// pure function of its arguments).  Compile with -ffp-contract=off, as the library is: the two products and the sum below are three
// IEEE float64 operations, each rounded once -- a fused multiply-add would move memberships on the boundary.
#pragma once
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_PLACES_FN __host__ __device__ __forceinline__
#else
#define LPD_PLACES_FN static inline
#endif

// LPD_PLACES_MAX_ITEMS, LPD_PLACES_MAX_SEGMENTS and LPD_PLACES_CHUNK are the public header's
#define LPD_PLACES_WAVE_QUERIES 4           // query rows a wave carries
#define LPD_PLACES_BLOCK_QUERIES 16         // ... and a 256-thread workgroup: four waves

// the right-hand side of the comparison: ONE product
LPD_PLACES_FN double lpd_place_radius_sq(double r) { return r * r; }

// (qx - px)^2 + (qy - py)^2 <= r2.  A NaN on either side compares false: never a member.  An infinite coordinate gives inf or
// inf - inf = NaN on the left: never a member of a finite radius either.  (a - b)^2 == (b - a)^2 exactly (a - b and b - a differ in
// sign only), so membership is symmetric in the two positions.
LPD_PLACES_FN bool lpd_place_within(double qx, double qy, double px, double py, double r2)
{
    const double dx = qx - px, dy = qy - py;
    return (dx * dx) + (dy * dy) <= r2;
}
