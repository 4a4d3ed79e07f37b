// lpd_tuple_math.h -- the integer and per-point arithmetic of lpd_sample_items / lpd_gather_tuples (csrc/lpd_tuples.hip): the
// Philox4x32-10 counter generator, the uniform drawn from one of its words, the jitter of one point, the permutation perm(j, c,
// seed, row) that turns "the j-th sample" into "the perm-th member of the pool", and the select of the r-th set bit of a word.
// THIS HEADER IS THE DEFINITION of perm (include/lpd_hip.h refers to it); tests/tuples_ref.py restates every function in numpy.
//
// Plain C++, no HIP types: the kernels include it for the device, and a host compiler can include it unchanged (every function is
// a pure function of its arguments).  Compile with -ffp-contract=off, as the library is.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/lpd_hip.h"      // the limits a caller meets: plain C

#if defined(__HIPCC__)
#define LPD_TUPLE_FN __host__ __device__ __forceinline__
#else
#define LPD_TUPLE_FN static inline
#endif

// LPD_TUPLE_MAX_ITEMS, LPD_TUPLE_MAX_SAMPLES, LPD_TUPLE_MAX_LISTS and LPD_TUPLE_MAX_ROWS are the public header's

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), published constants
#define LPD_PHILOX_M0 0xD2511F53u
#define LPD_PHILOX_M1 0xCD9E8D57u
#define LPD_PHILOX_W0 0x9E3779B9u
#define LPD_PHILOX_W1 0xBB67AE85u

struct LpdPhilox4 { uint32_t v[4]; };

LPD_TUPLE_FN LpdPhilox4 lpd_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)LPD_PHILOX_M0 * c0, p1 = (uint64_t)LPD_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += LPD_PHILOX_W0;      // the key is bumped between rounds (the bump after the last round is not used)
        k1 += LPD_PHILOX_W1;
    }
    LpdPhilox4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// u = ((r >> 9) + 0.5) * 2^-23: 23 bits plus the half, exact in fp32, 2^-24 <= u <= 1 - 2^-24 (never 0, never 1)
LPD_TUPLE_FN float lpd_tuple_uniform(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Jitter of point n of the cloud in batch slot b: three Box-Muller normals from ONE Philox block, times sigma, clamped to +-clip
// (the reference's np.clip(sigma * randn(B, N, 3), -clip, clip), loading_pointclouds.py:74-85).
//   (r0..r3) = philox(counter = (n, b, 0, 0), key = (seed_lo, seed_hi)),  u_i = uniform(r_i)
//   z0 = sqrt(-2 ln u0) cos(2 pi u1),  z1 = sqrt(-2 ln u0) sin(2 pi u1),  z2 = sqrt(-2 ln u2) cos(2 pi u3)
LPD_TUPLE_FN void lpd_tuple_jitter(uint32_t n, uint32_t b, uint32_t seed_lo, uint32_t seed_hi, float sigma, float clip, float* d)
{
    const LpdPhilox4 r = lpd_philox4x32_10(n, b, 0u, 0u, seed_lo, seed_hi);
    const float u0 = lpd_tuple_uniform(r.v[0]), u1 = lpd_tuple_uniform(r.v[1]);
    const float u2 = lpd_tuple_uniform(r.v[2]), u3 = lpd_tuple_uniform(r.v[3]);
    const float twopi = 6.28318530717958647692f;
    const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
    const float a = twopi * u1, c = twopi * u3;
    const float z0 = ra * cosf(a), z1 = ra * sinf(a), z2 = rb * cosf(c);
    d[0] = fminf(fmaxf(sigma * z0, -clip), clip);
    d[1] = fminf(fmaxf(sigma * z1, -clip), clip);
    d[2] = fminf(fmaxf(sigma * z2, -clip), clip);
}

// ---- perm(j, c, seed, row): a bijection of [0, c), a pure function of its arguments, 32-bit integer arithmetic only.
//
// c == 1: 0.  Otherwise let h >= 1 be the smallest integer with 4^h >= c (so 4^h < 4 c) and mask = 2^h - 1.  A value x < 4^h is
// the pair (L, R) = (x >> h, x & mask).  Four Feistel rounds i = 0 .. 3,
//     (L, R) <- (R, L ^ (mix(R ^ k_i) & mask)),        x' = (L << h) | R
// are a bijection of [0, 4^h) whatever the round function is; "cycle walking" -- x <- feistel(x) repeated until x < c, starting
// from x = feistel(j) -- restricts it to a bijection of [0, c) (fewer than four trips on average, since c > 4^h / 4; the walk
// cannot run for more than 4^h - c trips: it follows a cycle of a permutation that contains j < c).
//     mix(v)  = the 32-bit finaliser of MurmurHash3: v ^= v >> 16; v *= 0x85EBCA6B; v ^= v >> 13; v *= 0xC2B2AE35; v ^= v >> 16
//     base    = mix(seed_lo ^ mix(seed_hi ^ mix(row ^ 0x9E3779B9)))
//     k_i     = mix(base + (i + 1) * 0x9E3779B9)                                   (all arithmetic modulo 2^32)
LPD_TUPLE_FN uint32_t lpd_tuple_mix(uint32_t v)
{
    v ^= v >> 16;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
}

struct LpdPermKeys { uint32_t k[4]; };

LPD_TUPLE_FN LpdPermKeys lpd_tuple_perm_keys(uint64_t seed, uint32_t row)
{
    const uint32_t base = lpd_tuple_mix((uint32_t)seed ^ lpd_tuple_mix((uint32_t)(seed >> 32) ^ lpd_tuple_mix(row ^ 0x9E3779B9u)));
    LpdPermKeys K;
    for (uint32_t i = 0; i < 4; ++i) K.k[i] = lpd_tuple_mix(base + (i + 1u) * 0x9E3779B9u);
    return K;
}

// h of the definition above, c >= 2 (c <= 2^30: h <= 15)
LPD_TUPLE_FN int lpd_tuple_perm_half_bits(uint32_t c)
{
    int h = 1;
    while (h < 16 && (1u << (2 * h)) < c) ++h;
    return h;
}

LPD_TUPLE_FN uint32_t lpd_tuple_perm_with(uint32_t j, uint32_t c, const LpdPermKeys& K, int h)
{
    if (c <= 1u) return 0u;
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = j;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (int i = 0; i < 4; ++i) {
            const uint32_t t = L ^ (lpd_tuple_mix(R ^ K.k[i]) & mask);
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= c);
    return x;
}

LPD_TUPLE_FN uint32_t lpd_tuple_perm(uint32_t j, uint32_t c, uint64_t seed, uint32_t row)
{
    if (c <= 1u) return 0u;
    return lpd_tuple_perm_with(j, c, lpd_tuple_perm_keys(seed, row), lpd_tuple_perm_half_bits(c));
}

// ---- position of the r-th set bit (r = 0: the lowest) of w; 0 <= r < popcount(w), else 32
LPD_TUPLE_FN uint32_t lpd_tuple_select_bit(uint32_t w, uint32_t r)
{
    if (r >= (uint32_t)__builtin_popcount(w)) return 32u;
    uint32_t pos = 0;
    for (uint32_t width = 16; width > 0; width >>= 1) {
        const uint32_t low = w & ((1u << width) - 1u);
        const uint32_t n = (uint32_t)__builtin_popcount(low);
        if (r >= n) {
            r -= n;
            pos += width;
            w >>= width;
        } else {
            w = low;
        }
    }
    return pos;
}
