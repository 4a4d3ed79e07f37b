// lpd_map_table.h -- what lpd_map.hip, lpd_odom.hip and lpd_localize.hip share around the voxel hash table.  HIP only.
//   write side   lpd_map_table_add: one (key, sums) into a table by rule 4 of lpd_map_insert (include/lpd_hip.h) -- insert, rehash, crop.
//   read side    lpd_map_find_batch: the probe chains of a batch of cells around one cell -- touch_kernel and loc_pass_kernel.
//   host side    LPD_MAP_CHECK_*: the argument checks that the three files' entry points have in common, each naming its caller
//                (lpd_map_capacity_ok is lpd_map_math.h's, where a host compiler sees it).
#pragma once
#include "lpd_common.h"
#include "lpd_loc_math.h"
#include "lpd_map_math.h"

// (key, sums) into the caller's table: 0 lost, 1 added to a cell that was there, 2 added to a cell this call created.  keys never
// change once set, so a key that is read is final, and a slot that reads empty is settled by the compare-and-swap.
__device__ __forceinline__ int lpd_map_table_add(long long* __restrict__ keys, long long* __restrict__ acc, long long capacity, long long key,
                                                 long long sx, long long sy, long long sz, long long m)
{
    typedef unsigned long long u64;
    const u64 mask = (u64)capacity - 1;
    u64 s = lpd_map_mix(key) & mask;
    const int probes = lpd_map_probes(capacity);
    for (int p = 0; p < probes; ++p, s = (s + 1) & mask) {
        long long cur = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int created = 0;
        if (cur == LPD_MAP_EMPTY) {
            cur = (long long)atomicCAS((u64*)(keys + s), (u64)LPD_MAP_EMPTY, (u64)key);
            if (cur == LPD_MAP_EMPTY) {
                cur = key;
                created = 1;
            }
        }
        if (cur == key) {
            u64* a = (u64*)(acc + 4 * s);
            atomicAdd(a + 0, (u64)sx);
            atomicAdd(a + 1, (u64)sy);
            atomicAdd(a + 2, (u64)sz);
            atomicAdd(a + 3, (u64)m);
            return 1 + created;
        }
    }
    return 0;
}

// The B = LAYERS W^2 chains (W = 2 REACH + 1) of the cells q + (dx, dy, dz), |dx|, |dy| <= REACH, dz = z0 .. z0 + LAYERS - 1, in
// ascending (dz, dy, dx): all 27 at reach 1 (LAYERS = 3, z0 = -1), one dz layer of 25 at reach 2 (125 at once would not fit the
// registers).  A row is a gather-latency problem: the first probe of EVERY chain is loaded before any is compared; then each chain
// runs to its end (lpd_loc_find_after) and found(e, at) gets chain e's slot, or -1 for a cell that is absent or out of range.
template <int REACH, int LAYERS, class F>
__device__ __forceinline__ void lpd_map_find_batch(const int64_t* __restrict__ K, long long capacity, const int* q, int z0, F&& found)
{
    constexpr int W = 2 * REACH + 1, B = LAYERS * W * W;
    int64_t first[B], slot[B];
#pragma unroll
    for (int e = 0; e < B; ++e) {
        int64_t nk = 0;
        const int in = lpd_loc_neighbour(q, e % W - REACH, (e / W) % W - REACH, z0 + e / (W * W), &nk);
        slot[e] = in ? lpd_map_slot(nk, capacity) : 0;
        first[e] = K[slot[e]];
    }
#pragma unroll
    for (int e = 0; e < B; ++e) {
        int64_t nk = 0;
        const int in = lpd_loc_neighbour(q, e % W - REACH, (e / W) % W - REACH, z0 + e / (W * W), &nk);
        found(e, in ? lpd_loc_find_after(K, capacity, nk, slot[e], first[e]) : (int64_t)-1);
    }
}

// ---- the host side: `fn` is the entry point's name, a string literal ----------------------------------------------------------------------
#define LPD_MAP_CHECK_CAPACITY(fn, capacity) \
    LPD_CHECK_ARG(lpd_map_capacity_ok(capacity), fn ": capacity=%lld is not a power of two in 16 .. 2^36", (long long)(capacity))
#define LPD_MAP_CHECK_INV_CELL(fn, inv_cell)                                                \
    LPD_CHECK_ARG((inv_cell) >= LPD_MAP_INV_CELL_MIN && (inv_cell) <= LPD_MAP_INV_CELL_MAX, \
                  fn ": inv_cell=%g outside 1/16 .. 1024 (a cell of 2^-10 .. 16 m keeps every sum inside an int64)", (double)(inv_cell))
// the head of a call on the posed-scan table and a hash table: points [rows, ld], offsets [S + 1], the scans scan0 .. scan1-1
#define LPD_MAP_CHECK_SCANS(fn, ld, rows, S, scan0, scan1, inv_cell, capacity)                                                        \
    do {                                                                                                                              \
        LPD_CHECK_ARG((ld) >= 3 && (rows) >= 1, fn ": bad dims ld=%d rows=%d (ld >= 3, rows >= 1)", ld, rows);                        \
        LPD_CHECK_ARG((S) >= 1 && (S) <= LPD_DRIVE_MAX_SCANS, fn ": S=%d outside 1 .. 2^22", S);                                      \
        LPD_CHECK_ARG((scan0) >= 0 && (scan0) < (scan1) && (scan1) <= (S), fn ": scans %d .. %d outside 0 .. S=%d", scan0, scan1, S); \
        LPD_MAP_CHECK_INV_CELL(fn, inv_cell);                                                                                         \
        LPD_MAP_CHECK_CAPACITY(fn, capacity);                                                                                         \
    } while (0)
// reach and min_cells (4, the least, from a caller that makes no surf rows)
#define LPD_MAP_CHECK_REACH(fn, reach, min_cells)                                                                                   \
    do {                                                                                                                            \
        LPD_CHECK_ARG((reach) == 1 || (reach) == 2, fn ": reach=%d (1 or 2)", reach);                                               \
        const int cells_ = (2 * (reach) + 1) * (2 * (reach) + 1) * (2 * (reach) + 1);                                               \
        LPD_CHECK_ARG((min_cells) >= 4 && (min_cells) <= cells_, fn ": min_cells=%d outside 4 .. %d", min_cells, cells_);           \
    } while (0)
#define LPD_MAP_CHECK_TWO_TABLES(fn, keys_in, acc_in, capacity_in, keys, acc, capacity)                                                     \
    do {                                                                                                                                    \
        LPD_CHECK_ARG(lpd_map_capacity_ok(capacity_in) && lpd_map_capacity_ok(capacity),                                                    \
                      fn ": capacities %lld -> %lld are not powers of two in 16 .. 2^36", (long long)(capacity_in), (long long)(capacity)); \
        LPD_CHECK_ARG((const void*)(keys_in) != (const void*)(keys) && (const void*)(acc_in) != (const void*)(acc),                         \
                      fn ": the new table must not be the old one");                                                                        \
    } while (0)
