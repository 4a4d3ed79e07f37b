// lpd_map_table.h -- the write side of the voxel hash table that lpd_map.hip (insert, rehash) and lpd_odom.hip (crop) share: one
// (key, sums) into the caller's table by rule 4 of lpd_map_insert (include/lpd_hip.h).  HIP only.
#pragma once
#include "lpd_common.h"
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
