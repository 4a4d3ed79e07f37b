// lpd_carve.hip -- moving objects out of the drive map: per occupied cell, the rays of posed scans that pass through its content; the
// table without the cells that enough rays pierced; and the input rows that lie in such a cell.  Definition: include/lpd_hip.h;
// arithmetic: lpd_carve_math.h.
//
//   pierce   grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, CV_T = 256 threads, the chunk found, checked and staged by the
//            prologue and loader of insert_kernel (lpd_scan_chunk.h: of_call, span_ok, load, poses); the record of a scan
//            (LpdCarveScan: transform, sensor position in cells, whether its rays are traversed) is made once per workgroup.  One
//            thread a ray.  The walk is in integers and does not depend on the lookups, so it is taken CV_LOOK = 8 cells ahead: the
//            first probe of each of those cells is loaded before any chain is followed (the shape of lpd_map_find_batch), and the
//            32-byte surf row is loaded only for a cell that is found.  A pierce is one 32-bit integer add on the cell's slot.
//   carve    one thread per slot of the old table: copy_kernel of lpd_map.hip with the predicate lpd_carve_moving.
//   moving   the chunk walk again: every row made a key exactly as the insert makes it, one lookup, one byte a row.
// keys, acc and surf are only read; nothing is inserted into the old table.  Integer atomics only; no barrier across workgroups;
// nothing is read back.  The only addresses that come from data are slots masked by capacity - 1 (or returned by the lookup, which
// masks them) and rows / scans checked against their tables first.  A count belongs to a key: the same bits in every launch, at every
// capacity, under any batching of scans.
#include <math.h>

#include "lpd_common.h"
#include "lpd_carve_math.h"
#include "lpd_map_table.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int CV_T = 256;
constexpr int CV_CH = LPD_MAP_CHUNK;
constexpr int CV_R = CV_CH / CV_T;      // rows per thread
constexpr int CV_CAP = 64;              // scan records a workgroup keeps in LDS
constexpr int CV_LOOK = 8;              // cells of a ray whose first probes are in flight at once
using Chunk = LpdScanChunk<CV_T, CV_CH, CV_CAP>;
typedef unsigned long long u64;

__device__ __forceinline__ void load_row(const float* __restrict__ surf, int64_t s, float* row)
{
    const float4* p = reinterpret_cast<const float4*>(surf + (size_t)LPD_LOC_SURF * s);
    const float4 a = p[0], b = p[1];
    row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w;
    row[4] = b.x; row[5] = b.y; row[6] = b.z; row[7] = b.w;
}

__global__ __launch_bounds__(CV_T) void pierce_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                      const double* __restrict__ poses, int scan0, int scan1, const double* __restrict__ origin,
                                                      float inv_cell, const long long* __restrict__ keys, const float* __restrict__ surf,
                                                      long long capacity, int skip_end, int skip_start, int max_steps, float max_flat,
                                                      double clearance, double radius, int32_t* __restrict__ pierce, long long* __restrict__ info)
{
    __shared__ float buf[3 * CV_CH];
    __shared__ LpdCarveScan rel[CV_CAP];
    __shared__ int32_t soff[CV_CAP + 1];
    __shared__ int span[2];
    __shared__ u64 cnt[6];      // rays, rows dropped, rays cut, cells stepped into, cells found, pierces
    const int tid = threadIdx.x;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;      // uniform
    if (tid < 6) cnt[tid] = 0;                                               // the barrier of span_ok publishes these
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) {      // not read: its rows are counted as dropped
        if (tid == 0) atomicAdd((u64*)info + 1, (u64)cn);
        return;
    }
    Chunk::load(points, ld, g0, cn, buf, tid);
    const int ns = i_hi - i_lo + 1;
    const double org[3] = {origin[0], origin[1], origin[2]};
    const auto scan = [&](int i) { return lpd_carve_scan(poses + (size_t)12 * i, org, inv_cell); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, scan);      // i_lo + ns = i_hi + 1 <= scan1
    __syncthreads();
    const int64_t* K = (const int64_t*)keys;
    u64 n_ray = 0, n_drop = 0, n_cut = 0, n_step = 0, n_found = 0, n_pierce = 0;
#pragma unroll 1
    for (int k = 0; k < CV_R; ++k) {
        const int j = k * CV_T + tid;
        if (j >= cn) break;
        const LpdCarveScan sc = Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, scan);
        float w[3];
        int qa[3];
        if (!sc.ok || !lpd_loc_world(sc.r, inv_cell, buf[3 * j + 0], buf[3 * j + 1], buf[3 * j + 2], w, qa)) {
            ++n_drop;
            continue;
        }
        const float f[3] = {w[0] * inv_cell, w[1] * inv_cell, w[2] * inv_cell};
        LpdCarveRay ray;
        lpd_carve_ray(f, sc.e, &ray);
        ++n_ray;
        n_cut += (u64)lpd_carve_cut(ray.n, max_steps);
        const int visits = (int)lpd_carve_visits(ray.n, max_steps);
        if (visits == 0) continue;
        n_step += (u64)visits;
        float erow[LPD_LOC_SURF];
        const int64_t at_e = lpd_loc_find(K, capacity, lpd_map_key(ray.qa[0], ray.qa[1], ray.qa[2]));      // the endpoint's own cell, once a ray
        if (at_e >= 0) load_row(surf, at_e, erow);
#pragma unroll 1
        for (int v = 0; v < visits; v += CV_LOOK) {
            int64_t key[CV_LOOK], slot[CV_LOOK], first[CV_LOOK];
            bool look[CV_LOOK];
#pragma unroll
            for (int e = 0; e < CV_LOOK; ++e) {
                look[e] = false;
                key[e] = 0;
                slot[e] = 0;
                first[e] = 0;
                if (v + e < visits) {
                    lpd_carve_step(&ray);
                    look[e] = lpd_carve_looked(ray.q, ray.qa, ray.qb, skip_end, skip_start);
                    if (look[e]) {
                        key[e] = lpd_map_key(ray.q[0], ray.q[1], ray.q[2]);      // between two cells of the grid: in range
                        slot[e] = lpd_map_slot(key[e], capacity);
                        first[e] = K[slot[e]];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < CV_LOOK; ++e) {
                if (!look[e]) continue;
                const int64_t at = lpd_loc_find_after(K, capacity, key[e], slot[e], first[e]);
                if (at < 0) continue;
                ++n_found;
                float row[LPD_LOC_SURF];
                load_row(surf, at, row);
                if (lpd_carve_pierced(sc.r.u, w, row, at_e >= 0 ? erow : nullptr, max_flat, clearance, radius)) {
                    atomicAdd(pierce + at, 1);
                    ++n_pierce;
                }
            }
        }
    }
    if (n_ray) atomicAdd(&cnt[0], n_ray);
    if (n_drop) atomicAdd(&cnt[1], n_drop);
    if (n_cut) atomicAdd(&cnt[2], n_cut);
    if (n_step) atomicAdd(&cnt[3], n_step);
    if (n_found) atomicAdd(&cnt[4], n_found);
    if (n_pierce) atomicAdd(&cnt[5], n_pierce);
    __syncthreads();
    if (tid < 6 && cnt[tid]) atomicAdd((u64*)info + tid, cnt[tid]);
}

// copy_kernel of lpd_map.hip with the predicate of lpd_carve_math.h: an occupied slot that is not MOVING goes into the new table
__global__ __launch_bounds__(CV_T) void carve_kernel(const long long* __restrict__ keys_in, const long long* __restrict__ acc_in, long long cap_in,
                                                     const int32_t* __restrict__ pierce, int min_pierce, int ratio_q,
                                                     long long* __restrict__ keys, long long* __restrict__ acc, long long capacity,
                                                     long long* __restrict__ info)
{
    __shared__ u64 cnt[4];      // rows of the copied cells, rows lost, cells created, cells left behind
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long s = (long long)blockIdx.x * CV_T + threadIdx.x;
    const long long key = s < cap_in ? keys_in[s] : LPD_MAP_EMPTY;
    if (key >= 0) {
        const long long m = acc_in[4 * s + 3];
        if (lpd_carve_moving(m, pierce[s], min_pierce, ratio_q)) {
            atomicAdd(&cnt[3], (u64)1);
        } else {
            const int r = lpd_map_table_add(keys, acc, capacity, key, acc_in[4 * s + 0], acc_in[4 * s + 1], acc_in[4 * s + 2], m);
            atomicAdd(&cnt[r ? 0 : 1], (u64)m);
            if (r == 2) atomicAdd(&cnt[2], (u64)1);
        }
    }
    __syncthreads();
    const int to[4] = {0, 2, 3, 4};
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd((u64*)info + to[threadIdx.x], cnt[threadIdx.x]);
}

__global__ __launch_bounds__(CV_T) void moving_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                      const double* __restrict__ poses, int scan0, int scan1, const double* __restrict__ origin,
                                                      float inv_cell, const long long* __restrict__ keys, const long long* __restrict__ acc,
                                                      long long capacity, const int32_t* __restrict__ pierce, int min_pierce, int ratio_q,
                                                      unsigned char* __restrict__ flags, long long* __restrict__ info)
{
    __shared__ float buf[3 * CV_CH];
    __shared__ LpdDriveRel rel[CV_CAP];
    __shared__ int32_t soff[CV_CAP + 1];
    __shared__ int span[2];
    __shared__ unsigned flagged;
    const int tid = threadIdx.x;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;      // uniform; g0 + cn <= rows
    if (tid == 0) flagged = 0;                                               // the barrier of span_ok publishes it
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) {      // not read: the insert dropped its rows
        for (int j = tid; j < cn; j += CV_T) flags[g0 + j] = 0;
        if (tid == 0) atomicAdd((u64*)info + 1, (u64)cn);
        return;
    }
    Chunk::load(points, ld, g0, cn, buf, tid);
    const int ns = i_hi - i_lo + 1;
    const double org[3] = {origin[0], origin[1], origin[2]};
    const auto pose = [&](int i) { return lpd_map_rel(poses + (size_t)12 * i, org); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, pose);      // i_lo + ns = i_hi + 1 <= scan1
    __syncthreads();
    const int64_t* K = (const int64_t*)keys;
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < CV_R; ++k) {
        const int j = k * CV_T + tid;
        if (j < cn) {
            float w[3];
            int64_t key, U[3];
            int f = 0;
            if (lpd_map_row(Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, pose), inv_cell, buf[3 * j + 0], buf[3 * j + 1],
                            buf[3 * j + 2], w, &key, U)) {
                const int64_t at = lpd_loc_find(K, capacity, key);
                if (at >= 0) f = lpd_carve_moving(acc[4 * at + 3], pierce[at], min_pierce, ratio_q);
            }
            flags[g0 + j] = (unsigned char)f;
            mine += (unsigned)f;
        }
    }
    if (mine) atomicAdd(&flagged, mine);
    __syncthreads();
    if (tid == 0) {
        const unsigned n = flagged;
        if (n) atomicAdd((u64*)info + 0, (u64)n);
        if ((unsigned)cn > n) atomicAdd((u64*)info + 1, (u64)((unsigned)cn - n));
    }
}

}  // namespace

extern "C" int lpd_map_pierce(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                              const double* origin, float inv_cell, const long long* keys, const float* surf, long long capacity, int skip_end,
                              int skip_start, int max_steps, float max_flat, double clearance, double radius, int32_t* pierce, long long* info,
                              void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && origin && keys && surf && pierce && info, "lpd_map_pierce: null pointer");
    LPD_MAP_CHECK_SCANS("lpd_map_pierce", ld, rows, S, scan0, scan1, inv_cell, capacity);
    LPD_CHECK_ARG(((uintptr_t)surf & 15) == 0, "lpd_map_pierce: surf must be 16-byte aligned");
    LPD_CHECK_ARG(skip_end >= 0 && skip_end <= LPD_CARVE_MAX_SKIP && skip_start >= 0 && skip_start <= LPD_CARVE_MAX_SKIP,
                  "lpd_map_pierce: skip_end=%d, skip_start=%d outside 0 .. %d", skip_end, skip_start, LPD_CARVE_MAX_SKIP);
    LPD_CHECK_ARG(max_steps >= 1 && max_steps <= LPD_CARVE_MAX_STEPS, "lpd_map_pierce: max_steps=%d outside 1 .. %d", max_steps, LPD_CARVE_MAX_STEPS);
    LPD_CHECK_ARG(max_flat > 0.0f && max_flat <= 1.0f, "lpd_map_pierce: max_flat=%g outside (0, 1]", (double)max_flat);
    LPD_CHECK_ARG(clearance > 0.0 && lpd_icp_finite64(clearance) && radius > 0.0 && lpd_icp_finite64(radius),
                  "lpd_map_pierce: clearance=%g, radius=%g (metres, finite, > 0)", clearance, radius);
    const dim3 grid((unsigned)(((long long)rows + CV_CH - 1) / CV_CH));
    hipLaunchKernelGGL(pierce_kernel, grid, dim3(CV_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys, surf, capacity,
                       skip_end, skip_start, max_steps, max_flat, clearance, radius, pierce, info);
    LPD_CHECK_LAUNCH("lpd_map_pierce");
    return LPD_OK;
}

extern "C" int lpd_map_carve(const long long* keys_in, const long long* acc_in, long long capacity_in, const int32_t* pierce, int min_pierce,
                             int ratio_q, long long* keys, long long* acc, long long capacity, long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys_in && acc_in && pierce && keys && acc && info, "lpd_map_carve: null pointer");
    LPD_MAP_CHECK_TWO_TABLES("lpd_map_carve", keys_in, acc_in, capacity_in, keys, acc, capacity);
    LPD_CHECK_ARG(min_pierce >= 1, "lpd_map_carve: min_pierce=%d (>= 1)", min_pierce);
    LPD_CHECK_ARG(ratio_q >= 0 && ratio_q <= LPD_CARVE_MAX_RATIO_Q, "lpd_map_carve: ratio_q=%d outside 0 .. 2^20", ratio_q);
    hipLaunchKernelGGL(carve_kernel, dim3((unsigned)((capacity_in + CV_T - 1) / CV_T)), dim3(CV_T), 0, stream, keys_in, acc_in, capacity_in, pierce,
                       min_pierce, ratio_q, keys, acc, capacity, info);
    LPD_CHECK_LAUNCH("lpd_map_carve");
    return LPD_OK;
}

extern "C" int lpd_scan_moving(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                               const double* origin, float inv_cell, const long long* keys, const long long* acc, long long capacity,
                               const int32_t* pierce, int min_pierce, int ratio_q, unsigned char* flags, long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && origin && keys && acc && pierce && flags && info, "lpd_scan_moving: null pointer");
    LPD_MAP_CHECK_SCANS("lpd_scan_moving", ld, rows, S, scan0, scan1, inv_cell, capacity);
    LPD_CHECK_ARG(min_pierce >= 1, "lpd_scan_moving: min_pierce=%d (>= 1)", min_pierce);
    LPD_CHECK_ARG(ratio_q >= 0 && ratio_q <= LPD_CARVE_MAX_RATIO_Q, "lpd_scan_moving: ratio_q=%d outside 0 .. 2^20", ratio_q);
    const dim3 grid((unsigned)(((long long)rows + CV_CH - 1) / CV_CH));
    hipLaunchKernelGGL(moving_kernel, grid, dim3(CV_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys, acc, capacity,
                       pierce, min_pierce, ratio_q, flags, info);
    LPD_CHECK_LAUNCH("lpd_scan_moving");
    return LPD_OK;
}
