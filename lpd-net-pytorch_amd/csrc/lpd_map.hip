// lpd_map.hip -- the drive map: the nodes' correction of a pose graph carried to every scan, posed scans averaged into one global
// voxel grid kept as a hash table, and the copy of such a table into another.  Definition: include/lpd_hip.h; arithmetic: lpd_map_math.h.
//
//   correct  one thread per scan: a binary search over node_scan, two rigid candidates in float64, their blend.  The only atomics are
//            the two counters (the compiler folds a wave's adds into one).
//   insert   grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, MP_T = 256 threads.  A chunk is loaded as lpd_drive_rows loads it,
//            by the same code (lpd_scan_chunk.h; ld == 3: a flat copy with 16-byte accesses on the aligned body; ld == 4 with an aligned table: one 16-byte load a row), the
//            fp32 poses of its scans are made once per workgroup in float64 (MP_CAP = 64 of them; a chunk of more scans lets every row
//            make its own, the same bits), and every row becomes (key, Ux, Uy, Uz).
//              aggregated form (the default): the rows of the chunk are summed in a table of LPD_MAP_LDS_SLOTS slots in LDS first --
//              consecutive rows of a scan line fall into the same few cells -- with 64-bit LDS integer atomics and the same key; each
//              distinct key of the chunk then goes to the caller's table with ONE compare-and-swap probe sequence and four 64-bit adds.
//              A row that finds no LDS slot in LPD_MAP_LDS_PROBES probes goes straight to the caller's table.
//              direct form (LPD_DEBUG=map-direct): every row straight to the caller's table.
//            Both forms add the same integers to the same keys, so the extracted map is the same.
//   rehash   one thread per slot of an old table: its (key, sums) inserted into a new one (keys are never removed from a table, so a
//   crop     smaller map is a NEW table).  ONE kernel, copy_kernel: the crop (lpd_odom_math.h) is the rehash with a predicate -- only
//            the cells within keep_cells of the centre's cell go over.
// Shared with lpd_odom.hip and lpd_localize.hip: the chunk's prologue and loader (lpd_scan_chunk.h: of_call, span_ok, load, poses), the
// table insert and the entry points' argument checks (lpd_map_table.h), lpd_map_capacity_ok (lpd_map_math.h).
// Integer atomics only: a sum does not depend on the order of its terms.  WHICH slot a key lands in depends on timing; the mapping
// key -> (Sx, Sy, Sz, m) does not.  No barrier across workgroups.  The only address that comes from data is a slot index, masked by
// capacity - 1; every index into offsets, poses and points is checked against its table first.
#include <math.h>

#include "lpd_common.h"
#include "lpd_map_math.h"
#include "lpd_map_table.h"
#include "lpd_odom_math.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int MP_T = 256;
constexpr int MP_CH = LPD_MAP_CHUNK;
constexpr int MP_R = MP_CH / MP_T;      // rows per thread
constexpr int MP_CAP = 64;              // poses a workgroup keeps in LDS
constexpr int MP_LS = LPD_MAP_LDS_SLOTS;
using Chunk = LpdScanChunk<MP_T, MP_CH, MP_CAP>;
typedef unsigned long long u64;

__global__ __launch_bounds__(MP_T) void correct_kernel(const double* __restrict__ poses, const long long* __restrict__ D, int S,
                                                       const int32_t* __restrict__ node_scan, const double* __restrict__ node_pose, int V,
                                                       double* __restrict__ out, int32_t* __restrict__ info)
{
    const int i = blockIdx.x * MP_T + threadIdx.x;
    if (i >= S) return;
    double o[12];
    const int made = lpd_map_correct(poses, (const int64_t*)D, S, node_scan, node_pose, V, i, o);
    for (int k = 0; k < 12; ++k) out[(size_t)12 * i + k] = o[k];
    atomicAdd(info + (made ? 0 : 1), 1);
}

template <bool DIRECT>
__global__ __launch_bounds__(MP_T) void insert_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                      const double* __restrict__ poses, int scan0, int scan1, const double* __restrict__ origin,
                                                      float inv_cell, long long* __restrict__ keys, long long* __restrict__ acc,
                                                      long long capacity, long long* __restrict__ info)
{
    __shared__ float buf[3 * MP_CH];
    __shared__ LpdDriveRel rel[MP_CAP];
    __shared__ int32_t soff[MP_CAP + 1];
    __shared__ int span[2];
    __shared__ u64 cnt[4];                                    // inserted, dropped, lost, created
    __shared__ u64 lkey[DIRECT ? 1 : MP_LS];
    __shared__ u64 lacc[DIRECT ? 4 : 4 * MP_LS];
    const int tid = threadIdx.x;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;      // uniform
    if (tid < 4) cnt[tid] = 0;                                               // the barrier of span_ok publishes these and the LDS table
    if (!DIRECT)
        for (int s = tid; s < MP_LS; s += MP_T) {
            lkey[s] = (u64)LPD_MAP_EMPTY;
            lacc[4 * s + 0] = 0; lacc[4 * s + 1] = 0; lacc[4 * s + 2] = 0; lacc[4 * s + 3] = 0;
        }
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) {      // not read: its rows are counted as dropped
        if (tid == 0) atomicAdd((u64*)info + 1, (u64)cn);
        return;
    }
    Chunk::load(points, ld, g0, cn, buf, tid);
    const int ns = i_hi - i_lo + 1;
    const double org[3] = {origin[0], origin[1], origin[2]};
    const auto pose = [&](int i) { return lpd_map_rel(poses + (size_t)12 * i, org); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, pose);      // i_lo + ns = i_hi + 1 <= scan1
    __syncthreads();
    u64 n_ins = 0, n_drop = 0, n_lost = 0, n_new = 0;
#pragma unroll
    for (int k = 0; k < MP_R; ++k) {
        const int j = k * MP_T + tid;
        if (j < cn) {
            const float x = buf[3 * j + 0], y = buf[3 * j + 1], z = buf[3 * j + 2];
            float w[3];
            int64_t key, U[3];
            if (!lpd_map_row(Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, pose), inv_cell, x, y, z, w, &key, U)) {
                ++n_drop;
                continue;
            }
            bool placed = false;
            if (!DIRECT) {
                unsigned s = (unsigned)(lpd_map_mix(key) >> 32) & (MP_LS - 1);      // the high half: not the bits of the global slot
                for (int p = 0; p < LPD_MAP_LDS_PROBES && !placed; ++p, s = (s + 1) & (MP_LS - 1)) {
                    u64 cur = __hip_atomic_load(&lkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == (u64)LPD_MAP_EMPTY) cur = atomicCAS(&lkey[s], (u64)LPD_MAP_EMPTY, (u64)key);
                    if (cur == (u64)LPD_MAP_EMPTY || cur == (u64)key) {
                        atomicAdd(&lacc[4 * s + 0], (u64)U[0]);
                        atomicAdd(&lacc[4 * s + 1], (u64)U[1]);
                        atomicAdd(&lacc[4 * s + 2], (u64)U[2]);
                        atomicAdd(&lacc[4 * s + 3], (u64)1);
                        placed = true;
                    }
                }
            }
            if (!placed) {
                const int r = lpd_map_table_add(keys, acc, capacity, key, U[0], U[1], U[2], 1);
                if (r) ++n_ins; else ++n_lost;
                if (r == 2) ++n_new;
            }
        }
    }
    if (!DIRECT) {
        __syncthreads();
        for (int s = tid; s < MP_LS; s += MP_T) {
            const u64 key = lkey[s];
            if (key != (u64)LPD_MAP_EMPTY) {
                const u64 m = lacc[4 * s + 3];
                const int r = lpd_map_table_add(keys, acc, capacity, (long long)key, (long long)lacc[4 * s + 0], (long long)lacc[4 * s + 1],
                                                (long long)lacc[4 * s + 2], (long long)m);
                if (r) n_ins += m; else n_lost += m;
                if (r == 2) ++n_new;
            }
        }
    }
    if (n_ins) atomicAdd(&cnt[0], n_ins);
    if (n_drop) atomicAdd(&cnt[1], n_drop);
    if (n_lost) atomicAdd(&cnt[2], n_lost);
    if (n_new) atomicAdd(&cnt[3], n_new);
    __syncthreads();
    if (tid < 4 && cnt[tid]) atomicAdd((u64*)info + tid, cnt[tid]);
}

// Every occupied slot of one table into another, one thread per slot of the old one.  KEEP: only the cells within keep_cells of the
// centre's cell (lpd_odom_keep); without it centre and origin are not read and info [4] is never touched.  One global add a counter
// and workgroup, none for a counter that stayed 0: a cell's count m differs from lane to lane, so the compiler cannot fold a wave's adds.
template <bool KEEP>
__global__ __launch_bounds__(MP_T) void copy_kernel(const long long* __restrict__ keys_in, const long long* __restrict__ acc_in, long long cap_in,
                                                    const double* __restrict__ centre, const double* __restrict__ origin, float inv_cell,
                                                    int keep_cells, long long* __restrict__ keys, long long* __restrict__ acc,
                                                    long long capacity, long long* __restrict__ info)
{
    __shared__ u64 cnt[4];      // rows of the copied cells, rows lost, cells created, cells left behind
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long s = (long long)blockIdx.x * MP_T + threadIdx.x;
    const long long key = s < cap_in ? keys_in[s] : LPD_MAP_EMPTY;
    if (key >= 0) {
        bool keep = true;
        if (KEEP) {
            double c12[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) c12[k] = centre[k];
            const double org[3] = {origin[0], origin[1], origin[2]};
            int qc[3] = {0, 0, 0};
            const int has = lpd_odom_centre_cell(c12, org, inv_cell, qc);
            keep = lpd_odom_keep(key, has, qc, keep_cells);
        }
        if (!keep) {
            atomicAdd(&cnt[3], (u64)1);
        } else {
            const long long m = acc_in[4 * s + 3];
            const int r = lpd_map_table_add(keys, acc, capacity, key, acc_in[4 * s + 0], acc_in[4 * s + 1], acc_in[4 * s + 2], m);
            atomicAdd(&cnt[r ? 0 : 1], (u64)m);
            if (r == 2) atomicAdd(&cnt[2], (u64)1);
        }
    }
    __syncthreads();
    const int to[4] = {0, 2, 3, 4};
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd((u64*)info + to[threadIdx.x], cnt[threadIdx.x]);
}

}  // namespace

extern "C" int lpd_drive_correct(const double* poses, const long long* D, int S, const int32_t* node_scan, const double* node_pose, int V,
                                 double* out, int32_t* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(poses && D && node_scan && node_pose && out && info, "lpd_drive_correct: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_drive_correct: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(V >= 1 && V <= S, "lpd_drive_correct: V=%d outside 1 .. S=%d", V, S);
    LPD_CHECK_ARG((const void*)out != (const void*)poses && (const void*)out != (const void*)node_pose, "lpd_drive_correct: out must not alias its inputs");
    hipLaunchKernelGGL(correct_kernel, dim3((S + MP_T - 1) / MP_T), dim3(MP_T), 0, stream, poses, D, S, node_scan, node_pose, V, out, info);
    LPD_CHECK_LAUNCH("lpd_drive_correct");
    return LPD_OK;
}

extern "C" int lpd_map_insert(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                              const double* origin, float inv_cell, long long* keys, long long* acc, long long capacity, long long* info,
                              void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && origin && keys && acc && info, "lpd_map_insert: null pointer");
    LPD_MAP_CHECK_SCANS("lpd_map_insert", ld, rows, S, scan0, scan1, inv_cell, capacity);
    const dim3 grid((unsigned)(((long long)rows + MP_CH - 1) / MP_CH));
    if (lpd_debug("map-direct", 0))
        hipLaunchKernelGGL(insert_kernel<true>, grid, dim3(MP_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys,
                           acc, capacity, info);
    else
        hipLaunchKernelGGL(insert_kernel<false>, grid, dim3(MP_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys,
                           acc, capacity, info);
    LPD_CHECK_LAUNCH("lpd_map_insert");
    return LPD_OK;
}

extern "C" int lpd_map_rehash(const long long* keys_in, const long long* acc_in, long long capacity_in, long long* keys, long long* acc,
                              long long capacity, long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys_in && acc_in && keys && acc && info, "lpd_map_rehash: null pointer");
    LPD_MAP_CHECK_TWO_TABLES("lpd_map_rehash", keys_in, acc_in, capacity_in, keys, acc, capacity);
    hipLaunchKernelGGL(copy_kernel<false>, dim3((unsigned)((capacity_in + MP_T - 1) / MP_T)), dim3(MP_T), 0, stream, keys_in, acc_in, capacity_in,
                       (const double*)nullptr, (const double*)nullptr, 0.0f, 0, keys, acc, capacity, info);
    LPD_CHECK_LAUNCH("lpd_map_rehash");
    return LPD_OK;
}

extern "C" int lpd_map_crop(const long long* keys_in, const long long* acc_in, long long capacity_in, const double* centre_pose,
                            const double* origin, float inv_cell, int keep_cells, long long* keys, long long* acc, long long capacity,
                            long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys_in && acc_in && centre_pose && origin && keys && acc && info, "lpd_map_crop: null pointer");
    LPD_MAP_CHECK_TWO_TABLES("lpd_map_crop", keys_in, acc_in, capacity_in, keys, acc, capacity);
    LPD_MAP_CHECK_INV_CELL("lpd_map_crop", inv_cell);
    LPD_CHECK_ARG(keep_cells >= 0 && keep_cells <= LPD_ODOM_MAX_KEEP_CELLS, "lpd_map_crop: keep_cells=%d outside 0 .. 2^21", keep_cells);
    hipLaunchKernelGGL(copy_kernel<true>, dim3((unsigned)((capacity_in + MP_T - 1) / MP_T)), dim3(MP_T), 0, stream, keys_in, acc_in, capacity_in,
                       centre_pose, origin, inv_cell, keep_cells, keys, acc, capacity, info);
    LPD_CHECK_LAUNCH("lpd_map_crop");
    return LPD_OK;
}
