// lpd_odom.hip -- LiDAR odometry on the device: what turns lpd_map_insert and lpd_map_localize, run in turn scan after scan, into
// scan-to-local-map odometry that never waits for the host.  Definition: include/lpd_hip.h; arithmetic: lpd_odom_math.h.
//
//   predict  one thread: the constant-velocity start of scan t from the two poses before it, into pred [t] and pose [t].
//   motion   one thread: the motion of the sensor during scan t under the same model, into motion [t] -- what lpd_scan_deskew
//            (lpd_deskew.hip) takes for that scan (lpd_deskew_math.h).
//   accept   one thread: the decision on scan t after its localisation; a refused scan keeps its prediction and gets a NaN insert pose.
//   (crop    lpd_map_crop is the table-to-table copy of lpd_map.hip with the predicate of lpd_odom_math.h; its entry point is there.)
//   touch    grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, OD_T = 256 threads, the chunk found, checked and staged by the
//            prologue and loader of insert_kernel (lpd_scan_chunk.h: of_call, span_ok, load, poses) and every row made a cell exactly
//            as the insert makes it.  A row is a gather-latency problem of the shape of loc_pass_kernel's: (2 reach + 1)^3 independent
//            probe chains, run by the same lpd_map_find_batch (lpd_map_table.h): all 27 at reach 1, one dz layer of 25 at a time at
//            reach 2.  Every found slot gets dirty = 1: a plain byte store of one value, idempotent and order-free.  keys is only read.
//   refresh  a workgroup per 8192 slots: the flags read sixteen a load, the marked slots gathered in LDS, then one thread a MARKED slot:
//            its surf row by lpd_loc_surface -- the function surface_kernel calls -- and the flag cleared.
// Integer atomics only (the counters); no barrier across workgroups; nothing is read back.  The only
// addresses that come from data are slots masked by capacity - 1 and rows / scans checked against their tables first.
#include <math.h>

#include "lpd_common.h"
#include "lpd_deskew_math.h"
#include "lpd_map_table.h"
#include "lpd_odom_math.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int OD_T = 256;
constexpr int OD_CH = LPD_MAP_CHUNK;
constexpr int OD_R = OD_CH / OD_T;      // rows per thread
constexpr int OD_CAP = 64;              // poses a workgroup keeps in LDS
constexpr int OD_SPAN = 8192;           // slots whose flags one workgroup of the refresh reads
using Chunk = LpdScanChunk<OD_T, OD_CH, OD_CAP>;
typedef unsigned long long u64;

__global__ __launch_bounds__(64) void predict_kernel(double* __restrict__ pose, double* __restrict__ pred, int t,
                                                     const double* __restrict__ first_motion)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double o[12];
    lpd_odom_predict_pose(pose, t, first_motion, o);
    for (int k = 0; k < 12; ++k) pred[(size_t)12 * t + k] = pose[(size_t)12 * t + k] = o[k];
}

__global__ __launch_bounds__(64) void motion_kernel(const double* __restrict__ pose, int t, const double* __restrict__ first_motion,
                                                    double* __restrict__ motion)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double o[12];
    lpd_deskew_odom_motion(pose, t, first_motion, o);
    for (int k = 0; k < 12; ++k) motion[(size_t)12 * t + k] = o[k];
}

__global__ __launch_bounds__(64) void accept_kernel(const double* __restrict__ pred, double* __restrict__ pose, const int32_t* __restrict__ info,
                                                    const int32_t* __restrict__ offsets, int t, int share_q, double max_jump,
                                                    double* __restrict__ insert_pose, int32_t* __restrict__ state)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double p[12], q[12], ins[12];
    for (int k = 0; k < 12; ++k) {
        p[k] = pred[(size_t)12 * t + k];
        q[k] = pose[(size_t)12 * t + k];
    }
    const int32_t in4[4] = {info[4 * (size_t)t], info[4 * (size_t)t + 1], info[4 * (size_t)t + 2], info[4 * (size_t)t + 3]};
    const int64_t len = (int64_t)offsets[t + 1] - (int64_t)offsets[t];
    const int ok = lpd_odom_accept_pose(p, q, in4, len, t, share_q, max_jump, ins);
    for (int k = 0; k < 12; ++k) {
        pose[(size_t)12 * t + k] = q[k];
        insert_pose[(size_t)12 * t + k] = ins[k];
    }
    state[t] = ok;
}

// REACH 1: the 27 chains of a row at once.  REACH 2: one dz layer of 25 at a time.
template <int REACH>
__global__ __launch_bounds__(OD_T) void touch_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                     const double* __restrict__ poses, int scan0, int scan1, const double* __restrict__ origin,
                                                     float inv_cell, const long long* __restrict__ keys, long long capacity,
                                                     unsigned char* __restrict__ dirty)
{
    constexpr int LAYERS = REACH == 1 ? 3 : 1;      // dz layers of one batch: 27 or 25 chains in flight
    __shared__ float buf[3 * OD_CH];
    __shared__ LpdDriveRel rel[OD_CAP];
    __shared__ int32_t soff[OD_CAP + 1];
    __shared__ int span[2];
    const int tid = threadIdx.x;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;                           // uniform
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) return;          // not read: the insert dropped its rows
    Chunk::load(points, ld, g0, cn, buf, tid);
    const int ns = i_hi - i_lo + 1;
    const double org[3] = {origin[0], origin[1], origin[2]};
    const auto pose = [&](int i) { return lpd_map_rel(poses + (size_t)12 * i, org); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, pose);      // i_lo + ns = i_hi + 1 <= scan1
    __syncthreads();
    const int64_t* K = (const int64_t*)keys;
#pragma unroll 1
    for (int k = 0; k < OD_R; ++k) {
        const int j = k * OD_T + tid;
        if (j >= cn) break;
        float w[3];
        int q[3];
        if (!lpd_loc_world(Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, pose), inv_cell, buf[3 * j + 0], buf[3 * j + 1],
                           buf[3 * j + 2], w, q))
            continue;                              // the insert dropped this row
#pragma unroll 1
        for (int z0 = -REACH; z0 <= REACH; z0 += LAYERS)
            lpd_map_find_batch<REACH, LAYERS>(K, capacity, q, z0, [&](int, int64_t at) {
                if (at >= 0) dirty[at] = 1;
            });
    }
}

// A workgroup reads the flags of OD_SPAN slots, sixteen a load, gathers the marked ones in LDS and makes their rows with all lanes busy:
// an insert marks a small share of a large table, and one thread a slot would run a wave for every marked lane.  The order of the list
// depends on timing; a row does not depend on its place in it.
__global__ __launch_bounds__(OD_T) void refresh_kernel(const long long* __restrict__ keys, const long long* __restrict__ acc, long long capacity,
                                                       int reach, int min_cells, float* __restrict__ surf, unsigned char* __restrict__ dirty,
                                                       long long* __restrict__ info)
{
    __shared__ int list[OD_SPAN];
    __shared__ int count;
    __shared__ unsigned made[2];      // rows written with a normal, without one
    const int tid = threadIdx.x;
    if (tid == 0) count = 0;
    if (tid < 2) made[tid] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * OD_SPAN;      // capacity is a power of two >= 16: whole groups of sixteen flags
    for (int v = tid; v < OD_SPAN / 16; v += OD_T) {
        const long long s0 = base + 16 * (long long)v;
        if (s0 >= capacity) break;
        uint4* f = reinterpret_cast<uint4*>(dirty + s0);
        const uint4 w = *f;
        if ((w.x | w.y | w.z | w.w) == 0) continue;
        const unsigned word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if ((word[e >> 2] >> (8 * (e & 3))) & 0xffu) list[atomicAdd(&count, 1)] = 16 * v + e;
        *f = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const int n = count;      // at most OD_SPAN
    for (int e = tid; e < n; e += OD_T) {
        const long long s = base + list[e];
        float row[LPD_LOC_SURF];
        const int r = lpd_loc_surface((const int64_t*)keys, (const int64_t*)acc, capacity, s, reach, min_cells, row);
        float4* o = reinterpret_cast<float4*>(surf + (size_t)LPD_LOC_SURF * s);
        o[0] = make_float4(row[0], row[1], row[2], row[3]);
        o[1] = make_float4(row[4], row[5], row[6], row[7]);
        if (r) atomicAdd(&made[r - 1], 1u);
    }
    __syncthreads();
    if (tid < 2 && made[tid]) atomicAdd((u64*)info + tid, (u64)made[tid]);
}

}  // namespace

extern "C" int lpd_odom_predict(double* pose, double* pred, int S, int t, const double* first_motion, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(pose && pred, "lpd_odom_predict: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_odom_predict: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(t >= 0 && t < S, "lpd_odom_predict: t=%d outside 0 .. S-1=%d", t, S - 1);
    LPD_CHECK_ARG((const void*)pose != (const void*)pred, "lpd_odom_predict: pred must not be pose");
    hipLaunchKernelGGL(predict_kernel, dim3(1), dim3(64), 0, stream, pose, pred, t, first_motion);
    LPD_CHECK_LAUNCH("lpd_odom_predict");
    return LPD_OK;
}

extern "C" int lpd_odom_motion(const double* pose, int S, int t, const double* first_motion, double* motion, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(pose && motion, "lpd_odom_motion: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_odom_motion: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(t >= 0 && t < S, "lpd_odom_motion: t=%d outside 0 .. S-1=%d", t, S - 1);
    LPD_CHECK_ARG((const void*)pose != (const void*)motion, "lpd_odom_motion: motion must not be pose");
    hipLaunchKernelGGL(motion_kernel, dim3(1), dim3(64), 0, stream, pose, t, first_motion, motion);
    LPD_CHECK_LAUNCH("lpd_odom_motion");
    return LPD_OK;
}

extern "C" int lpd_odom_accept(const double* pred, double* pose, const int32_t* info, const int32_t* offsets, int S, int t, int share_q,
                               double max_jump, double* insert_pose, int32_t* state, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(pred && pose && info && offsets && insert_pose && state, "lpd_odom_accept: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_odom_accept: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(t >= 0 && t < S, "lpd_odom_accept: t=%d outside 0 .. S-1=%d", t, S - 1);
    LPD_CHECK_ARG(share_q >= 0 && share_q <= LPD_ODOM_SHARE_UNITS, "lpd_odom_accept: share_q=%d outside 0 .. %d", share_q, LPD_ODOM_SHARE_UNITS);
    LPD_CHECK_ARG(max_jump >= 0.0 && max_jump <= 1.0e6, "lpd_odom_accept: max_jump=%g outside 0 .. 1e6", max_jump);
    hipLaunchKernelGGL(accept_kernel, dim3(1), dim3(64), 0, stream, pred, pose, info, offsets, t, share_q, max_jump, insert_pose, state);
    LPD_CHECK_LAUNCH("lpd_odom_accept");
    return LPD_OK;
}

extern "C" int lpd_map_touch(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                             const double* origin, float inv_cell, const long long* keys, long long capacity, int reach, unsigned char* dirty,
                             void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && origin && keys && dirty, "lpd_map_touch: null pointer");
    LPD_MAP_CHECK_SCANS("lpd_map_touch", ld, rows, S, scan0, scan1, inv_cell, capacity);
    LPD_MAP_CHECK_REACH("lpd_map_touch", reach, 4);
    const dim3 grid((unsigned)(((long long)rows + OD_CH - 1) / OD_CH));
    if (reach == 1)
        hipLaunchKernelGGL(touch_kernel<1>, grid, dim3(OD_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys, capacity,
                           dirty);
    else
        hipLaunchKernelGGL(touch_kernel<2>, grid, dim3(OD_T), 0, stream, points, ld, rows, offsets, poses, scan0, scan1, origin, inv_cell, keys, capacity,
                           dirty);
    LPD_CHECK_LAUNCH("lpd_map_touch");
    return LPD_OK;
}

extern "C" int lpd_map_surface_touched(const long long* keys, const long long* acc, long long capacity, int reach, int min_cells, float* surf,
                                       unsigned char* dirty, long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys && acc && surf && dirty && info, "lpd_map_surface_touched: null pointer");
    LPD_MAP_CHECK_CAPACITY("lpd_map_surface_touched", capacity);
    LPD_MAP_CHECK_REACH("lpd_map_surface_touched", reach, min_cells);
    LPD_CHECK_ARG(((uintptr_t)surf & 15) == 0 && ((uintptr_t)dirty & 15) == 0, "lpd_map_surface_touched: surf and dirty must be 16-byte aligned");
    hipLaunchKernelGGL(refresh_kernel, dim3((unsigned)((capacity + OD_SPAN - 1) / OD_SPAN)), dim3(OD_T), 0, stream, keys, acc, capacity, reach, min_cells,
                       surf, dirty, info);
    LPD_CHECK_LAUNCH("lpd_map_surface_touched");
    return LPD_OK;
}
