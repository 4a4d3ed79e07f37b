// lpd_localize.hip -- the read side of the voxel hash table and the localisation of posed scans against it: lpd_map_surface makes one
// (centroid, normal, flatness, cells used) row per slot, lpd_map_localize runs a trimmed point-to-plane ICP of whole scans against those
// rows.  Definition: include/lpd_hip.h; arithmetic: lpd_loc_math.h.
//
//   surface  one thread per slot: the (2 reach + 1)^3 lookups around the slot's cell, the centred moments of the present centroids, the
//            three-row Jacobi of lpd_icp_math.h.  The only place that divides in float64 (lpd_map_mean) and the only reader of acc.
//   init     one thread per scan: its validity, info = (1 | -1, 0, 0, 0), and into ws its fp32 world pose (lpd_map_rel), its centre g
//            (float64) and g32.
//   pass     THE HOT PATH.  grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, LC_T = 256 threads, the chunk found, checked and
//            staged by the prologue and loader of insert_kernel (lpd_scan_chunk.h: of_call, span_ok, load, poses); the fp32 poses,
//            centres and validity of its scans come from ws into LDS (LC_CAP = 64 of them; a chunk of more scans reads ws per row --
//            the same bits).  A row is a gather-latency problem: 27 independent probe chains.  The FIRST probe of all 27 cells is
//            loaded before any is compared (lpd_map_find_batch of lpd_map_table.h, which touch_kernel of lpd_odom.hip runs as well),
//            then the first 16 bytes of the found slots' surf rows (the centroid) feed the running minimum, and the winner's second 16
//            bytes (normal, flatness) decide the correspondence.  acc is never touched and nothing is divided.  The table was written by
//            earlier launches: plain loads.
//            The 29 integer terms: a thread sums its rows while they belong to one scan; when all rows of a wave do, the wave sums by
//            butterfly and sends ONE 64-bit atomic a sum to sums [scan]; otherwise the thread's terms go to the chunk's per-scan LDS
//            sums (or, in a chunk of more than 64 scans, straight to the global ones).  All roads add the same integers.
//   step     one thread per scan: lpd_loc_step in float64 on the pass's sums, pose and info in place, the next pass's fp32 pose into ws.
//            Behind the last pass it only writes info [3].
// iters + 1 pass launches, iters + 1 step launches, one init and one memset; nothing synchronises.  Integer atomics only.  The only
// addresses that come from data are slots masked by capacity - 1 and rows / scans checked against their tables first.
#include <math.h>

#include "lpd_common.h"
#include "lpd_loc_math.h"
#include "lpd_map_table.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int LC_T = 256;
constexpr int LC_CH = LPD_MAP_CHUNK;
constexpr int LC_R = LC_CH / LC_T;      // rows per thread
constexpr int LC_CAP = 64;              // scans a workgroup keeps in LDS
using Chunk = LpdScanChunk<LC_T, LC_CH, LC_CAP>;
typedef unsigned long long u64;

struct LcState { float m[9], u[3], g32[3]; int32_t valid; double g[3], pad; };      // ws [S]: 96 bytes a scan
static_assert(sizeof(LcState) == 96, "the workspace is 96 bytes a scan");

__global__ __launch_bounds__(LC_T) void surface_kernel(const long long* __restrict__ keys, const long long* __restrict__ acc, long long capacity,
                                                       int reach, int min_cells, float* __restrict__ surf, long long* __restrict__ info)
{
    const long long s = (long long)blockIdx.x * LC_T + threadIdx.x;
    int r = 0;
    if (s < capacity) {
        float row[LPD_LOC_SURF];
        r = lpd_loc_surface((const int64_t*)keys, (const int64_t*)acc, capacity, s, reach, min_cells, row);
        float4* o = reinterpret_cast<float4*>(surf + (size_t)LPD_LOC_SURF * s);
        o[0] = make_float4(row[0], row[1], row[2], row[3]);
        o[1] = make_float4(row[4], row[5], row[6], row[7]);
    }
    const int with = __syncthreads_count(r == 1), without = __syncthreads_count(r == 2);
    if (threadIdx.x == 0 && with) atomicAdd((u64*)info, (u64)with);
    if (threadIdx.x == 0 && without) atomicAdd((u64*)info + 1, (u64)without);
}

__device__ __forceinline__ void lc_store_rel(LcState* __restrict__ st, const double* pose, const double* origin)
{
    const LpdDriveRel r = lpd_map_rel(pose, origin);
#pragma unroll
    for (int e = 0; e < 9; ++e) st->m[e] = r.m[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) st->u[e] = r.u[e];
}

__global__ __launch_bounds__(LC_T) void loc_init_kernel(const int32_t* __restrict__ offsets, int rows, int scan0, int scan1,
                                                        const double* __restrict__ origin, const double* __restrict__ pose,
                                                        int32_t* __restrict__ info, LcState* __restrict__ ws)
{
    const int i = scan0 + blockIdx.x * LC_T + threadIdx.x;
    if (i >= scan1) return;
    double P12[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P12[e] = pose[12 * (size_t)i + e];
    const double org[3] = {origin[0], origin[1], origin[2]};
    const bool ok = lpd_loc_scan_valid(P12, offsets[i], offsets[i + 1], rows);
    info[4 * (size_t)i] = ok ? 1 : -1;
    info[4 * (size_t)i + 1] = info[4 * (size_t)i + 2] = info[4 * (size_t)i + 3] = 0;
    LcState st;
#pragma unroll
    for (int e = 0; e < 9; ++e) st.m[e] = 0.0f;
#pragma unroll
    for (int e = 0; e < 3; ++e) st.u[e] = st.g32[e] = 0.0f, st.g[e] = 0.0;
    st.pad = 0.0;
    st.valid = ok ? 1 : 0;
    if (ok) {
        lc_store_rel(&st, P12, org);
        lpd_loc_centre(P12, org, st.g, st.g32);
    }
    ws[i] = st;
}

__device__ __forceinline__ long long lc_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(LC_T) void loc_pass_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                        int scan0, int scan1, float inv_cell, const long long* __restrict__ keys,
                                                        const float* __restrict__ surf, long long capacity, const LcState* __restrict__ ws,
                                                        float dmax, float max_flat, long long* __restrict__ sums, long long* __restrict__ cell)
{
    __shared__ float buf[3 * LC_CH];
    __shared__ LpdDriveRel rel[LC_CAP];
    __shared__ int32_t soff[LC_CAP + 1];
    __shared__ int span[2];
    __shared__ float sg[LC_CAP][3];
    __shared__ int sval[LC_CAP];
    __shared__ u64 lsum[LC_CAP * LPD_ICP_SUMS];
    const int tid = threadIdx.x, lane = tid & 63;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;                      // uniform
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) {           // not read: its rows have no correspondence
        if (cell)
            for (int j = tid; j < cn; j += LC_T) cell[g0 + j] = -1;
        return;
    }
    const int ns = i_hi - i_lo + 1;
    const auto pose = [&](int i) {
        LpdDriveRel r;
#pragma unroll
        for (int e = 0; e < 9; ++e) r.m[e] = ws[i].m[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) r.u[e] = ws[i].u[e];
        return r;
    };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, pose);      // i_lo + ns = i_hi + 1 <= scan1
    int guard = !table;
    if (table) {
        if (tid < ns) {
            const LcState* st = ws + i_lo + tid;
            sg[tid][0] = st->g32[0]; sg[tid][1] = st->g32[1]; sg[tid][2] = st->g32[2];
            sval[tid] = st->valid;
            guard = !st->valid;
        }
        for (int e = tid; e < ns * LPD_ICP_SUMS; e += LC_T) lsum[e] = 0;
    }
    // The rows of an invalid scan are never read: a chunk that holds one (or more than 64 scans) loads row by row, behind the scan's flag
    const bool guarded = __syncthreads_or(guard);
    const auto scan_of = [&](long long g) { return table ? lpd_drive_scan_of(soff, 0, ns, g) : lpd_drive_scan_of(offsets, i_lo, i_lo + ns, g) - i_lo; };
    const auto valid_of = [&](int li) { return table ? sval[li] : ws[i_lo + li].valid; };
    if (!guarded) {
        Chunk::load(points, ld, g0, cn, buf, tid);
    } else {
        for (int j = tid; j < cn; j += LC_T)
            if (valid_of(scan_of(g0 + j))) {
                const float* p = points + (size_t)(g0 + j) * ld;
                buf[3 * j + 0] = p[0]; buf[3 * j + 1] = p[1]; buf[3 * j + 2] = p[2];
            }
    }
    __syncthreads();
    const int64_t* K = (const int64_t*)keys;
    long long t[29];
#pragma unroll
    for (int e = 0; e < 29; ++e) t[e] = 0;
    int tscan = -1;      // the scan (within the chunk) whose terms t holds
    const auto add_slow = [&](int li) {
#pragma unroll
        for (int e = 0; e < 29; ++e)
            if (t[e] != 0) {
                if (table) atomicAdd(&lsum[li * LPD_ICP_SUMS + e], (u64)t[e]);
                else atomicAdd((u64*)sums + (size_t)(i_lo + li) * LPD_ICP_SUMS + e, (u64)t[e]);
            }
    };
#pragma unroll 1
    for (int k = 0; k < LC_R; ++k) {
        const int j = k * LC_T + tid;
        if (j >= cn) break;
        const long long g = g0 + j;
        const int li = scan_of(g);
        long long out = -1;
        if (valid_of(li)) {
            LpdDriveRel r;
            float g32[3];
            if (table) {
                r = rel[li];
                g32[0] = sg[li][0]; g32[1] = sg[li][1]; g32[2] = sg[li][2];
            } else {
                r = pose(i_lo + li);
                g32[0] = ws[i_lo + li].g32[0]; g32[1] = ws[i_lo + li].g32[1]; g32[2] = ws[i_lo + li].g32[2];
            }
            float w[3], p[3];
            int q[3];
            if (lpd_loc_world(r, inv_cell, buf[3 * j + 0], buf[3 * j + 1], buf[3 * j + 2], w, q) && lpd_loc_centred(w, g32, p)) {
                // the slots of the 27 cells, or -1: the first probe of all 27 chains before any is compared
                int64_t slot[27];
                lpd_map_find_batch<1, 3>(K, capacity, q, -1, [&](int e, int64_t at) { slot[e] = at; });
                // the centroids of the present cells, the running minimum in ascending key order
                float best = INFINITY;
                int64_t at = -1;
                float4 ca = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int e = 0; e < 27; ++e)
                    if (slot[e] >= 0) {
                        const float4 a = *reinterpret_cast<const float4*>(surf + (size_t)LPD_LOC_SURF * slot[e]);
                        const float d2 = lpd_icp_d2(a.x, a.y, a.z, w[0], w[1], w[2]);
                        if (lpd_icp_nearer(d2, best)) {
                            best = d2;
                            at = slot[e];
                            ca = a;
                        }
                    }
                if (at >= 0) {
                    const float4 b = *reinterpret_cast<const float4*>(surf + (size_t)LPD_LOC_SURF * at + 4);
                    const float row[LPD_LOC_SURF] = {ca.x, ca.y, ca.z, ca.w, b.x, b.y, b.z, b.w};
                    if (lpd_loc_accept(row, best, dmax, max_flat)) {
                        int64_t tt[LPD_ICP_SUMS];
                        lpd_loc_terms(p, row, g32, tt);
                        if (tscan >= 0 && tscan != li) {      // the thread's rows changed scan: what it holds goes the slow road
                            add_slow(tscan);
#pragma unroll
                            for (int e = 0; e < 29; ++e) t[e] = 0;
                        }
                        tscan = li;
#pragma unroll
                        for (int e = 0; e < 29; ++e) t[e] += (long long)tt[e];
                        out = K[at];
                    }
                }
            }
        }
        if (cell) cell[g] = out;
    }
    const u64 act = __ballot(tscan >= 0);
    if (act) {      // uniform over the wave
        const int one = __shfl(tscan, __ffsll((long long)act) - 1, 64);
        if (__ballot(tscan >= 0 && tscan != one) == 0ull) {
            long long mine = 0;      // lane e keeps sum e: the butterfly leaves the total in every lane
#pragma unroll
            for (int e = 0; e < 29; ++e) {
                const long long s = lc_wave_sum(t[e]);
                mine = lane == e ? s : mine;
            }
            if (lane < 29 && mine != 0) atomicAdd((u64*)sums + (size_t)(i_lo + one) * LPD_ICP_SUMS + lane, (u64)mine);
        } else if (tscan >= 0) {
            add_slow(tscan);
        }
    }
    if (table) {      // uniform over the workgroup
        __syncthreads();
        for (int e = tid; e < ns * LPD_ICP_SUMS; e += LC_T) {
            const u64 v = lsum[e];
            if (v != 0) atomicAdd((u64*)sums + (size_t)i_lo * LPD_ICP_SUMS + e, v);
        }
    }
}

__global__ __launch_bounds__(LC_T) void loc_step_kernel(int scan0, int scan1, int step, int min_inliers, const double* __restrict__ origin,
                                                        const long long* __restrict__ sums, double* __restrict__ pose, int32_t* __restrict__ info,
                                                        LcState* __restrict__ ws)
{
    const int i = scan0 + blockIdx.x * LC_T + threadIdx.x;
    if (i >= scan1 || !ws[i].valid) return;
    int64_t s[LPD_ICP_SUMS];
#pragma unroll
    for (int e = 0; e < 29; ++e) s[e] = (int64_t)sums[(size_t)i * LPD_ICP_SUMS + e];
    int32_t* o = info + 4 * (size_t)i;
    if (!step) {
        o[3] = (int32_t)s[LPD_ICP_SUM_M];
        return;
    }
    double P12[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P12[e] = pose[12 * (size_t)i + e];
    const double org[3] = {origin[0], origin[1], origin[2]}, g[3] = {ws[i].g[0], ws[i].g[1], ws[i].g[2]};
    if (lpd_loc_step(s, min_inliers, org, g, P12)) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[12 * (size_t)i + e] = P12[e];
        lc_store_rel(ws + i, P12, org);
        o[1] += 1;
    } else {
        o[2] += 1;
    }
}

}  // namespace

extern "C" int lpd_map_surface(const long long* keys, const long long* acc, long long capacity, int reach, int min_cells, float* surf,
                               long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys && acc && surf && info, "lpd_map_surface: null pointer");
    LPD_MAP_CHECK_CAPACITY("lpd_map_surface", capacity);
    LPD_MAP_CHECK_REACH("lpd_map_surface", reach, min_cells);
    LPD_CHECK_ARG(((uintptr_t)surf & 15) == 0, "lpd_map_surface: surf must be 16-byte aligned");
    hipLaunchKernelGGL(surface_kernel, dim3((unsigned)((capacity + LC_T - 1) / LC_T)), dim3(LC_T), 0, stream, keys, acc, capacity, reach, min_cells,
                       surf, info);
    LPD_CHECK_LAUNCH("lpd_map_surface");
    return LPD_OK;
}

extern "C" long long lpd_map_localize_workspace_bytes(int S, int iters)
{
    return S >= 1 && S <= LPD_DRIVE_MAX_SCANS && iters >= 0 && iters <= LPD_LOC_MAX_ITERS ? (long long)S * (long long)sizeof(LcState) : 0;
}

extern "C" int lpd_map_localize(const float* points, int ld, int rows, const int32_t* offsets, int S, int scan0, int scan1, const double* origin,
                                float inv_cell, const long long* keys, const float* surf, long long capacity, const float* dmax, int iters,
                                int min_inliers, float max_flat, double* pose, int32_t* info, long long* sums, long long* cell, void* ws,
                                void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && origin && keys && surf && dmax && pose && info && sums, "lpd_map_localize: null pointer");
    LPD_MAP_CHECK_SCANS("lpd_map_localize", ld, rows, S, scan0, scan1, inv_cell, capacity);
    LPD_CHECK_ARG(iters >= 0 && iters <= LPD_LOC_MAX_ITERS, "lpd_map_localize: iters=%d outside 0 .. %d", iters, LPD_LOC_MAX_ITERS);
    LPD_CHECK_ARG(min_inliers >= LPD_ICP_MIN_INLIERS, "lpd_map_localize: min_inliers=%d below %d", min_inliers, LPD_ICP_MIN_INLIERS);
    LPD_CHECK_ARG(max_flat > 0.0f && max_flat <= 1.0f, "lpd_map_localize: max_flat=%g outside (0, 1]", (double)max_flat);
    for (int s = 0; s <= iters; ++s)
        LPD_CHECK_ARG(lpd_icp_finite(dmax[s]) && dmax[s] > 0.0f && dmax[s] <= LPD_ICP_MAX_DMAX, "lpd_map_localize: dmax[%d]=%g (finite, > 0, <= %g)", s,
                      (double)dmax[s], (double)LPD_ICP_MAX_DMAX);
    LPD_CHECK_ARG(((uintptr_t)surf & 15) == 0, "lpd_map_localize: surf must be 16-byte aligned");
    LPD_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "lpd_map_localize: the workspace (lpd_map_localize_workspace_bytes, 16-byte aligned) is missing");
    const size_t per_pass = (size_t)S * LPD_ICP_SUMS;
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)(iters + 1) * per_pass * sizeof(long long), stream);
    if (e != hipSuccess) {
        lpd_set_error("lpd_map_localize: clearing the sums failed: %s", hipGetErrorString(e));
        return LPD_ERR_LAUNCH;
    }
    const unsigned sblocks = (unsigned)((scan1 - scan0 + LC_T - 1) / LC_T);
    const dim3 grid((unsigned)(((long long)rows + LC_CH - 1) / LC_CH));
    LcState* st = (LcState*)ws;
    hipLaunchKernelGGL(loc_init_kernel, dim3(sblocks), dim3(LC_T), 0, stream, offsets, rows, scan0, scan1, origin, (const double*)pose, info, st);
    for (int s = 0; s <= iters; ++s) {
        long long* ss = sums + (size_t)s * per_pass;
        hipLaunchKernelGGL(loc_pass_kernel, grid, dim3(LC_T), 0, stream, points, ld, rows, offsets, scan0, scan1, inv_cell, keys, surf, capacity,
                           (const LcState*)st, dmax[s], max_flat, ss, s == iters ? cell : (long long*)nullptr);
        hipLaunchKernelGGL(loc_step_kernel, dim3(sblocks), dim3(LC_T), 0, stream, scan0, scan1, s < iters ? 1 : 0, min_inliers, origin,
                           (const long long*)ss, pose, info, st);
    }
    LPD_CHECK_LAUNCH("lpd_map_localize");
    return LPD_OK;
}
