// lpd_odom.hip -- LiDAR odometry on the device: what turns lpd_map_insert and lpd_map_localize, run in turn scan after scan, into
// scan-to-local-map odometry that never waits for the host.  Definition: include/lpd_hip.h; arithmetic: lpd_odom_math.h.
//
//   predict  one thread: the constant-velocity start of scan t from the two poses before it, into pred [t] and pose [t].
//   accept   one thread: the decision on scan t after its localisation; a refused scan keeps its prediction and gets a NaN insert pose.
//   crop     one thread per slot of an old table: lpd_map_rehash with a predicate -- the cells within keep_cells of the centre's cell go
//            into the new table by the shared lpd_map_table_add (keys are never removed from a table, so a smaller map is a NEW table).
//   touch    grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, OD_T = 256 threads, the chunk staged by the loader of insert_kernel
//            (lpd_scan_chunk.h) and every row made a cell exactly as the insert makes it.  A row is a gather-latency problem of the
//            shape of loc_pass_kernel's: (2 reach + 1)^3 independent probe chains.  The first probe of a batch of chains (all 27 at
//            reach 1, one dz layer of 25 at reach 2: 125 at once would not fit the registers) is loaded before any is compared; then
//            each chain runs to its end (lpd_loc_find_after) and every found slot gets dirty = 1: a plain byte store of one value,
//            idempotent and order-free.  keys is only read.
//   refresh  a workgroup per 8192 slots: the flags read sixteen a load, the marked slots gathered in LDS, then one thread a MARKED slot:
//            its surf row by lpd_loc_surface -- the function surface_kernel calls -- and the flag cleared.
// Integer atomics only (the counters, and the shared table insert); no barrier across workgroups; nothing is read back.  The only
// addresses that come from data are slots masked by capacity - 1 and rows / scans checked against their tables first.
#include <math.h>

#include "lpd_common.h"
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

__global__ __launch_bounds__(OD_T) void crop_kernel(const long long* __restrict__ keys_in, const long long* __restrict__ acc_in, long long cap_in,
                                                    const double* __restrict__ centre, const double* __restrict__ origin, float inv_cell,
                                                    int keep_cells, long long* __restrict__ keys, long long* __restrict__ acc,
                                                    long long capacity, long long* __restrict__ info)
{
    __shared__ u64 cnt[4];      // rows of the kept cells, rows lost, cells created, cells left behind
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long s = (long long)blockIdx.x * OD_T + threadIdx.x;
    const long long key = s < cap_in ? keys_in[s] : LPD_MAP_EMPTY;
    if (key >= 0) {
        double c12[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) c12[k] = centre[k];
        const double org[3] = {origin[0], origin[1], origin[2]};
        int qc[3] = {0, 0, 0};
        const int has = lpd_odom_centre_cell(c12, org, inv_cell, qc);
        if (!lpd_odom_keep(key, has, qc, keep_cells)) {
            atomicAdd(&cnt[3], (u64)1);
        } else {
            const long long m = acc_in[4 * s + 3];
            const int r = lpd_map_table_add(keys, acc, capacity, key, acc_in[4 * s + 0], acc_in[4 * s + 1], acc_in[4 * s + 2], m);
            atomicAdd(&cnt[r ? 0 : 1], (u64)m);
            if (r == 2) atomicAdd(&cnt[2], (u64)1);
        }
    }
    // one global add a counter and workgroup: a cell's count m differs from lane to lane, so the compiler cannot fold a wave's adds
    __syncthreads();
    const int to[4] = {0, 2, 3, 4};
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd((u64*)info + to[threadIdx.x], cnt[threadIdx.x]);
}

// REACH 1: the 27 chains of a row at once.  REACH 2: one dz layer of 25 at a time.
template <int REACH>
__global__ __launch_bounds__(OD_T) void touch_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                     const double* __restrict__ poses, int scan0, int scan1, const double* __restrict__ origin,
                                                     float inv_cell, const long long* __restrict__ keys, long long capacity,
                                                     unsigned char* __restrict__ dirty)
{
    constexpr int W = 2 * REACH + 1;
    constexpr int LAYERS = REACH == 1 ? W : 1;      // dz layers of one batch
    constexpr int B = LAYERS * W * W;               // chains in flight: 27 or 25
    __shared__ float buf[3 * OD_CH];
    __shared__ LpdDriveRel rel[OD_CAP];
    __shared__ int32_t soff[OD_CAP + 1];
    __shared__ int span[2];
    const int tid = threadIdx.x;
    const long long lo = offsets[scan0], hi = offsets[scan1];      // 0 <= scan0 < scan1 <= S: the host's check
    if (!(lo >= 0 && lo <= hi && hi <= rows)) return;              // uniform: nothing is read
    const long long c0 = (long long)blockIdx.x * OD_CH;
    const long long g0 = c0 > lo ? c0 : lo, g1 = c0 + OD_CH < hi ? c0 + OD_CH : hi;
    if (g0 >= g1) return;                                          // uniform
    const int cn = (int)(g1 - g0);                                 // 1 .. 1024 rows, all in [lo, hi) within [0, rows)
    Chunk::find_span(offsets, scan0, scan1, g0, cn, span, tid);
    __syncthreads();
    const int i_lo = span[0], i_hi = span[1];      // both in [scan0, scan1 - 1]
    int bad = !(i_lo <= i_hi && (long long)offsets[i_lo] <= g0 && g1 - 1 < (long long)offsets[i_hi + 1]);      // lpd_map_chunk_ok
    if (!bad)
        for (int i = i_lo + tid; i <= i_hi; i += OD_T) bad |= offsets[i] > offsets[i + 1];
    if (__syncthreads_or(bad)) return;             // not read: the insert dropped its rows
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
        for (int z0 = -REACH; z0 <= REACH; z0 += LAYERS) {
            // the first probe of the batch's chains, before any is compared
            int64_t first[B], slot[B];
#pragma unroll
            for (int e = 0; e < B; ++e) {
                int64_t nk = 0;
                const int in = lpd_loc_neighbour(q, e % W - REACH, (e / W) % W - REACH, z0 + e / (W * W), &nk);
                slot[e] = in ? lpd_map_slot(nk, capacity) : 0;
                first[e] = K[slot[e]];
            }
            // each chain to its end: the slot of the cell, or -1
#pragma unroll
            for (int e = 0; e < B; ++e) {
                int64_t nk = 0;
                const int in = lpd_loc_neighbour(q, e % W - REACH, (e / W) % W - REACH, z0 + e / (W * W), &nk);
                const int64_t at = in ? lpd_loc_find_after(K, capacity, nk, slot[e], first[e]) : -1;
                if (at >= 0) dirty[at] = 1;
            }
        }
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

bool od_capacity_ok(long long c) { return c >= LPD_MAP_MIN_CAPACITY && c <= LPD_MAP_MAX_CAPACITY && (c & (c - 1)) == 0; }

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

extern "C" int lpd_map_crop(const long long* keys_in, const long long* acc_in, long long capacity_in, const double* centre_pose,
                            const double* origin, float inv_cell, int keep_cells, long long* keys, long long* acc, long long capacity,
                            long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(keys_in && acc_in && centre_pose && origin && keys && acc && info, "lpd_map_crop: null pointer");
    LPD_CHECK_ARG(od_capacity_ok(capacity_in) && od_capacity_ok(capacity), "lpd_map_crop: capacities %lld -> %lld are not powers of two in 16 .. 2^36",
                  capacity_in, capacity);
    LPD_CHECK_ARG((const void*)keys_in != (const void*)keys && (const void*)acc_in != (const void*)acc, "lpd_map_crop: the new table must not be the old one");
    LPD_CHECK_ARG(inv_cell >= LPD_MAP_INV_CELL_MIN && inv_cell <= LPD_MAP_INV_CELL_MAX, "lpd_map_crop: inv_cell=%g outside 1/16 .. 1024",
                  (double)inv_cell);
    LPD_CHECK_ARG(keep_cells >= 0 && keep_cells <= LPD_ODOM_MAX_KEEP_CELLS, "lpd_map_crop: keep_cells=%d outside 0 .. 2^21", keep_cells);
    hipLaunchKernelGGL(crop_kernel, dim3((unsigned)((capacity_in + OD_T - 1) / OD_T)), dim3(OD_T), 0, stream, keys_in, acc_in, capacity_in, centre_pose,
                       origin, inv_cell, keep_cells, keys, acc, capacity, info);
    LPD_CHECK_LAUNCH("lpd_map_crop");
    return LPD_OK;
}

extern "C" int lpd_map_touch(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, int scan0, int scan1,
                             const double* origin, float inv_cell, const long long* keys, long long capacity, int reach, unsigned char* dirty,
                             void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && origin && keys && dirty, "lpd_map_touch: null pointer");
    LPD_CHECK_ARG(ld >= 3 && rows >= 1, "lpd_map_touch: bad dims ld=%d rows=%d (ld >= 3, rows >= 1)", ld, rows);
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_map_touch: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(scan0 >= 0 && scan0 < scan1 && scan1 <= S, "lpd_map_touch: scans %d .. %d outside 0 .. S=%d", scan0, scan1, S);
    LPD_CHECK_ARG(inv_cell >= LPD_MAP_INV_CELL_MIN && inv_cell <= LPD_MAP_INV_CELL_MAX, "lpd_map_touch: inv_cell=%g outside 1/16 .. 1024",
                  (double)inv_cell);
    LPD_CHECK_ARG(od_capacity_ok(capacity), "lpd_map_touch: capacity=%lld is not a power of two in 16 .. 2^36", capacity);
    LPD_CHECK_ARG(reach == 1 || reach == 2, "lpd_map_touch: reach=%d (1 or 2)", reach);
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
    LPD_CHECK_ARG(od_capacity_ok(capacity), "lpd_map_surface_touched: capacity=%lld is not a power of two in 16 .. 2^36", capacity);
    LPD_CHECK_ARG(reach == 1 || reach == 2, "lpd_map_surface_touched: reach=%d (1 or 2)", reach);
    const int cells = (2 * reach + 1) * (2 * reach + 1) * (2 * reach + 1);
    LPD_CHECK_ARG(min_cells >= 4 && min_cells <= cells, "lpd_map_surface_touched: min_cells=%d outside 4 .. %d", min_cells, cells);
    LPD_CHECK_ARG(((uintptr_t)surf & 15) == 0 && ((uintptr_t)dirty & 15) == 0, "lpd_map_surface_touched: surf and dirty must be 16-byte aligned");
    hipLaunchKernelGGL(refresh_kernel, dim3((unsigned)((capacity + OD_SPAN - 1) / OD_SPAN)), dim3(OD_T), 0, stream, keys, acc, capacity, reach, min_cells,
                       surf, dirty, info);
    LPD_CHECK_LAUNCH("lpd_map_surface_touched");
    return LPD_OK;
}
