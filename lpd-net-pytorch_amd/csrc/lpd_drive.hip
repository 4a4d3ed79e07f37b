// lpd_drive.hip -- submaps from a drive: posed scans cut by distance travelled into windows and brought into one frame per window.  What
// the reference's .bin submaps and its pointcloud_locations_20m_10overlap.csv come from, an offline step that is not part of it; this
// file is that step on the device.  Definition: include/lpd_hip.h; arithmetic: lpd_drive_math.h.
//
//   steps   one thread per scan: the float64 length of the step from the scan in front, quantised to 2^-16 m in an int64.  The
//           caller's torch.cumsum makes the distance D from it: integer sums, exact in any order.
//   plan    one thread per window: three lower bounds on D, rows = offsets[end] - offsets[first], the position as bit-copies.
//   rows    grid (chunk, window), DR_T = 256 threads, a chunk is LPD_DRIVE_CHUNK = 1024 consecutive rows of the window -- which are
//           consecutive rows of the input, because a window is a contiguous range of scans.  With ld == 3 a chunk is 12 KiB of
//           consecutive floats on both sides, whatever the row it starts at: it is copied global -> LDS -> global as a FLAT array with
//           16-byte accesses on the aligned body (at most three scalar elements at either end), and the transform runs on the LDS copy
//           in place, row j at floats 3 j .. 3 j + 2 (stride 3: no bank conflict).  ld == 4 with an aligned table: one 16-byte load
//           per row.  The relative poses of the chunk's scans are computed ONCE per workgroup in float64 by the first threads and kept
//           in LDS as fp32 (DR_CAP = 64 scans: a pushbroom chunk holds two or three, a sweep chunk one); each row finds its scan by a
//           binary search in the LDS copy of the chunk's offsets.  A chunk of more than DR_CAP scans (scans of a handful of rows)
//           lets every row compute its own relative pose with the same function: the same bits, by the slow road.  The copies, the
//           load, the search for the chunk's scans and the pose table are lpd_scan_chunk.h, shared with lpd_map_insert.
// No atomics.  Every index that becomes an address is checked against its table first: plan, out_off and offsets are the caller's
// device memory and may hold anything.
#include <math.h>

#include "lpd_common.h"
#include "lpd_drive_math.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int DR_T = 256;
constexpr int DR_CH = LPD_DRIVE_CHUNK;
constexpr int DR_R = DR_CH / DR_T;      // rows per thread
constexpr int DR_CAP = 64;              // relative poses a workgroup keeps in LDS
using Chunk = LpdScanChunk<DR_T, DR_CH, DR_CAP>;

__global__ __launch_bounds__(DR_T) void steps_kernel(const double* __restrict__ poses, int S, long long* __restrict__ q)
{
    const int i = blockIdx.x * DR_T + threadIdx.x;
    if (i >= S) return;
    q[i] = i == 0 ? 0 : (long long)lpd_drive_step(poses + (size_t)12 * (i - 1), poses + (size_t)12 * i);
}

__global__ __launch_bounds__(DR_T) void plan_kernel(const long long* __restrict__ D, int S, const int32_t* __restrict__ offsets,
                                                    const double* __restrict__ poses, long long L, long long T, long long w0, int W,
                                                    int32_t* __restrict__ plan, double* __restrict__ position)
{
    const int j = blockIdx.x * DR_T + threadIdx.x;
    if (j >= W) return;
    const LpdDriveWindow win = lpd_drive_window((const int64_t*)D, S, (int64_t)L, (int64_t)T, (int64_t)(w0 + j));
    // first <= end <= S: both index offsets [S+1]; the difference of two int32 in 64 bits, kept when it is an int32
    const long long n = (long long)offsets[win.end] - (long long)offsets[win.first];
    plan[4 * j + 0] = win.first;
    plan[4 * j + 1] = win.end;
    plan[4 * j + 2] = win.ref;
    plan[4 * j + 3] = win.ref >= 0 && n >= 0 && n < (1ll << 31) ? (int32_t)n : 0;
    const double* t = poses + (size_t)12 * (win.ref >= 0 ? win.ref : 0);      // ref < end <= S
    position[3 * j + 0] = win.ref >= 0 ? t[3] : 0.0;
    position[3 * j + 1] = win.ref >= 0 ? t[7] : 0.0;
    position[3 * j + 2] = win.ref >= 0 ? t[11] : 0.0;
}

__global__ __launch_bounds__(DR_T) void rows_kernel(const float* __restrict__ points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                    const double* __restrict__ poses, int S, const int32_t* __restrict__ plan,
                                                    const int32_t* __restrict__ out_off, int frame, int max_len, float* __restrict__ out)
{
    __shared__ float buf[3 * DR_CH];
    __shared__ LpdDriveRel rel[DR_CAP];
    __shared__ int32_t soff[DR_CAP + 1];
    __shared__ int span[2];
    const int w = blockIdx.y, tid = threadIdx.x, c0 = blockIdx.x * DR_CH;
    const int first = plan[4 * w + 0], end = plan[4 * w + 1], ref = plan[4 * w + 2], n = plan[4 * w + 3];
    // uniform over the workgroup: a window that is empty, longer than max_len, or whose plan is not one -- not written
    if (!(first >= 0 && first < end && end <= S && ref >= first && ref < end && n >= 1 && n <= max_len) || c0 >= n) return;
    const long long in0 = offsets[first], in1 = offsets[end], ob = out_off[w], oe = out_off[w + 1];
    if (!(in0 >= 0 && in1 - in0 == n && in1 <= rows && ob >= 0 && oe - ob == n)) return;
    const int cn = n - c0 < DR_CH ? n - c0 : DR_CH;      // rows of this chunk
    const long long g0 = in0 + c0;                       // its first input row; g0 + cn <= in1 <= rows
    Chunk::load(points, ld, g0, cn, buf, tid);
    Chunk::find_span(offsets, first, end, g0, cn, span, tid);
    __syncthreads();
    const int i_lo = span[0], i_hi = span[1] >= span[0] ? span[1] : span[0];      // first <= i_lo <= i_hi < end
    const int ns = i_hi - i_lo + 1;
    const double* Pr = poses + (size_t)12 * ref;
    const auto pose = [&](int i) { return lpd_drive_rel(poses + (size_t)12 * i, Pr, frame); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, pose);      // i_lo + ns = i_hi + 1 <= end <= S
    if (table) __syncthreads();
#pragma unroll
    for (int k = 0; k < DR_R; ++k) {
        const int j = k * DR_T + tid;
        if (j < cn) {
            const float x = buf[3 * j + 0], y = buf[3 * j + 1], z = buf[3 * j + 2];
            const LpdDriveRel r = Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, pose);
            buf[3 * j + 0] = lpd_drive_coord(r.m + 0, r.u[0], x, y, z);      // the row's own three floats: no other thread reads them
            buf[3 * j + 1] = lpd_drive_coord(r.m + 3, r.u[1], x, y, z);
            buf[3 * j + 2] = lpd_drive_coord(r.m + 6, r.u[2], x, y, z);
        }
    }
    __syncthreads();
    Chunk::copy_out(out + (size_t)(ob + c0) * 3, buf, 3 * cn, tid);
}

}  // namespace

extern "C" int lpd_drive_steps(const double* poses, int S, long long* q, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(poses && q, "lpd_drive_steps: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_drive_steps: S=%d outside 1 .. 2^22", S);
    hipLaunchKernelGGL(steps_kernel, dim3((S + DR_T - 1) / DR_T), dim3(DR_T), 0, stream, poses, S, q);
    LPD_CHECK_LAUNCH("lpd_drive_steps");
    return LPD_OK;
}

extern "C" int lpd_drive_plan(const long long* D, int S, const int32_t* offsets, const double* poses, long long L, long long T, long long w0, int W,
                              int32_t* plan, double* position, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(D && offsets && poses && plan && position, "lpd_drive_plan: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_drive_plan: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(L >= 1 && L <= LPD_DRIVE_MAX_UNITS && T >= 1 && T <= LPD_DRIVE_MAX_UNITS, "lpd_drive_plan: L=%lld T=%lld outside 1 .. 2^40", L, T);
    LPD_CHECK_ARG(W >= 1 && W <= LPD_DRIVE_MAX_WINDOWS, "lpd_drive_plan: W=%d outside 1 .. %d", W, LPD_DRIVE_MAX_WINDOWS);
    LPD_CHECK_ARG(w0 >= 0 && w0 + W <= LPD_DRIVE_MAX_WINDOW_NO, "lpd_drive_plan: windows w0=%lld .. w0+W=%lld outside 0 .. 2^22", w0, w0 + W);
    hipLaunchKernelGGL(plan_kernel, dim3((W + DR_T - 1) / DR_T), dim3(DR_T), 0, stream, D, S, offsets, poses, L, T, w0, W, plan, position);
    LPD_CHECK_LAUNCH("lpd_drive_plan");
    return LPD_OK;
}

extern "C" int lpd_drive_rows(const float* points, int ld, int rows, const int32_t* offsets, const double* poses, int S, const int32_t* plan, int W,
                              const int32_t* out_off, int frame, int max_len, float* out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && poses && plan && out_off && out, "lpd_drive_rows: null pointer");
    LPD_CHECK_ARG(ld >= 3 && rows >= 1, "lpd_drive_rows: bad dims ld=%d rows=%d (ld >= 3, rows >= 1)", ld, rows);
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_drive_rows: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(W >= 1 && W <= LPD_DRIVE_MAX_WINDOWS, "lpd_drive_rows: W=%d outside 1 .. %d", W, LPD_DRIVE_MAX_WINDOWS);
    LPD_CHECK_ARG(frame == 0 || frame == 1, "lpd_drive_rows: frame=%d (0 world axes, 1 the reference scan's frame)", frame);
    LPD_CHECK_ARG(max_len >= 1 && max_len <= LPD_DRIVE_MAX_POINTS, "lpd_drive_rows: max_len=%d outside 1 .. 2^20", max_len);
    LPD_CHECK_ARG((const void*)out != (const void*)points, "lpd_drive_rows: out must not alias points");
    hipLaunchKernelGGL(rows_kernel, dim3((max_len + DR_CH - 1) / DR_CH, W), dim3(DR_T), 0, stream, points, ld, rows, offsets, poses, S, plan, out_off,
                       frame, max_len, out);
    LPD_CHECK_LAUNCH("lpd_drive_rows");
    return LPD_OK;
}
