// lpd_deskew.hip -- motion compensation of LiDAR sweeps on the device: every row of the scan table brought into the frame of its
// sweep's reference time.  Definition: include/lpd_hip.h; arithmetic: lpd_deskew_math.h.
//
//   deskew   grid = the chunks of LPD_MAP_CHUNK = 1024 input rows, DK_T = 256 threads, the chunk found, checked and staged by the
//            prologue and loader that insert_kernel uses (lpd_scan_chunk.h: of_call, span_ok, load, poses, row_pose).  The staged
//            "pose" of a scan is LpdDeskewScan: the motion's quaternion with its sign chosen and its translation, made ONCE a chunk by
//            the first threads.  A row costs its time (one coalesced fp32 load), the blend (float64: one square root, four divisions,
//            some forty products and sums) and three float64 dot products; it is written back into its place in LDS, and the chunk
//            leaves as a flat array with 16-byte stores (copy_out).  A chunk reads all of its rows before it writes any and no two
//            chunks share a row, so out may be points itself when ld == 3.  A refused chunk is neither read nor written.
//   motions  one thread a scan: lpd_deskew_drive_motion.
// Integer atomics only (the two counters, one per wave); no barrier across workgroups; nothing is read back.  Every index that becomes
// an address is checked against its table first: rows by of_call, scans by span_ok.
#include <math.h>

#include "lpd_common.h"
#include "lpd_deskew_math.h"
#include "lpd_scan_chunk.h"

namespace {

constexpr int DK_T = 256;
constexpr int DK_CH = LPD_MAP_CHUNK;
constexpr int DK_R = DK_CH / DK_T;      // rows per thread
constexpr int DK_CAP = 64;              // scans whose part a workgroup keeps in LDS
using Chunk = LpdScanChunk<DK_T, DK_CH, DK_CAP>;
typedef unsigned long long u64;

// points and out carry no __restrict__: they may be one table
__global__ __launch_bounds__(DK_T) void deskew_kernel(const float* points, int ld, int rows, const int32_t* __restrict__ offsets,
                                                      const float* __restrict__ times, const double* __restrict__ motion, int scan0, int scan1,
                                                      double ref, float* out, long long* __restrict__ info)
{
    __shared__ float buf[3 * DK_CH];
    __shared__ LpdDeskewScan rel[DK_CAP];
    __shared__ int32_t soff[DK_CAP + 1];
    __shared__ int span[2];
    const int tid = threadIdx.x;
    long long g0;
    int cn, i_lo, i_hi;
    if (!Chunk::of_call(offsets, rows, scan0, scan1, &g0, &cn)) return;                           // uniform
    if (!Chunk::span_ok(offsets, scan0, scan1, g0, cn, span, tid, &i_lo, &i_hi)) return;          // not read, not written
    Chunk::load(points, ld, g0, cn, buf, tid);
    const int ns = i_hi - i_lo + 1;
    const auto scan = [&](int i) { return lpd_deskew_scan(motion + (size_t)12 * i); };
    const bool table = Chunk::poses(offsets, i_lo, ns, rel, soff, tid, scan);      // i_lo + ns = i_hi + 1 <= scan1
    __syncthreads();
    unsigned moved = 0, passed = 0;      // of this WAVE: the same in all its lanes
#pragma unroll 1
    for (int k = 0; k < DK_R; ++k) {
        const int j = k * DK_T + tid;
        int done = 0;
        if (j < cn) {
            const LpdDeskewScan s = Chunk::row_pose(table, rel, soff, offsets, i_lo, ns, g0 + j, scan);
            float o[3];
            done = lpd_deskew_row(s, times[g0 + j], ref, buf[3 * j + 0], buf[3 * j + 1], buf[3 * j + 2], o);
            buf[3 * j + 0] = o[0];      // the thread's own row: nobody else reads or writes it before the barrier
            buf[3 * j + 1] = o[1];
            buf[3 * j + 2] = o[2];
        }
        moved += (unsigned)__popcll(__ballot(j < cn && done));
        passed += (unsigned)__popcll(__ballot(j < cn && !done));
    }
    __syncthreads();
    Chunk::copy_out(out + (size_t)g0 * 3, buf, 3 * cn, tid);
    if ((tid & 63) == 0) {
        if (moved) atomicAdd((u64*)info + 0, (u64)moved);
        if (passed) atomicAdd((u64*)info + 1, (u64)passed);
    }
}

__global__ __launch_bounds__(DK_T) void motions_kernel(const double* __restrict__ poses, int S, double* __restrict__ motion)
{
    const int i = blockIdx.x * DK_T + threadIdx.x;
    if (i >= S) return;
    double o[12];
    lpd_deskew_drive_motion(poses, S, i, o);
    for (int k = 0; k < 12; ++k) motion[(size_t)12 * i + k] = o[k];
}

}  // namespace

extern "C" int lpd_scan_deskew(const float* points, int ld, int rows, const int32_t* offsets, const float* times, const double* motion, int S,
                               int scan0, int scan1, double ref, float* out, long long* info, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(points && offsets && times && motion && out && info, "lpd_scan_deskew: null pointer");
    LPD_CHECK_ARG(ld >= 3 && rows >= 1, "lpd_scan_deskew: bad dims ld=%d rows=%d (ld >= 3, rows >= 1)", ld, rows);
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_scan_deskew: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG(scan0 >= 0 && scan0 < scan1 && scan1 <= S, "lpd_scan_deskew: scans %d .. %d outside 0 .. S=%d", scan0, scan1, S);
    LPD_CHECK_ARG(ref >= 0.0 && ref <= 1.0, "lpd_scan_deskew: ref=%g outside 0 .. 1", ref);
    LPD_CHECK_ARG((const void*)out != (const void*)points || ld == 3, "lpd_scan_deskew: out may be points only when ld == 3 (ld=%d)", ld);
    hipLaunchKernelGGL(deskew_kernel, dim3((unsigned)(((long long)rows + DK_CH - 1) / DK_CH)), dim3(DK_T), 0, stream, points, ld, rows, offsets, times,
                       motion, scan0, scan1, ref, out, info);
    LPD_CHECK_LAUNCH("lpd_scan_deskew");
    return LPD_OK;
}

extern "C" int lpd_drive_motions(const double* poses, int S, double* motion, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(poses && motion, "lpd_drive_motions: null pointer");
    LPD_CHECK_ARG(S >= 1 && S <= LPD_DRIVE_MAX_SCANS, "lpd_drive_motions: S=%d outside 1 .. 2^22", S);
    LPD_CHECK_ARG((const void*)poses != (const void*)motion, "lpd_drive_motions: motion must not be poses");
    hipLaunchKernelGGL(motions_kernel, dim3((unsigned)((S + DK_T - 1) / DK_T)), dim3(DK_T), 0, stream, poses, S, motion);
    LPD_CHECK_LAUNCH("lpd_drive_motions");
    return LPD_OK;
}
