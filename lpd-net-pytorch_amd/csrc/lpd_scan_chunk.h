// lpd_scan_chunk.h -- one workgroup stages a chunk of the ragged scan table (points [rows][ld], offsets [S+1], one pose a scan): the
// steps that rows_kernel (lpd_drive.hip), insert_kernel (lpd_map.hip), touch_kernel (lpd_odom.hip), loc_pass_kernel
// (lpd_localize.hip) and deskew_kernel (lpd_deskew.hip, whose "pose" of a scan is the per-scan part of its motion) share.  HIP only.
// A chunk is cn <= CH consecutive rows of the table from row g0 on, which belong to the consecutive scans i_lo .. i_hi.  LpdScanChunk<T, CH, CAP> serves a workgroup of T threads that keeps CAP poses; the LDS arrays (buf
// [3 CH], rel [CAP], soff [CAP + 1], span [2]) are the kernel's and come in as pointers.  Nothing here knows which kernel calls it, what
// a pose is relative to, or what becomes of a row.
//
//   of_call    the chunk of workgroup blockIdx.x among the rows of the scans scan0 .. scan1-1 of a call (the rule of lpd_map_math.h) ->
//              g0 and cn, or false = nothing to do; both ways out are uniform.  rows_kernel cuts its windows from a plan instead.
//   span_ok    CONTAINS TWO BARRIERS: find_span, a barrier, lpd_map_chunk_ok with its loop shared among the threads, and the vote
//              (__syncthreads_or) -> i_lo, i_hi and whether the chunk is read.  What a kernel wrote to LDS before the call is visible
//              to all threads behind it; what becomes of a refused chunk is the kernel's.
//   load       the rows' coordinates into buf, row j at floats 3 j .. 3 j + 2 (stride 3: no bank conflict).  ld == 3: the chunk is
//              3 cn consecutive floats, copied as a FLAT array with 16-byte accesses on the aligned body (copy_in; copy_out is the way
//              back).  ld == 4 with a 16-byte aligned table: one 16-byte load a row.  Every other table by the float.
//   find_span  the scans of the chunk's first and last row into span[]: two waves, one search each.
//   poses      with ns = i_hi - i_lo + 1 <= CAP: rel[t] = pose(i_lo + t) and soff[t] = offsets[i_lo + t], made ONCE per workgroup by
//              the first threads; -> whether that table was made.
//   row_pose   the pose of row g: rel[its scan, found in soff] with the table, else pose(its scan, found in offsets) on the spot --
//              the same callable, so the same bits by the slow road (a chunk of more than CAP scans: scans of a handful of rows).
// Only span_ok meets a barrier: behind poses (and behind find_span, for a kernel that calls it itself) the kernel places one (uniformly,
// or inside the uniform `if (table)`), where its own steps between them want it.  Every index that becomes an address is the caller's
// to have checked: g0 + cn <= rows, and lo < hi <= S for the scans searched -- what of_call and span_ok do for the host's scan0 < scan1.
#pragma once
#include "lpd_common.h"
#include "lpd_drive_math.h"

template <int T, int CH, int CAP>
struct LpdScanChunk {
    static constexpr int R = CH / T;      // rows per thread

    // n floats global -> LDS (copy_in) or LDS -> global (copy_out): scalar elements up to the first 16-byte boundary of the GLOBAL
    // side, 16-byte accesses on the body, scalar elements behind it.  Nothing outside [g, g + n) is touched.
    static __device__ __forceinline__ int head(const float* g, int n)
    {
        const int h = (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u);
        return h < n ? h : n;
    }

    static __device__ __forceinline__ void copy_in(const float* __restrict__ g, float* s, int n, int tid)
    {
        const int h = head(g, n), body = (n - h) >> 2, tail0 = h + 4 * body;
        if (tid < h) s[tid] = g[tid];
        for (int v = tid; v < body; v += T) {
            const float4 a = *reinterpret_cast<const float4*>(g + h + 4 * v);
            float* d = s + h + 4 * v;
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
        }
        if (tid < n - tail0) s[tail0 + tid] = g[tail0 + tid];
    }

    static __device__ __forceinline__ void copy_out(float* __restrict__ g, const float* s, int n, int tid)
    {
        const int h = head(g, n), body = (n - h) >> 2, tail0 = h + 4 * body;
        if (tid < h) g[tid] = s[tid];
        for (int v = tid; v < body; v += T) {
            const float* d = s + h + 4 * v;
            *reinterpret_cast<float4*>(g + h + 4 * v) = make_float4(d[0], d[1], d[2], d[3]);
        }
        if (tid < n - tail0) g[tail0 + tid] = s[tail0 + tid];
    }

    static __device__ __forceinline__ void load(const float* __restrict__ points, int ld, long long g0, int cn, float* buf, int tid)
    {
        const float* src = points + (size_t)g0 * ld;
        if (ld == 3) {
            copy_in(src, buf, 3 * cn, tid);
        } else if (ld == 4 && ((uintptr_t)points & 15) == 0) {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int j = k * T + tid;
                if (j < cn) {
                    const float4 a = *reinterpret_cast<const float4*>(src + (size_t)j * 4);
                    buf[3 * j + 0] = a.x; buf[3 * j + 1] = a.y; buf[3 * j + 2] = a.z;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int j = k * T + tid;
                if (j < cn) {
                    const float* p = src + (size_t)j * ld;
                    buf[3 * j + 0] = p[0]; buf[3 * j + 1] = p[1]; buf[3 * j + 2] = p[2];
                }
            }
        }
    }

    // span[0], span[1] = the scans among lo .. hi-1 of rows g0 and g0 + cn - 1; both lie in [lo, hi-1] whatever offsets holds
    static __device__ __forceinline__ void find_span(const int32_t* __restrict__ offsets, int lo, int hi, long long g0, int cn, int* span, int tid)
    {
        if (tid == 0) span[0] = lpd_drive_scan_of(offsets, lo, hi, g0);
        if (tid == 64) span[1] = lpd_drive_scan_of(offsets, lo, hi, g0 + cn - 1);
    }

    // -> false: the call reads nothing, or this workgroup has no row.  Else cn = 1 .. CH rows from g0 on, all in [lo, hi) within [0, rows)
    static __device__ __forceinline__ bool of_call(const int32_t* __restrict__ offsets, int rows, int scan0, int scan1, long long* g0, int* cn)
    {
        const long long lo = offsets[scan0], hi = offsets[scan1];
        if (!(lo >= 0 && lo <= hi && hi <= rows)) return false;
        const long long c0 = (long long)blockIdx.x * CH;
        const long long a = c0 > lo ? c0 : lo, b = c0 + CH < hi ? c0 + CH : hi;
        if (a >= b) return false;
        *g0 = a;
        *cn = (int)(b - a);
        return true;
    }

    // BARRIERS INSIDE.  i_lo, i_hi: both in [scan0, scan1 - 1]; -> whether this part of the table is one, the same in every thread
    static __device__ __forceinline__ bool span_ok(const int32_t* __restrict__ offsets, int scan0, int scan1, long long g0, int cn, int* span,
                                                   int tid, int* i_lo, int* i_hi)
    {
        find_span(offsets, scan0, scan1, g0, cn, span, tid);
        __syncthreads();
        const int lo = span[0], hi = span[1];
        int bad = !(lo <= hi && (long long)offsets[lo] <= g0 && g0 + cn - 1 < (long long)offsets[hi + 1]);
        if (!bad)
            for (int i = lo + tid; i <= hi; i += T) bad |= offsets[i] > offsets[i + 1];
        *i_lo = lo;
        *i_hi = hi;
        return !__syncthreads_or(bad);
    }

    // pose(i) -> the record of scan i: an LpdDriveRel, or what else a kernel makes once a scan (Rec is the type of its LDS table).
    // Reads offsets[i_lo .. i_lo + ns]: i_lo + ns = i_hi + 1 <= S
    template <class Rec, class P>
    static __device__ __forceinline__ bool poses(const int32_t* __restrict__ offsets, int i_lo, int ns, Rec* rel, int32_t* soff, int tid, P&& pose)
    {
        if (ns > CAP) return false;
        if (tid < ns) rel[tid] = pose(i_lo + tid);
        if (tid <= ns) soff[tid] = offsets[i_lo + tid];
        return true;
    }

    template <class Rec, class P>
    static __device__ __forceinline__ Rec row_pose(bool table, const Rec* rel, const int32_t* soff, const int32_t* __restrict__ offsets, int i_lo,
                                                   int ns, long long g, P&& pose)
    {
        if (table) return rel[lpd_drive_scan_of(soff, 0, ns, g)];
        return pose(lpd_drive_scan_of(offsets, i_lo, i_lo + ns, g));
    }
};
