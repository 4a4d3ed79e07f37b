// lpd_scan_chunk.h -- one workgroup stages a chunk of the ragged scan table (points [rows][ld], offsets [S+1], one pose a scan): the
// steps that rows_kernel (lpd_drive.hip) and insert_kernel (lpd_map.hip) share.  HIP only.  A chunk is cn <= CH consecutive rows of
// the table from row g0 on, which belong to the consecutive scans i_lo .. i_hi.  LpdScanChunk<T, CH, CAP> serves a workgroup of T
// threads that keeps CAP poses; the LDS arrays (buf [3 CH], rel [CAP], soff [CAP + 1], span [2]) are the kernel's and come in as
// pointers.  Nothing here knows which kernel calls it, what a pose is relative to, or what becomes of a row.
//
//   load       the rows' coordinates into buf, row j at floats 3 j .. 3 j + 2 (stride 3: no bank conflict).  ld == 3: the chunk is
//              3 cn consecutive floats, copied as a FLAT array with 16-byte accesses on the aligned body (copy_in; copy_out is the way
//              back).  ld == 4 with a 16-byte aligned table: one 16-byte load a row.  Every other table by the float.
//   find_span  the scans of the chunk's first and last row into span[]: two waves, one search each.
//   poses      with ns = i_hi - i_lo + 1 <= CAP: rel[t] = pose(i_lo + t) and soff[t] = offsets[i_lo + t], made ONCE per workgroup by
//              the first threads; -> whether that table was made.
//   row_pose   the pose of row g: rel[its scan, found in soff] with the table, else pose(its scan, found in offsets) on the spot --
//              the same callable, so the same bits by the slow road (a chunk of more than CAP scans: scans of a handful of rows).
// None of these meets a barrier: the kernel places one behind find_span and one behind poses (uniformly, or inside the uniform
// `if (table)`), where its own steps between them want it.  Every index that becomes an address is the caller's to have checked:
// g0 + cn <= rows, and lo < hi <= S for the scans searched.
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

    // pose(i) -> LpdDriveRel of scan i.  Reads offsets[i_lo .. i_lo + ns]: i_lo + ns = i_hi + 1 <= S
    template <class P>
    static __device__ __forceinline__ bool poses(const int32_t* __restrict__ offsets, int i_lo, int ns, LpdDriveRel* rel, int32_t* soff, int tid,
                                                 P&& pose)
    {
        if (ns > CAP) return false;
        if (tid < ns) rel[tid] = pose(i_lo + tid);
        if (tid <= ns) soff[tid] = offsets[i_lo + tid];
        return true;
    }

    template <class P>
    static __device__ __forceinline__ LpdDriveRel row_pose(bool table, const LpdDriveRel* rel, const int32_t* soff,
                                                           const int32_t* __restrict__ offsets, int i_lo, int ns, long long g, P&& pose)
    {
        if (table) return rel[lpd_drive_scan_of(soff, 0, ns, g)];
        return pose(lpd_drive_scan_of(offsets, i_lo, i_lo + ns, g));
    }
};
