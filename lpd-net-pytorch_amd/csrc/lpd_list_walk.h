// lpd_list_walk.h -- one lane per point walks its kNN list once: the skeleton that local_features_kernel (lpd_feat.hip) and
// point_normals_kernel (lpd_icp.hip) share.  HIP only.  A kernel opens the walk (lpd_walk_open), hands lpd_walk a callable that
// receives every neighbour's centred difference in list order, and writes its results to row mrow(); its entry point asks
// lpd_walk_plan for the launch.  Nothing here knows which kernel calls it.
//
// Two forms of the neighbour read, same arithmetic, same bits:
//   LDS form  (N <= 4096)  the cloud's coordinates, 12 N bytes, are staged in LDS by each 512-thread block (48 KiB: three blocks per
//                          CU); the 3 K gathers of a lane are LDS reads.  A cloud with ldx == 3 on a 16-byte aligned base is one
//                          contiguous run of 3 N floats and is staged in 16-byte pieces, the tail and every other cloud by the float.
//   L2 form   (larger N)   the gathers go to global memory; a cloud's coordinates (48 N bytes of distinct lines at most) stay in L2,
//                          and Z-ordered clouds (lpd_morton_sort) make the lists of neighbouring lanes hit the same lines.
// The index lists are the only sizeable traffic (4 K bytes per point).  A list is a contiguous row: with K % 4 == 0 and a 16-byte
// aligned base the lane reads it as int4 pieces (each 64-byte line of a row is consumed by one lane in consecutive iterations and is
// fetched once); other K take 4-byte loads.  "Any list is legal": an index outside the cloud reads the cloud's last point instead of
// someone else's memory.
#pragma once
#include "lpd_common.h"

constexpr int LPD_WALK_LDS_MAX_N = 4096;      // 12 N bytes of LDS: 48 KiB
constexpr int LPD_WALK_T_LDS = 512, LPD_WALK_T_L2 = 256;

template <bool LDS>
constexpr int lpd_walk_threads = LDS ? LPD_WALK_T_LDS : LPD_WALK_T_L2;

struct LpdListWalk {
    const float* xc;         // the lane's cloud in global memory
    const int32_t* row;      // the lane's list
    size_t row0;             // b * N: the cloud's first row of every output (uniform over the block)
    int i;                   // the lane's point of the cloud
    float px, py, pz;        // the lane's own point
    int ldx;
    unsigned last;           // N - 1
    __device__ __forceinline__ size_t mrow() const { return row0 + i; }      // the lane's row of every output
};

__device__ __forceinline__ float* lpd_walk_lds()
{
    extern __shared__ __attribute__((aligned(16))) float lpd_walk_cloud[];      // [N][3] (LDS form)
    return lpd_walk_cloud;
}

template <bool LDS>
__device__ __forceinline__ void lpd_walk_point(const LpdListWalk& w, unsigned n, float& x, float& y, float& z)
{
    if (LDS) { const float* cloud = lpd_walk_lds(); x = cloud[3 * n]; y = cloud[3 * n + 1]; z = cloud[3 * n + 2]; }
    else { const float* pn = w.xc + (size_t)n * w.ldx; x = pn[0]; y = pn[1]; z = pn[2]; }
}

// Block blockIdx.x is tile blockIdx.x % tiles of cloud blockIdx.x / tiles.  The whole block stages the cloud (LDS form) and meets
// the barrier; -> false for a lane behind the cloud's last point, which leaves.
template <bool LDS>
__device__ __forceinline__ bool lpd_walk_open(LpdListWalk& w, const float* __restrict__ xyz, int ldx, const int32_t* __restrict__ idx, int N, int K)
{
    constexpr int T = lpd_walk_threads<LDS>;
    const int tiles = (N + T - 1) / T;
    const int b = blockIdx.x / tiles, i = (blockIdx.x % tiles) * T + (int)threadIdx.x;
    const float* xc = xyz + (size_t)b * N * ldx;
    w.xc = xc;      // what is uniform over the block is set on this side of the lanes' parting: it stays in scalar registers
    w.ldx = ldx;
    w.last = (unsigned)(N - 1);
    w.row0 = (size_t)b * N;
    if (LDS) {
        float* cloud = lpd_walk_lds();
        if (ldx == 3 && ((uintptr_t)xc & 15) == 0) {      // the cloud is one contiguous run of 3 N floats
            const int n4 = (3 * N) >> 2;
            for (int e = threadIdx.x; e < n4; e += T) reinterpret_cast<float4*>(cloud)[e] = reinterpret_cast<const float4*>(xc)[e];
            for (int e = 4 * n4 + threadIdx.x; e < 3 * N; e += T) cloud[e] = xc[e];
        } else {
            for (int p = threadIdx.x; p < N; p += T) {
                cloud[3 * p + 0] = xc[(size_t)p * ldx + 0];
                cloud[3 * p + 1] = xc[(size_t)p * ldx + 1];
                cloud[3 * p + 2] = xc[(size_t)p * ldx + 2];
            }
        }
        __syncthreads();
    }
    if (i >= N) return false;
    w.i = i;
    lpd_walk_point<LDS>(w, (unsigned)i, w.px, w.py, w.pz);
    w.row = idx + w.mrow() * K;
    return true;
}

// f(j, dx, dy, dz) for j = 0 .. kmax - 1 in list order: (dx, dy, dz) = the j-th neighbour minus the lane's own point.  vec4: the
// host's word that a row may be read as int4 pieces (lpd_walk_plan).  INLINE4 is the kernel's choice by the size of its callable:
// true inlines it four times a group, straight-line (a small body); false keeps it once, in a loop of one entry that selects the
// entry's coordinates (a large body, four copies of which would crowd the registers and the instruction cache).
template <bool LDS, bool INLINE4, class F>
__device__ __forceinline__ void lpd_walk(const LpdListWalk& w, int kmax, int vec4, F&& f)
{
    for (int j0 = 0; j0 < kmax; j0 += 4) {
        int4 q;
        if (vec4) q = *reinterpret_cast<const int4*>(w.row + j0);      // K % 4 == 0: j0 + 3 < K
        else {
            q.x = w.row[j0];
            q.y = j0 + 1 < kmax ? w.row[j0 + 1] : 0;
            q.z = j0 + 2 < kmax ? w.row[j0 + 2] : 0;
            q.w = j0 + 3 < kmax ? w.row[j0 + 3] : 0;
        }
        const unsigned nn[4] = {min((unsigned)q.x, w.last), min((unsigned)q.y, w.last), min((unsigned)q.z, w.last), min((unsigned)q.w, w.last)};
        float cx[4], cy[4], cz[4];      // the four gathers are issued together; f is called in list order
#pragma unroll
        for (int t = 0; t < 4; ++t) lpd_walk_point<LDS>(w, nn[t], cx[t], cy[t], cz[t]);
        if constexpr (INLINE4) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (j0 + t < kmax) f(j0 + t, cx[t] - w.px, cy[t] - w.py, cz[t] - w.pz);
        } else {
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                const int j = j0 + t;
                if (j >= kmax) break;
                const float nx = t == 0 ? cx[0] : t == 1 ? cx[1] : t == 2 ? cx[2] : cx[3];
                const float ny = t == 0 ? cy[0] : t == 1 ? cy[1] : t == 2 ? cy[2] : cy[3];
                const float nz = t == 0 ? cz[0] : t == 1 ? cz[1] : t == 2 ? cz[2] : cz[3];
                f(j, nx - w.px, ny - w.py, nz - w.pz);
            }
        }
    }
}

// The launch of a walk over B clouds of N points with lists of K entries at idx.  force_l2: the caller's LPD_DEBUG switch.
struct LpdWalkPlan {
    bool lds;
    int threads, vec4;
    long long blocks;      // the caller refuses 2^31 and more
    size_t lds_bytes;
};

inline LpdWalkPlan lpd_walk_plan(const int32_t* idx, int B, int N, int K, bool force_l2)
{
    LpdWalkPlan p;
    p.lds = N <= LPD_WALK_LDS_MAX_N && !force_l2;
    p.threads = p.lds ? LPD_WALK_T_LDS : LPD_WALK_T_L2;
    p.blocks = (long long)B * ((N + p.threads - 1) / p.threads);
    p.vec4 = (K % 4 == 0 && ((uintptr_t)idx & 15) == 0) ? 1 : 0;
    p.lds_bytes = p.lds ? (size_t)N * 3 * sizeof(float) : 0;
    return p;
}
