// lpd_icp.hip -- a verified place match refined to a full 6-DoF pose: unit normals of a cloud from its kNN lists (lpd_point_normals)
// and trimmed point-to-plane ICP of (query, candidate) pairs (lpd_icp_pairs).  Definition: include/lpd_hip.h; arithmetic:
// lpd_icp_math.h.  What stands between lpd_align_pairs' yaw and shift and a loop-closure constraint, without copying a cloud back.
//
// point_normals_kernel   one lane per point, the lane walks its list once (lpd_list_walk.h, the walk of lpd_feat.hip: the cloud in
//                        LDS or through L2) adding the moments (lpd_feat_add), then the three-row Jacobi.
// icp_init_kernel        one thread per pair: the pair's validity, info = (1 | -1, 0, 0, 0) and the fp32 pose into ws.
// icp_pass_kernel        THE HOT PATH: N x N distance evaluations per pair and pass, in the order the definition fixes (no MFMA: a
//                        -2 a.b expansion loses the bits).  IC_T = 256 threads = 4 waves, one workgroup per (pair, chunk of IC_CHUNK =
//                        64 points of A).  THE LANES ARE A's POINTS, and the four waves hold the same 64 points: B's scaled points are
//                        staged in LDS as three planes, IC_TILE = 4096 points a tile (48 KiB; larger clouds stream tiles through it),
//                        and wave w takes the groups of four consecutive j numbered w, w + 4, w + 8 ... of the tile: every lane of a
//                        wave reads the same three 16-byte words (a broadcast: no bank conflict), 8 VALU operations a candidate plus
//                        the compare and two selects, the running minimum in registers.  A wave meets its candidates in ascending j
//                        and takes a later one only when strictly nearer; the four waves' minima are combined as the integer minimum
//                        of (bits of d2) << 32 | j -- d2 is not negative, so the order of the bits is the order of the values, and a
//                        tie goes to the lowest j.  One wave per pair-chunk instead would leave P = 1 at N = 4096 with 64 waves on a
//                        chip of 1024 SIMDs; this way it has 256, and P = 25 fills the chip.
//                        Wave 0 then decides the correspondence, forms the quantised row and the 29 terms of lpd_icp_math.h, sums them
//                        over the wave and adds them to sums [pass][pair] with 64-bit integer atomics: exact, so the same bits in any
//                        order.  The call clears `sums` first (one memset).
// icp_step_kernel        one thread per pair: lpd_icp_solve in float64 on the pass's sums, the pose and info updated in place, the fp32
//                        pose of the next pass into ws.  Behind the last pass it only writes info [3].
// iters + 1 pass launches, iters + 1 step launches, one init and one memset; nothing synchronises.
#include <math.h>

#include "lpd_common.h"
#include "lpd_icp_math.h"
#include "lpd_list_walk.h"

namespace {

template <bool LDS>
__global__ __launch_bounds__(lpd_walk_threads<LDS>) void point_normals_kernel(const float* __restrict__ xyz, int ldx,
                                                                              const int32_t* __restrict__ idx, int N, int K,
                                                                              float* __restrict__ normals, float* __restrict__ flatness,
                                                                              int vec4)
{
    LpdListWalk w;
    if (!lpd_walk_open<LDS>(w, xyz, ldx, idx, N, K)) return;
    LpdFeatMoments m;
    lpd_feat_init(m);
    lpd_walk<LDS, true>(w, K, vec4, [&](int, float dx, float dy, float dz) { lpd_feat_add(m, dx, dy, dz); });
    float n3[3], flat;
    lpd_icp_normal(m, K, n3, &flat);
    const size_t mrow = w.mrow();
    normals[3 * mrow] = n3[0];
    normals[3 * mrow + 1] = n3[1];
    normals[3 * mrow + 2] = n3[2];
    if (flatness) flatness[mrow] = flat;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int IC_T = 256;
constexpr int IC_WAVES = IC_T / 64;
constexpr int IC_CHUNK = 64;            // points of A per workgroup
constexpr int IC_TILE = 4096;           // points of B per LDS tile: three planes of 16 KiB
static_assert(IC_TILE % 4 == 0 && IC_CHUNK == 64, "a group is four candidates; a chunk is one wave of lanes");

struct IcState { float m[9], u[3]; int32_t valid, pad[3]; };      // ws [P]: 64 bytes a pair
static_assert(sizeof(IcState) == 64, "the workspace is 64 bytes a pair");

struct IcK { int TA, TB, N, P, chunks; };

__device__ __forceinline__ bool ic_pair_ok(const int32_t* __restrict__ pairs, int p, int TA, int TB, int* ra, int* rb)
{
    *ra = pairs[2 * p];
    *rb = pairs[2 * p + 1];
    return *ra >= 0 && *ra < TA && *rb >= 0 && *rb < TB;
}

__device__ __forceinline__ void ic_store_state(IcState* __restrict__ st, const double* __restrict__ pose)
{
    const LpdIcpPose32 T = lpd_icp_pose32(pose);
#pragma unroll
    for (int e = 0; e < 9; ++e) st->m[e] = T.m[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) st->u[e] = T.u[e];
}

__global__ __launch_bounds__(IC_T) void icp_init_kernel(const int32_t* __restrict__ pairs, IcK K, const double* __restrict__ pose,
                                                        int32_t* __restrict__ info, IcState* __restrict__ ws)
{
    const int p = blockIdx.x * IC_T + threadIdx.x;
    if (p >= K.P) return;
    int ra, rb;
    const bool ok = ic_pair_ok(pairs, p, K.TA, K.TB, &ra, &rb);
    info[4 * (size_t)p] = ok ? 1 : -1;
    info[4 * (size_t)p + 1] = info[4 * (size_t)p + 2] = info[4 * (size_t)p + 3] = 0;
    ws[p].valid = ok ? 1 : 0;
    if (ok) ic_store_state(ws + p, pose + 12 * (size_t)p);
}

__device__ __forceinline__ long long ic_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(IC_T) void icp_pass_kernel(const float* __restrict__ A, const float* __restrict__ scaleA,
                                                        const float* __restrict__ B, const float* __restrict__ scaleB,
                                                        const float* __restrict__ normalsB, const int32_t* __restrict__ pairs, IcK K,
                                                        const IcState* __restrict__ ws, float dmax, long long* __restrict__ sums,
                                                        int32_t* __restrict__ nn)
{
    __shared__ __align__(16) float Bx[IC_TILE], By[IC_TILE], Bz[IC_TILE];
    __shared__ unsigned long long wkey[IC_WAVES][IC_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x / K.chunks, ch = blockIdx.x - p * K.chunks;
    const int N = K.N;
    const int i = ch * IC_CHUNK + lane;
    const IcState st = ws[p];
    if (!st.valid) {      // uniform over the workgroup: nothing of the tables is read
        if (nn && wave == 0 && i < N) nn[(size_t)p * N + i] = -1;
        return;
    }
    const int ra = pairs[2 * p], rb = pairs[2 * p + 1];
    const float* pb = B + (size_t)rb * N * 3;
    const float sb = scaleB ? scaleB[rb] : 1.0f;
    LpdIcpPose32 T;
#pragma unroll
    for (int e = 0; e < 9; ++e) T.m[e] = st.m[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) T.u[e] = st.u[e];
    float pt[3] = {NAN, NAN, NAN};
    bool live = false;
    if (i < N) {
        const float* pa = A + ((size_t)ra * N + i) * 3;
        live = lpd_icp_transform(T, pa[0], pa[1], pa[2], scaleA ? scaleA[ra] : 1.0f, pt);
    }
    const float px = pt[0], py = pt[1], pz = pt[2];
    float best = INFINITY;
    int bj = -1;
    for (int t0 = 0; t0 < N; t0 += IC_TILE) {
        const int cnt = min(IC_TILE, N - t0), cnt4 = (cnt + 3) & ~3;
        if (t0) __syncthreads();      // the tile before has been read by every wave
        for (int j = tid; j < cnt4; j += IC_T) {
            const bool in = j < cnt;      // the last group is filled with NaN: never nearer
            const float* q = pb + (size_t)(t0 + (in ? j : 0)) * 3;
            Bx[j] = in ? q[0] * sb : NAN;
            By[j] = in ? q[1] * sb : NAN;
            Bz[j] = in ? q[2] * sb : NAN;
        }
        __syncthreads();
        const int groups = cnt4 >> 2;
#pragma unroll 2
        for (int g = wave; g < groups; g += IC_WAVES) {
            const float4 qx = reinterpret_cast<const float4*>(Bx)[g];
            const float4 qy = reinterpret_cast<const float4*>(By)[g];
            const float4 qz = reinterpret_cast<const float4*>(Bz)[g];
            const int j0 = t0 + 4 * g;
            const float d0 = lpd_icp_d2(qx.x, qy.x, qz.x, px, py, pz);
            const float d1 = lpd_icp_d2(qx.y, qy.y, qz.y, px, py, pz);
            const float d2 = lpd_icp_d2(qx.z, qy.z, qz.z, px, py, pz);
            const float d3 = lpd_icp_d2(qx.w, qy.w, qz.w, px, py, pz);
            if (lpd_icp_nearer(d0, best)) { best = d0; bj = j0; }
            if (lpd_icp_nearer(d1, best)) { best = d1; bj = j0 + 1; }
            if (lpd_icp_nearer(d2, best)) { best = d2; bj = j0 + 2; }
            if (lpd_icp_nearer(d3, best)) { best = d3; bj = j0 + 3; }
        }
    }
    // (+inf, -1) = 0x7F800000'FFFFFFFF is above every key of a candidate: best < +inf there
    wkey[wave][lane] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bj;
    __syncthreads();
    if (wave != 0) return;
    unsigned long long key = wkey[0][lane];
#pragma unroll
    for (int w = 1; w < IC_WAVES; ++w) key = wkey[w][lane] < key ? wkey[w][lane] : key;
    const int js = (int)(unsigned)(key & 0xFFFFFFFFull);
    const float dbest = __uint_as_float((unsigned)(key >> 32));
    bool has = live && js >= 0 && js < N && lpd_icp_within(dbest, dmax);
    long long t[LPD_ICP_SUMS];
#pragma unroll
    for (int e = 0; e < LPD_ICP_SUMS; ++e) t[e] = 0;
    if (has) {
        const float* nb = normalsB + ((size_t)rb * N + js) * 3;
        const float n3[3] = {nb[0], nb[1], nb[2]};
        has = !lpd_icp_normal_zero(n3[0], n3[1], n3[2]);
        if (has) {
            const float* qb = pb + (size_t)js * 3;
            const float q3[3] = {qb[0] * sb, qb[1] * sb, qb[2] * sb};
            int64_t Ji[6], ri, tt[LPD_ICP_SUMS];
            lpd_icp_row(pt, q3, n3, Ji, &ri);
            lpd_icp_terms(Ji, ri, tt);
#pragma unroll
            for (int e = 0; e < 29; ++e) t[e] = (long long)tt[e];
        }
    }
    if (nn && i < N) nn[(size_t)p * N + i] = has ? js : -1;
    if (__ballot(has) == 0ull) return;      // uniform over the wave
    long long mine = 0;      // lane e keeps sum e: the butterfly leaves the total in every lane
#pragma unroll
    for (int e = 0; e < 29; ++e) {
        const long long s = ic_wave_sum(t[e]);
        mine = lane == e ? s : mine;
    }
    if (lane < 29 && mine != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(sums + (size_t)p * LPD_ICP_SUMS + lane), (unsigned long long)mine);
}

__global__ __launch_bounds__(IC_T) void icp_step_kernel(IcK K, int step, int min_inliers, const long long* __restrict__ sums,
                                                        double* __restrict__ pose, int32_t* __restrict__ info, IcState* __restrict__ ws)
{
    const int p = blockIdx.x * IC_T + threadIdx.x;
    if (p >= K.P || !ws[p].valid) return;
    int64_t s[LPD_ICP_SUMS];
#pragma unroll
    for (int e = 0; e < 29; ++e) s[e] = (int64_t)sums[(size_t)p * LPD_ICP_SUMS + e];
    int32_t* o = info + 4 * (size_t)p;
    if (!step) {
        o[3] = (int32_t)s[LPD_ICP_SUM_M];
        return;
    }
    double P12[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P12[e] = pose[12 * (size_t)p + e];
    if (lpd_icp_solve(s, min_inliers, P12)) {
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[12 * (size_t)p + e] = P12[e];
        ic_store_state(ws + p, P12);
        o[1] += 1;
    } else {
        o[2] += 1;
    }
}

inline bool ic_dims_ok(int P, int N, int iters)
{
    return P >= 1 && P <= LPD_ICP_MAX_PAIRS && N >= 1 && N <= LPD_ICP_MAX_POINTS && iters >= 0 && iters <= LPD_ICP_MAX_ITERS;
}

}  // namespace

extern "C" int lpd_point_normals(const float* xyz, int ldx, const int32_t* idx, int B, int N, int K, float* normals, float* flatness,
                                 void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(xyz && idx && normals, "lpd_point_normals: null pointer");
    LPD_CHECK_ARG(B > 0 && N > 0 && ldx >= 3, "lpd_point_normals: bad dims B=%d N=%d ldx=%d", B, N, ldx);
    LPD_CHECK_ARG(K >= 4 && K <= 64 && K <= N, "lpd_point_normals: need 4 <= K <= 64 and K <= N (K=%d N=%d)", K, N);
    LPD_CHECK_ARG((long long)B * N < (1ll << 31), "lpd_point_normals: B * N = %lld rows exceed 2^31", (long long)B * N);
    LPD_CHECK_ARG((const void*)normals != (const void*)xyz && (const void*)flatness != (const void*)xyz, "lpd_point_normals: an output aliases xyz");
    // A/B switch, read on every call (a test flips it inside one process): LPD_DEBUG=normals-l2 sends every cloud through the L2 form
    const LpdWalkPlan plan = lpd_walk_plan(idx, B, N, K, lpd_debug("normals-l2", 0) != 0);
    LPD_CHECK_ARG(plan.blocks < (1ll << 31), "lpd_point_normals: grid of %lld blocks", plan.blocks);
    hipLaunchKernelGGL(plan.lds ? point_normals_kernel<true> : point_normals_kernel<false>, dim3((unsigned)plan.blocks), dim3(plan.threads),
                       plan.lds_bytes, stream, xyz, ldx, idx, N, K, normals, flatness, plan.vec4);
    LPD_CHECK_LAUNCH("lpd_point_normals");
    return LPD_OK;
}

extern "C" long long lpd_icp_workspace_bytes(int P, int N, int iters)
{
    return ic_dims_ok(P, N, iters) ? (long long)P * (long long)sizeof(IcState) : 0;
}

extern "C" int lpd_icp_pairs(const float* A, int TA, const float* scaleA, const float* B, int TB, const float* scaleB, const float* normalsB,
                             int N, const int32_t* pairs, int P, const float* dmax, int iters, int min_inliers, double* pose, int32_t* info,
                             long long* sums, int32_t* nn, void* ws, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    LPD_CHECK_ARG(A && B && normalsB && pairs && dmax && pose && info && sums, "lpd_icp_pairs: null pointer");
    LPD_CHECK_ARG(TA >= 1 && TB >= 1 && N >= 1 && N <= LPD_ICP_MAX_POINTS, "lpd_icp_pairs: bad dims TA=%d TB=%d N=%d (>= 1, N <= %d)", TA, TB, N,
                  LPD_ICP_MAX_POINTS);
    LPD_CHECK_ARG(P >= 1 && P <= LPD_ICP_MAX_PAIRS, "lpd_icp_pairs: P=%d outside 1 .. 2^20", P);
    LPD_CHECK_ARG(iters >= 0 && iters <= LPD_ICP_MAX_ITERS, "lpd_icp_pairs: iters=%d outside 0 .. %d", iters, LPD_ICP_MAX_ITERS);
    LPD_CHECK_ARG(min_inliers >= LPD_ICP_MIN_INLIERS, "lpd_icp_pairs: min_inliers=%d below %d", min_inliers, LPD_ICP_MIN_INLIERS);
    for (int s = 0; s <= iters; ++s)
        LPD_CHECK_ARG(lpd_icp_finite(dmax[s]) && dmax[s] > 0.0f && dmax[s] <= LPD_ICP_MAX_DMAX, "lpd_icp_pairs: dmax[%d]=%g (finite, > 0, <= %g)", s,
                      (double)dmax[s], (double)LPD_ICP_MAX_DMAX);
    LPD_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "lpd_icp_pairs: the workspace (lpd_icp_workspace_bytes, 16-byte aligned) is missing");
    IcK K;
    K.TA = TA; K.TB = TB; K.N = N; K.P = P;
    K.chunks = (N + IC_CHUNK - 1) / IC_CHUNK;      // <= 256, P <= 2^20: the grid stays below 2^31
    const size_t per_pass = (size_t)P * LPD_ICP_SUMS;
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)(iters + 1) * per_pass * sizeof(long long), stream);
    if (e != hipSuccess) {
        lpd_set_error("lpd_icp_pairs: clearing the sums failed: %s", hipGetErrorString(e));
        return LPD_ERR_LAUNCH;
    }
    const unsigned pblocks = (unsigned)((P + IC_T - 1) / IC_T);
    IcState* st = (IcState*)ws;
    hipLaunchKernelGGL(icp_init_kernel, dim3(pblocks), dim3(IC_T), 0, stream, pairs, K, (const double*)pose, info, st);
    for (int s = 0; s <= iters; ++s) {
        long long* ss = sums + (size_t)s * per_pass;
        hipLaunchKernelGGL(icp_pass_kernel, dim3((unsigned)((long long)P * K.chunks)), dim3(IC_T), 0, stream, A, scaleA, B, scaleB, normalsB, pairs,
                           K, (const IcState*)st, dmax[s], ss, s == iters ? nn : (int32_t*)nullptr);
        hipLaunchKernelGGL(icp_step_kernel, dim3(pblocks), dim3(IC_T), 0, stream, K, s < iters ? 1 : 0, min_inliers, (const long long*)ss, pose,
                           info, st);
    }
    LPD_CHECK_LAUNCH("lpd_icp_pairs");
    return LPD_OK;
}
